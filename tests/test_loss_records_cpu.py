"""The records the loss path passes around, on CPU tensors: ring slots and their generations (a backward must never read
another batch's rows), the gathered-rows record without a process group, the pending prefetch (taken only by the forward it
was made for, and waited for exactly once) and the argument checks of `as_rows`.  Also: `engine` still exports the CLIP
schedule that lives in `clip.py`."""
import weakref

import pytest
import torch

B, C, T = 2, 8, 5


def _loss():
    from speech_decoding_amd import loss
    return loss


def _take(state, key="k", shape=(B, C, T), dtype=torch.float32):
    return _loss()._ring_rows(state, key, *shape, dtype, "cpu")


# ---------------------------------------------------------------------------------------------------- rings
def test_ring_slot_is_valid_until_its_buffer_is_handed_out_again():
    state = _loss().LossState()
    state.ring_depth = 2
    a, b, c = _take(state), _take(state), _take(state)
    assert not a.valid() and b.valid() and c.valid()
    assert c.buf is a.buf and b.buf is not a.buf
    assert (a.gen, b.gen, c.gen) == (1, 1, 2)
    ring = next(iter(state.rings.values()))
    assert a.ring is ring and ring.bufs == [a.buf, b.buf] and ring.gens == [2, 1] and ring.next == 3


def test_another_shape_or_dtype_gets_a_ring_of_its_own():
    state = _loss().LossState()
    a = _take(state)
    assert _take(state, shape=(B + 1, C, T)).ring is not a.ring
    assert _take(state, shape=(B, C, T + 1)).ring is not a.ring
    assert _take(state, dtype=torch.bfloat16).ring is not a.ring
    assert _take(state, key="other").ring is not a.ring
    assert len(state.rings) == 5 and a.valid()
    assert _take(state).ring is a.ring


def test_the_ninth_key_evicts_the_oldest_ring_and_old_slots_answer_from_their_own():
    state = _loss().LossState()
    first = _take(state, key=0)
    for k in range(1, 8):
        _take(state, key=k)
    assert len(state.rings) == 8 and first.ring in state.rings.values()
    _take(state, key=8)
    assert len(state.rings) == 8 and first.ring not in state.rings.values()
    assert [k[0] for k in state.rings] == list(range(1, 9))                # oldest first
    assert first.valid()                                   # nobody can hand the evicted ring's buffer out again
    again = _take(state, key=0)                            # a new ring under the old key
    assert again.ring is not first.ring and again.buf is not first.buf and first.valid()


def test_ring_depth_is_read_when_a_ring_is_created():
    state = _loss().LossState()
    state.ring_depth = 3
    a = _take(state)
    state.ring_depth = 1
    assert len(a.ring.bufs) == 3
    _take(state), _take(state)
    assert a.valid()
    assert _take(state).buf is a.buf and not a.valid()
    assert len(_take(state, key="later").ring.bufs) == 1


# ---------------------------------------------------------------------------------------------------- gather without a group
def test_gather_without_a_group_hands_back_the_callers_rows_slot_and_norms(monkeypatch):
    loss = _loss()
    from speech_decoding_amd import lib as L, ops
    slot = _take(loss.LossState())
    rows, sq = ops.new_rows(B, T, L.pad_channels(C), torch.float32, "cpu"), torch.arange(float(B))

    def boom(*a, **k):
        raise AssertionError("norms were handed in: no kernel may run")
    monkeypatch.setattr(ops, "rows_sumsq", boom)
    g = loss.gather_speech_rows(rows, B, T, None, slot=slot, sq=sq)
    assert g.rows is rows and g.sq is sq and g.slot is slot
    assert g.n == B and g.col0 == 0 and len(g.works) == 0 and g.done is None
    g.wait()                                               # nothing to wait for


def test_gather_without_a_group_takes_the_norms_it_was_not_given(monkeypatch):
    loss = _loss()
    from speech_decoding_amd import lib as L, ops
    rows, sq, seen = ops.new_rows(B, T, L.pad_channels(C), torch.float32, "cpu"), torch.ones(B), []
    monkeypatch.setattr(ops, "rows_sumsq", lambda *a: seen.append(a) or sq)
    g = loss.gather_speech_rows(rows, B, T, None)
    row_elems = L.rows_tp(T) * rows.shape[1]
    assert g.sq is sq and g.rows is rows and g.slot is None and g.n == B
    assert len(seen) == 1 and seen[0][0] is rows and seen[0][1:] == (B, row_elems, row_elems)


# ---------------------------------------------------------------------------------------------------- pending prefetch
class _Work:
    def __init__(self):
        self.waits = 0

    def wait(self):
        self.waits += 1


def _pending(state, Y, dtype=torch.float32):
    loss = _loss()
    works = [_Work(), _Work()]
    g = loss.GatheredRows(torch.zeros(4, 8), torch.zeros(2), 2, 0, None, works, None)
    state.pending = loss.Pending(weakref.ref(Y), dtype, g)
    return g, works


def test_a_prefetch_is_taken_only_for_its_own_tensor_and_dtype():
    loss = _loss()
    state, Y = loss.LossState(), torch.zeros(2, 8, 5)
    g, works = _pending(state, Y)
    assert loss._take_prefetched(state, Y.clone(), torch.float32) is None          # equal content, another tensor
    assert loss._take_prefetched(state, Y, torch.bfloat16) is None
    assert state.pending is not None and state.pending.rows is g and [w.waits for w in works] == [0, 0]
    assert loss._take_prefetched(state, Y, torch.float32) is g
    assert state.pending is None and [w.waits for w in works] == [1, 1]
    assert loss._take_prefetched(state, Y, torch.float32) is None
    assert [w.waits for w in works] == [1, 1]


def test_drain_waits_for_each_collective_once_and_drops_the_prefetch():
    loss = _loss()
    state, Y = loss.LossState(), torch.zeros(2, 8, 5)
    _, works = _pending(state, Y)
    state.drain()
    assert state.pending is None and [w.waits for w in works] == [1, 1]
    state.drain()                                          # nothing pending: a no-op
    assert state.pending is None and [w.waits for w in works] == [1, 1]
    _, works = _pending(state, Y)
    _take(state)
    state.clear()                                          # release_buffers: drains first, then drops the rings
    assert state.pending is None and not state.rings and [w.waits for w in works] == [1, 1]


# ---------------------------------------------------------------------------------------------------- as_rows
def test_as_rows_rejects_a_wrong_shape_and_a_host_tensor():
    loss = _loss()
    from speech_decoding_amd import SdaError
    with pytest.raises(ValueError, match=r"^Z: expected shape \(2, 8, 5\), got \(2, 8, 6\)$"):
        loss.as_rows(torch.zeros(2, 8, 6), B, C, T, torch.float32, "Z")
    with pytest.raises(SdaError, match=r"^Z must live on the MI355X device \(there is no CPU path\)$"):
        loss.as_rows(torch.zeros(B, C, T), B, C, T, torch.float32, "Z")
    state = loss.LossState()                               # the ring-backed pack checks the same, before it takes a slot
    with pytest.raises(ValueError, match=r"^x: expected shape \(2, 8, 5\), got \(3, 8, 5\)$"):
        loss._pack_ring(state, torch.zeros(3, 8, 5), B, C, T, torch.float32, "x", "loss.Y")
    with pytest.raises(SdaError, match=r"^x must live on the MI355X device"):
        loss._pack_ring(state, torch.zeros(B, C, T), B, C, T, torch.float32, "x", "loss.Y")
    assert not state.rings


# ---------------------------------------------------------------------------------------------------- the old import names
@pytest.mark.parametrize("name", ["ClipCtx", "ClipBlockStats", "clip_forward", "clip_block_stats", "clip_block_finish",
                                  "clip_backward", "clip_backward_y"])
def test_engine_still_exports_the_clip_schedule(name):
    from speech_decoding_amd import clip, engine
    assert getattr(engine, name) is getattr(clip, name)
    assert getattr(clip, name).__module__ == "speech_decoding_amd.clip"


def test_the_loss_calls_the_schedule_through_clip():
    loss = _loss()
    from speech_decoding_amd import clip
    assert loss.clip is clip and not hasattr(loss, "E") and not hasattr(loss, "engine")
