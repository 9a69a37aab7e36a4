"""Decoding against windows of continuous speech tracks on the MI355X (retrieval.WindowBank, sda_sim_gemm_windows,
sda_window_sumsq).

Yardsticks.  Exact regime (tests/window_bank_cases.py: integer operands, every dot product and norm below 2^24): the same
candidates cut out on the host and materialised into a SpeechBank, bit for bit, and the numpy restatement whose planted bugs
test_window_bank_cpu.py tells apart.  Real operands: the float64 cosine of the same rounded operands under the tie-tolerant
checks and the TOL = 1e-4 of tests/test_retrieval_gpu.py (the project's exact-path tolerance), no row skipped.

Measured on the MI355X, max |score - fp64 score| over both cases: bf16 1.1e-6, fp16 1.2e-6 (printed by
test_real_operands_against_float64; the checks use TOL, not these).
"""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from tests import window_bank_cases as W      # noqa: E402

DEV = "cuda:0"
DT = {"bf16": torch.bfloat16, "fp16": torch.float16}
TOL = 1e-4
SMALL_SCRATCH = 64 << 10      # case a: all 5 queries in one block, 256 candidates per chunk; case b: 64 queries per block

_banks = {}


def dev(x):
    return torch.from_numpy(np.ascontiguousarray(x)).to(DEV)


def window_bank(c, dtype):
    from speech_decoding_amd import WindowBank
    bank = WindowBank(c["F"], c["T"], dtype=DT[dtype], device=DEV)
    got = [bank.add_track(dev(t), s) for t, s in zip(c["tracks"], c["local"])]
    assert [len(r) for r in got] == [len(s) for s in c["local"]] and got[0].start == 0 and got[-1].stop == len(bank) == c["M"]
    return bank


def banks(shape, dtype, exact=True):
    """(case, window bank, the same candidates materialised into a SpeechBank), built once and shared (never written to)."""
    from speech_decoding_amd import SpeechBank
    key = (shape, dtype, exact)
    if key not in _banks:
        c = W.case(shape, exact)
        _banks[key] = (c, window_bank(c, dtype), SpeechBank.from_tensor(dev(W.windows_of(c["table"], c["starts"], c["T"])), dtype=DT[dtype]))
    return _banks[key]


def same_bits(a, b):
    assert len(a) == len(b)
    for x, y in zip(a, b):
        assert (x is None) == (y is None)
        if x is not None:
            assert x.dtype == y.dtype and x.shape == y.shape
            assert torch.equal(x.view(torch.int32) if x.dtype == torch.float32 else x, y.view(torch.int32) if y.dtype == torch.float32 else y)


def check_exact(shape, dtype, **kw):
    from speech_decoding_amd import retrieve
    c, wb, sb = banks(shape, dtype)
    Q, labels = dev(c["queries"]), dev(c["labels"])
    got = retrieve(Q, wb, k=10, labels=labels, **kw)
    same_bits(got, retrieve(Q, sb, k=10, labels=labels, **kw))
    idx, sc, ranks = W.restate(c)
    assert torch.equal(got.indices.cpu(), torch.from_numpy(idx))
    assert torch.equal(got.scores.cpu().view(torch.int32), torch.from_numpy(sc).view(torch.int32))
    assert torch.equal(got.ranks.cpu(), torch.from_numpy(ranks))
    return got


@pytest.mark.parametrize("dtype", ["bf16", "fp16"])
@pytest.mark.parametrize("shape", ["a", "b"])
def test_exact_against_the_materialised_bank(shape, dtype):
    c, wb, sb = banks(shape, dtype)
    assert wb.starts.dtype == torch.int32 and torch.equal(wb.starts.cpu(), torch.from_numpy(c["starts"].astype(np.int32)))
    assert np.array_equal(wb.starts_host, c["starts"])
    Cp = W.pad64(c["F"])
    assert wb.table.shape == (c["table"].shape[0], Cp) and wb.table.dtype == DT[dtype]
    assert torch.equal(wb.table[:, : c["F"]].double().cpu(), torch.from_numpy(c["table"]))
    assert not bool(wb.table[:, c["F"]:].any())                     # channel padding zero
    assert wb.nbytes == c["table"].shape[0] * Cp * 2 + 8 * c["M"] + 4 * c["table"].shape[0]
    assert wb.nbytes < sb.rows.numel() * 2
    want = torch.from_numpy(W.restate(c).csq.astype(np.float32))
    assert torch.equal(wb.norms_sq.cpu(), want) and torch.equal(sb.norms_sq.cpu(), want)       # the integer sums
    check_exact(shape, dtype)


@pytest.mark.parametrize("dtype", ["bf16", "fp16"])
@pytest.mark.parametrize("shape", ["a", "b"])
def test_exact_across_scratch_sizes(shape, dtype):
    from speech_decoding_amd import lib as L
    from speech_decoding_amd.retrieval import plan_blocks
    c = W.case(shape)
    nb, mc, tiles256, _ = plan_blocks(c["N"], c["M"], c["T"] * L.pad_channels(c["F"]), DT[dtype], SMALL_SCRATCH)
    assert tiles256 and (mc == 256 < c["M"] if shape == "a" else nb < c["N"])   # a: three chunks of 256 candidates; b: several query blocks
    same_bits(check_exact(shape, dtype, scratch_bytes=SMALL_SCRATCH), check_exact(shape, dtype))


def check_against_fp64(res, ref, labels, k, what):
    """tests/test_retrieval_gpu.py's checks: the r-th largest score, the score of the returned index, order and tie rule, rank
    bounds #{j : s_j > s_l + 2 TOL} <= rank <= #{j != l : s_j >= s_l - 2 TOL}.  Returns the largest score error."""
    N, M = ref.shape
    idx, sc = res.indices.cpu(), res.scores.cpu().double()
    assert idx.shape == (N, k) and idx.dtype == torch.int64 and res.scores.dtype == torch.float32
    top = torch.sort(ref, dim=1, descending=True).values[:, :k]
    err1 = float((sc - top).abs().max())
    assert idx.min() >= 0 and idx.max() < M
    assert all(len(set(row.tolist())) == k for row in idx), "indices repeat within a row"
    err2 = float((torch.gather(ref, 1, idx) - sc).abs().max())
    print(f"{what}: max |score - r-th largest fp64| {err1:.3e}, max |score - fp64 score of its index| {err2:.3e}")
    assert err1 <= TOL and err2 <= TOL
    s32 = res.scores.cpu()
    assert bool((s32[:, 1:] <= s32[:, :-1]).all()), "scores are not non-increasing"
    tied = s32[:, 1:] == s32[:, :-1]
    assert bool((idx[:, 1:] > idx[:, :-1])[tied].all()), "equal scores not in ascending index order"
    r = res.ranks.cpu()
    assert r.dtype == torch.int32 and r.shape == (N,)
    sl = ref[torch.arange(N), labels][:, None]
    lo = (ref > sl + 2 * TOL).sum(dim=1)
    other = torch.arange(M)[None, :] != labels[:, None]
    hi = ((ref >= sl - 2 * TOL) & other).sum(dim=1)
    assert bool((lo <= r).all()) and bool((r <= hi).all()), (lo.tolist(), r.tolist(), hi.tolist())
    return max(err1, err2)


@pytest.mark.parametrize("dtype", ["bf16", "fp16"])
@pytest.mark.parametrize("shape", ["a", "b"])
def test_real_operands_against_float64(shape, dtype):
    """Seeded normal tracks against the float64 cosine of the same rounded operands, whole and in small blocks.
    Measured on the MI355X, max |score - fp64 score|: see the module docstring."""
    from speech_decoding_amd import retrieve
    c, wb, _ = banks(shape, dtype, exact=False)
    cos, csq, _ = W.cosine64(c, dtype)
    ref, labels = torch.from_numpy(cos), torch.from_numpy(c["labels"])
    Q = dev(c["queries"])
    for scratch in (1 << 30, SMALL_SCRATCH):
        res = retrieve(Q, wb, k=10, labels=dev(c["labels"]), scratch_bytes=scratch)
        err = check_against_fp64(res, ref, labels, 10, f"real {shape} {dtype} scratch {scratch}")
        print(f"MEASURED {shape} {dtype}: {err:.3e}")
    rel = np.abs(wb.norms_sq.cpu().double().numpy() - csq) / csq
    print(f"norms_sq {shape} {dtype}: max relative error {rel.max():.3e}")
    assert rel.max() <= (c["T"] * c["F"] + 2) * 2.0 ** -24          # fp32 summation of T * F exact products in any order


@pytest.mark.parametrize("reduce", ["sum", "max"])
@pytest.mark.parametrize("shape", ["a", "b"])
def test_classes_equal_the_materialised_bank(shape, reduce):
    from speech_decoding_amd import retrieve_classes
    c, wb, sb = banks(shape, "bf16")
    ids = W.class_ids(c["M"])
    assert np.bincount(ids)[:4].min() > 4 and (np.bincount(ids)[4:] == 1).all()
    Q, labels = dev(c["queries"]), dev(ids[c["labels"]])
    kw = dict(k=5, scale=float(np.exp(5.1)), reduce=reduce, labels=labels, return_matrix=True)
    a, b = retrieve_classes(Q, wb, ids, **kw), retrieve_classes(Q, sb, ids, **kw)
    same_bits(a, b)
    same_bits(retrieve_classes(Q, wb, ids, scratch_bytes=SMALL_SCRATCH, **kw), b)
    assert bool((a.ranks.cpu() >= 0).all())


@pytest.mark.parametrize("dtype", ["bf16", "fp16"])
def test_growth_in_three_calls_equals_one_sitting(dtype):
    """Three tracks added one by one to a bank that grows from nothing hold the bytes, starts and norms of the same rows added
    as ONE track in one call; the same retrieve call twice gives the same bits."""
    from speech_decoding_amd import WindowBank, retrieve
    F, T = 40, 24
    rng = np.random.RandomState(3)
    tracks = [rng.randn(F, Lt).astype(np.float32) for Lt in (100, 333, 64)]
    local = [rng.randint(0, t.shape[1] - T + 1, size=m) for t, m in zip(tracks, (7, 300, 41))]
    grown = WindowBank(F, T, dtype=DT[dtype], device=DEV)
    got = [grown.add_track(dev(t), s) for t, s in zip(tracks, local)]
    assert got == [range(0, 7), range(7, 307), range(307, 348)]
    assert grown.add_track(dev(tracks[0]), []) == range(348, 348) and len(grown) == 348       # no window: nothing is added
    first = np.cumsum([0] + [t.shape[1] for t in tracks])
    whole = WindowBank(F, T, dtype=DT[dtype], device=DEV)
    whole.add_track(dev(np.concatenate(tracks, axis=1)), np.concatenate([s + r0 for s, r0 in zip(local, first)]))
    assert len(whole) == len(grown) and whole.nbytes == grown.nbytes
    assert torch.equal(grown.table.view(torch.int16), whole.table.view(torch.int16))
    assert torch.equal(grown.starts, whole.starts) and np.array_equal(grown.starts_host, whole.starts_host)
    assert torch.equal(grown.norms_sq.view(torch.int32), whole.norms_sq.view(torch.int32))
    assert torch.equal(grown.row_norms_sq.view(torch.int32), whole.row_norms_sq.view(torch.int32))
    # a strided, differently typed source packs to the same bytes
    other = WindowBank(F, T, dtype=DT[dtype], device=DEV)
    for t, s in zip(tracks, local):
        src = dev(t).to(DT[dtype]).t().contiguous().t()             # (F, L) with strides (1, F)
        assert not src.is_contiguous()
        other.add_track(src, s)
    assert torch.equal(other.table.view(torch.int16), grown.table.view(torch.int16))
    Q = dev(rng.randn(9, F, T).astype(np.float32))
    labels = np.arange(9) * 31
    a, b, c = retrieve(Q, grown, labels=labels), retrieve(Q, grown, labels=labels), retrieve(Q, whole, labels=labels)
    same_bits(a, b)
    same_bits(a, c)


def test_edges_one_candidate_one_query_and_all_the_same_window():
    from speech_decoding_amd import SpeechBank, WindowBank, retrieve
    c = W.case("a")
    track, T = c["tracks"][1], c["T"]                               # 333 rows
    Q = dev(c["queries"])
    one = WindowBank(c["F"], T, device=DEV)
    one.add_track(dev(track), [333 - T])                            # the last window of the table
    win = dev(track[:, 333 - T:][None])
    res = retrieve(Q, one, k=1, labels=np.zeros(c["N"], dtype=np.int64))
    same_bits(res, retrieve(Q, SpeechBank.from_tensor(win), k=1, labels=np.zeros(c["N"], dtype=np.int64)))
    assert res.indices.cpu().tolist() == [[0]] * c["N"] and res.ranks.cpu().tolist() == [0] * c["N"]
    _, wb, sb = banks("a", "bf16")
    same_bits(retrieve(Q[3:4], wb, k=10, labels=c["labels"][3:4]), retrieve(Q[3:4], sb, k=10, labels=c["labels"][3:4]))       # N = 1
    same = WindowBank(c["F"], T, device=DEV)
    same.add_track(dev(track), [57] * 300)                          # every candidate the same window: the scores tie
    res = retrieve(Q, same, k=10, labels=np.full(c["N"], 299))
    assert res.indices.cpu().tolist() == [list(range(10))] * c["N"]
    assert bool((res.scores == res.scores[:, :1]).all()) and res.ranks.cpu().tolist() == [299] * c["N"]
    assert torch.equal(same.norms_sq, same.norms_sq[:1].expand(300))
