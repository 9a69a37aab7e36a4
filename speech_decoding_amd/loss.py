"""MI355X-native `CLIPLoss` with the reference's signature (speech_decoding/utils/loss.py:28-84).

forward(x, y, fast=True, return_logits=False): x = speech embeddings Y (B, F, T), y = brain embeddings
Z (B, F, T); loss = (CE(logits) + CE(logitsᵀ)) / 2 with logits = x̂ ŷᵀ · exp(temp).  The norms, the
similarity GEMM, the softmax statistics, the gradient coefficient matrix and the embedding gradient
all run in libsdamd.so.  Under torch.distributed (one process per GPU) the speech rows are all-gathered
so the negatives span the GLOBAL batch; each rank owns the columns of its local brain embeddings.  Gradients reach x, y and
temp, as in the reference; x's is computed only when x requires one.

`SigmoidLoss` is the pairwise sigmoid contrastive loss on the same operands, buffers and gradient kernels (sda_sigmoid_*): every
(speech, brain) pair is its own binary decision, with a learned temperature and bias; nothing in the reference corresponds to it.

Also `MSELoss` (loss.py:15-25), the reference's regression objective, on the sda_mse_* kernels, and its two clamped helpers
`torch_exp` / `torch_log` (loss.py:8-13, plain torch).
"""
from __future__ import annotations

import weakref
from typing import NamedTuple, Optional

import numpy as np
import torch
import torch.nn as nn

from . import clip
from . import lib as L
from . import ops

_rank_cache = []          # [(weakref(Y), weakref(Z), Y._version, Z._version, ranks, labels key)] from the last CLIPLoss forward


class RingSlot:
    """A ring buffer handed out at generation `gen`; valid() is False once the slot has been handed out again."""
    __slots__ = ("ring", "idx", "gen", "buf")

    def __init__(self, ring, idx, gen, buf):
        self.ring, self.idx, self.gen, self.buf = ring, idx, gen, buf

    def valid(self) -> bool:
        return self.ring.gens[self.idx] == self.gen


class Ring:
    """Persistent RL buffers of one shape for packed inputs (no per-call 200 MB allocation + memset), in rotation so that the
    buffer a pending backward still needs survives one further forward (e.g. an eval pass between forward and backward).
    gens[i] counts the hand-outs of bufs[i]: a backward that comes later than that finds its slot's generation changed."""
    __slots__ = ("bufs", "gens", "next")

    def __init__(self, bufs):
        self.bufs, self.gens, self.next = bufs, [0] * len(bufs), 0

    def take(self) -> RingSlot:
        idx = self.next % len(self.bufs)
        self.next += 1
        self.gens[idx] += 1
        return RingSlot(self, idx, self.gens[idx], self.bufs[idx])


class GatheredRows:
    """The rows one side of the loss reads, and what must be waited for before reading them: `rows` holds `n` samples (the
    global batch) with squared norms `sq`, this rank's own from sample `col0` on; `slot` is the ring slot that owns the rows
    a backward will read; `works` are the collectives still filling them, `done` the event of a side stream that issued them."""
    __slots__ = ("rows", "sq", "n", "col0", "slot", "works", "done")

    def __init__(self, rows, sq, n, col0=0, slot=None, works=(), done=None):
        self.rows, self.sq, self.n, self.col0, self.slot, self.works, self.done = rows, sq, n, col0, slot, works, done

    def wait(self):
        """The current stream waits for the side stream and for RCCL's; the host does not block."""
        if self.done is not None:
            torch.cuda.current_stream(self.rows.device).wait_event(self.done)
        for work in self.works:
            work.wait()


class Pending(NamedTuple):
    """A speech-side prefetch no forward has consumed yet: for which tensor object and compute dtype, and its rows."""
    y_ref: weakref.ref
    dtype: torch.dtype
    rows: GatheredRows


class LossState:
    """Buffers that outlive one call, owned by ONE CLIPLoss instance (nothing is shared between instances by shape): the rotating
    packed-speech buffers and the pending speech-side prefetch.  A backward checks the generation of the ring slot it was given,
    so a buffer recycled by later forwards raises instead of silently feeding another batch's rows into the gradient."""

    def __init__(self):
        self.rings = {}           # (key, B, C, T, dtype, device) -> Ring
        self.pending: Optional[Pending] = None
        self.ring_depth = 2
        self.emulated = {}        # distributed.emulate_world: the resident stand-ins (rows, norms) for the other ranks' speech rows

    def drain(self):
        """Wait for a pending prefetch's collectives (the speech-row all-gather issued one batch ahead and never consumed:
        the last one of a run) and drop it.  A process group torn down while such a collective is still in flight aborts
        the process ("terminate called without an active exception": a transport thread destroyed while joinable)."""
        if self.pending is None:
            return
        rows = self.pending.rows
        if rows.done is not None:
            rows.done.synchronize()
        for work in rows.works:
            work.wait()
        if torch.cuda.is_available():
            torch.cuda.synchronize()
        self.pending = None

    def clear(self):
        self.drain()
        self.rings.clear()
        self.emulated.clear()


_DEFAULT_STATE = LossState()      # for the module-level helpers called without a CLIPLoss instance


def _cache_ranks(Y, Z, cnt, labels_key=None):
    _rank_cache.clear()
    _rank_cache.append((weakref.ref(Y), weakref.ref(Z), Y._version, Z._version, cnt, labels_key))


def _cached_ranks(Y, Z, labels_key=None):
    """Ranks of the last CLIPLoss forward — valid for the SAME two tensor objects while neither has been written in place
    since (torch's version counters, as ops.ROW_NORMS checks them): an edit of Z between loss_func(Y, Z) and
    classifier(Z, Y) sends the classifier back to computing its own ranks.  Ranks counted with speech labels serve a query
    with the same labels only, unlabelled ranks an unlabelled query only."""
    for wy, wz, vy, vz, cnt, key in _rank_cache:
        if wy() is Y and wz() is Z and Y._version == vy and Z._version == vz and _same_labels_key(key, labels_key):
            return cnt
    return None


class SpeechLabels(NamedTuple):
    """The local samples' speech ids as the kernels take them, and what identifies their values without a device read."""
    dev: torch.Tensor            # int32 [B] on the device
    host: Optional[np.ndarray]   # the same values on the host (None for a device tensor handed in as int32)
    key: object                  # bytes of the values, or ("tensor", weakref, version) of an int32 device tensor


def _same_labels_key(a, b) -> bool:
    if a is None or b is None:
        return a is None and b is None
    if isinstance(a, bytes) or isinstance(b, bytes):
        return isinstance(a, bytes) and isinstance(b, bytes) and a == b
    return a[1]() is not None and a[1]() is b[1]() and a[2] == b[2]


def speech_labels(labels, B: int, device) -> Optional[SpeechLabels]:
    """Check and upload the speech ids of the B local samples: a host sequence, a numpy array or a torch int32 / int64 tensor of
    length B whose values fit int32.  A wrong length, a non-integer dtype or a value outside int32 raises ValueError before
    anything is launched.  Host data and int64 tensors are checked on the host (an int64 device tensor costs one copy back:
    hand in int32 to avoid it); an int32 device tensor is taken as it is."""
    if labels is None:
        return None
    if isinstance(labels, SpeechLabels):
        if labels.dev.numel() != B:
            raise ValueError(f"labels: expected {B} speech ids (one per local sample), got {labels.dev.numel()}")
        return labels
    if isinstance(labels, torch.Tensor):
        if labels.dtype not in (torch.int32, torch.int64):
            raise ValueError(f"labels: expected an int32 or int64 tensor, got {labels.dtype}")
        if labels.dim() != 1 or labels.numel() != B:
            raise ValueError(f"labels: expected {B} speech ids (one per local sample), got shape {tuple(labels.shape)}")
        if labels.dtype == torch.int32 and labels.is_cuda:
            return SpeechLabels(labels.detach().contiguous(), None, ("tensor", weakref.ref(labels), labels._version))
        labels = labels.detach().cpu().numpy()
    a = np.asarray(labels)
    if a.dtype.kind not in "iu":
        raise ValueError(f"labels: expected integer speech ids, got dtype {a.dtype}")
    if a.ndim != 1 or a.size != B:
        raise ValueError(f"labels: expected {B} speech ids (one per local sample), got shape {a.shape}")
    if int(a.min()) < -2 ** 31 or int(a.max()) > 2 ** 31 - 1:
        raise ValueError("labels: speech ids must fit int32")
    a32 = np.ascontiguousarray(a.astype(np.int32))
    return SpeechLabels(ops.upload_small(a32, device), a32, a32.tobytes())


def gather_labels(lab: SpeechLabels, B: int, group) -> torch.Tensor:
    """The labels of the global batch in rank order (device int32 [B_global]): one small all-gather on the side group that
    gathers the speech rows.  In an emulated world the stand-in rows get labels that match nothing: the local ids are renumbered
    from 0 (in the order of their values) and every stand-in row gets an id of its own behind them."""
    if group is None:
        return lab.dev
    import torch.distributed as dist
    from .distributed import emulated_world, side_group
    world = dist.get_world_size(group)
    local = lab.dev
    held = emulated_world() if world == 1 and emulated_world() > 1 else world
    if held != world:
        host = lab.host if lab.host is not None else lab.dev.cpu().numpy()
        _, dense = np.unique(host, return_inverse=True)
        local = ops.upload_small(np.ascontiguousarray(dense.astype(np.int32)), lab.dev.device)
    out = torch.empty(B * held, dtype=torch.int32, device=local.device)
    dist.all_gather_into_tensor(out[: B * world], local, group=side_group("gather", group))
    if held != world:
        out[B:] = torch.arange(B, B * held, dtype=torch.int32, device=local.device)
    return out


_rows_base = ops.rows_base      # its name while it lived here: kept for code outside this tree that imported it; use ops.rows_base


def _ring_rows(state: LossState, key, B, Cc, T, dtype, device) -> RingSlot:
    """The next slot of `state`'s ring for this key and shape; a new ring gets `ring_depth` buffers."""
    k = (key, B, Cc, T, dtype, str(device))
    ring = state.rings.get(k)
    if ring is None:
        if len(state.rings) >= 8:                  # ragged last batches etc.: keep the most recent shapes only
            state.rings.pop(next(iter(state.rings)))
        ring = state.rings[k] = Ring([ops.new_rows(B, T, L.pad_channels(Cc), dtype, device) for _ in range(state.ring_depth)])
    return ring.take()


def _check_rows_arg(t: torch.Tensor, B: int, Cc: int, T: int, name: str):
    if tuple(t.shape) != (B, Cc, T):
        raise ValueError(f"{name}: expected shape {(B, Cc, T)}, got {tuple(t.shape)}")
    if not t.is_cuda:
        raise L.SdaError(f"{name} must live on the MI355X device (there is no CPU path)")


def as_rows(t: torch.Tensor, B: int, Cc: int, T: int, dtype, name: str) -> torch.Tensor:
    """Return the RL buffer behind `t` (zero copy when `t` is a rows_view made by this package), else
    pack a plain (B, C, T) tensor into a fresh RL buffer."""
    _check_rows_arg(t, B, Cc, T, name)
    return ops.rows_of(t, Cc, dtype)[0]


def _pack_ring(state: LossState, t: torch.Tensor, B: int, Cc: int, T: int, dtype, name: str, ring_key: str):
    """as_rows that packs into a rotating persistent buffer of `state`: (buffer, its RingSlot; None behind a rows_view)."""
    _check_rows_arg(t, B, Cc, T, name)
    base = ops.rows_base(t, B, Cc, T, dtype)
    if base is not None:
        return base, None
    slot = _ring_rows(state, ring_key, B, Cc, T, dtype, t.device)
    return ops.pack_rows(t.detach(), slot.buf), slot          # pack_rows rewrites every valid row


def _dist_group():
    from .distributed import active_group
    return active_group()


EMULATE_COPY_REMOTE = True      # emulated world: re-deliver the stand-in rows every step (a device copy in place of the wire)


def gather_speech_rows(Yt_local: torch.Tensor, B: int, T: int, group, async_op: bool = False,
                       state: Optional[LossState] = None, slot: Optional[RingSlot] = None, ring_key: str = "loss.Yall",
                       sq: Optional[torch.Tensor] = None) -> GatheredRows:
    """All-gather the packed speech rows of every rank (RCCL all_gather over xGMI; samples are contiguous blocks of Tp rows, so
    the gather lands directly in RL order) together with their squared norms (computed once, on the rank that owns the rows,
    unless `sq` hands them in).  The record's `slot` owns the rows the backward will read (the local pack without a group, the
    gathered buffer with one).  The same helper gathers the brain rows for the speech-side gradient (ring_key "loss.Zall").
    distributed.emulate_world(W) at world size 1: this rank is rank 0 of W.  Its own rows travel through the real all-gather
    (one rank); the (W - 1) * B rows of the other ranks are resident stand-ins, copied into the gathered buffer every step on
    the stream the gather is issued from — HBM sees the bytes a real gather would have landed (plus the copy's reads)."""
    row_elems = L.rows_tp(T) * Yt_local.shape[1]
    sq_local = sq if sq is not None else ops.rows_sumsq(Yt_local, B, row_elems, row_elems)
    if group is None:
        return GatheredRows(Yt_local, sq_local, B, 0, slot)
    import torch.distributed as dist
    from .distributed import emulated_world, side_group
    state = state or _DEFAULT_STATE
    world, rank = dist.get_world_size(group), dist.get_rank(group)
    Tp, dev = L.rows_tp(T), Yt_local.device
    held, remote = world, None                  # the buffer holds the rows of `held` ranks, the gather lands those of `world`
    if world == 1 and emulated_world() > 1:
        held = emulated_world()
        remote = _emulated_remote(state, B, held, Yt_local.shape[1], T, Yt_local.dtype, dev)
    slot = _ring_rows(state, ring_key, B * held, Yt_local.shape[1], T, Yt_local.dtype, dev)
    rows, sq_all = slot.buf, torch.empty(B * held, dtype=torch.float32, device=dev)
    bulk = side_group("gather", group)          # own communicator: must not queue in front of the BatchNorm all-reduces
    w1 = dist.all_gather_into_tensor(rows[: B * world * Tp], Yt_local[: B * Tp], group=bulk, async_op=async_op)
    w2 = dist.all_gather_into_tensor(sq_all[: B * world], sq_local, group=bulk, async_op=async_op)
    if remote is not None:
        if EMULATE_COPY_REMOTE or slot.gen == 1:
            rows[B * Tp: held * B * Tp].copy_(remote[0])
        sq_all[B:].copy_(remote[1])
    return GatheredRows(rows, sq_all, B * held, rank * B, slot, [w1, w2] if async_op else [])


def _emulated_remote(state: LossState, B, W, Cp, T, dt, dev):
    """The resident (rows, norms) that stand in for the W - 1 other ranks of an emulated world: seeded N(0, 1) rows packed by
    sda_pack_rows, norms by sda_rows_sumsq, made once per shape."""
    Tp = L.rows_tp(T)
    key = ("remote", B, W, Cp, T, dt, str(dev))
    rem = state.emulated.get(key)
    if rem is None:
        rows = torch.zeros(((W - 1) * B * Tp, Cp), dtype=dt, device=dev)
        nsq = torch.empty((W - 1) * B, dtype=torch.float32, device=dev)
        g = torch.Generator(device=dev).manual_seed(4242)
        tmp = ops.new_rows(B, T, Cp, dt, dev)
        for k in range(W - 1):
            ops.pack_rows(torch.randn((B, Cp, T), generator=g, device=dev), tmp)
            rows[k * B * Tp: (k + 1) * B * Tp].copy_(tmp[: B * Tp])
            nsq[k * B: (k + 1) * B] = ops.rows_sumsq(tmp, B, Tp * Cp, Tp * Cp)
        rem = state.emulated[key] = (rows, nsq)
    return rem


_prefetch_streams = {}    # device -> side stream the speech-side work runs on
PREFETCH_ON_SIDE_STREAM = True


def prefetch_speech(Y: torch.Tensor, dtype=None, global_negatives: bool = True, state: Optional[LossState] = None):
    """Start the speech-side work of the loss EARLY: pack Y into row layout, take its row norms and, under data
    parallelism, launch the all-gather of the packed rows asynchronously on RCCL's stream.  Y does not depend on
    the encoder, so calling this before `brain_encoder(X, ...)` hides the 1.4 GB (8 GPUs, config 3) gather behind
    the forward.  The pack + norms (HBM-bound, ~0.2 ms at config 2) run on a side stream of their own, beside the
    encoder's first layers instead of in front of them."""
    B, F, T = Y.shape
    dtype = dtype or torch.float32
    state = state or _DEFAULT_STATE
    group = _dist_group() if global_negatives else None

    def pack_and_gather() -> GatheredRows:
        Yt_local, slot = _pack_ring(state, Y, B, F, T, dtype, "x (speech embeddings)", "loss.Y")
        return gather_speech_rows(Yt_local, B, T, group, async_op=True, state=state, slot=slot)
    if PREFETCH_ON_SIDE_STREAM and Y.is_cuda:
        main = torch.cuda.current_stream(Y.device)
        side = _prefetch_streams.get(str(Y.device))
        if side is None:
            side = _prefetch_streams[str(Y.device)] = torch.cuda.Stream(device=Y.device)
        ev = torch.cuda.Event()
        ev.record(main)
        side.wait_event(ev)                       # Y itself, and the previous user of the ring buffer, are on `main`
        with torch.cuda.stream(side):
            g = pack_and_gather()
            g.done = torch.cuda.Event()
            g.done.record(side)
        g.sq.record_stream(main)
    else:
        g = pack_and_gather()
    state.pending = Pending(weakref.ref(Y), dtype, g)


def _take_prefetched(state: LossState, Y, dtype) -> Optional[GatheredRows]:
    p = state.pending
    if p is None or p.y_ref() is not Y or p.dtype != dtype:
        return None
    state.pending = None
    p.rows.wait()
    return p.rows


_RECYCLED = ("CLIPLoss.backward: the packed {what} rows of this forward were recycled by later forwards of the same CLIPLoss "
             "(more than `ring_depth` forwards before this backward); raise loss_func._state.ring_depth or call backward earlier")


def speech_negatives(negatives, F: int, T: int, dtype, device) -> Optional[clip.ClipNegatives]:
    """Check the extra speech negatives of one forward — a retrieval.WindowBank, every candidate of which is a negative — against
    the brain rows' shape, compute dtype and device, and name them for the kernels.  Everything is refused here, before the
    first launch.  None passes."""
    if negatives is None or isinstance(negatives, clip.ClipNegatives):
        return negatives
    from .retrieval import WindowBank
    if not isinstance(negatives, WindowBank):
        raise L.SdaError(f"CLIPLoss: negatives must be a WindowBank (windows of resident speech tracks, e.g. feed.speech_bank(idx)), "
                         f"got {type(negatives).__name__}; a tensor of materialised segments is not taken: load each as a track")
    if dtype == torch.float32:
        raise L.SdaError("CLIPLoss: negatives with float32 compute; the windowed similarity GEMM serves 16-bit storage only (bfloat16 "
                         "or float16) and nothing materialises the windows instead: run the loss on bfloat16 or float16 embeddings")
    if (negatives.F, negatives.T) != (F, T) or negatives.dtype != dtype:
        raise L.SdaError(f"CLIPLoss: negatives of F={negatives.F}, T={negatives.T}, {negatives.dtype} against brain embeddings of "
                         f"F={F}, T={T}, {dtype} (the compute dtype)")
    if len(negatives) == 0:
        raise L.SdaError("CLIPLoss: an empty bank of negatives (pass negatives=None for none)")
    ng = clip.ClipNegatives.of(negatives)
    if ng.table.device != torch.device(device):
        raise L.SdaError(f"CLIPLoss: the negatives' table is on {ng.table.device}, the brain embeddings on {device}")
    span = min(ops.sim_gemm_windows_span(negatives.row_elems), ops.clip_dz_windows_span(negatives.row_elems))
    if ng.hi - ng.lo > span:
        raise L.SdaError(f"CLIPLoss: the negatives' windows span table rows {ng.lo} ... {ng.hi}, more than the {span} rows (4 GB) one "
                         "launch addresses; draw them from neighbouring tracks (nothing is chunked)")
    return ng


class _ClipFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, module: "CLIPLoss", Y, Z, temp, labels=None, negatives=None):
        import torch.distributed as dist
        B, F, T = Z.shape
        lab = speech_labels(labels, B, Z.device)    # refused here, before the first launch, when they are malformed
        dtype = Z.dtype if Z.dtype in ops.COMPUTE_DTYPES else torch.float32
        neg = speech_negatives(negatives, F, T, dtype, Z.device)
        Zt = as_rows(Z, B, F, T, dtype, "y (brain embeddings)")
        group = _dist_group() if module.global_negatives else None
        state = module._state
        want_y = ctx.needs_input_grad[1]            # (False under no_grad even for a leaf that requires a gradient)
        y_rows = False
        if want_y:
            # the gradient leaves in the argument's own form: the row-layout buffer of a rows view in the compute dtype, else a
            # (B, F, T) tensor of the argument's dtype
            y_rows = ops.rows_base(Y, B, F, T, dtype) is not None
            if not y_rows and not Y.is_cuda:
                raise L.SdaError("CLIPLoss: x (speech embeddings) must live on the MI355X device (there is no CPU path)")
            if not y_rows and Y.dtype not in ops.COMPUTE_DTYPES:
                raise L.SdaError(f"CLIPLoss: a speech embedding that requires a gradient must be fp32, bf16 or fp16, got {Y.dtype}")
            if group is not None and dist.get_world_size(group) == 1:
                from .distributed import emulated_world
                if emulated_world() > 1:
                    raise L.SdaError("CLIPLoss: the emulated world (stand-in rows for the other ranks) has no gradient for the "
                                     "speech embeddings; detach x or run real ranks")
        yg = _take_prefetched(state, Y, dtype)
        if yg is None:
            Yt_local, slot = _pack_ring(state, Y, B, F, T, dtype, "x (speech embeddings)", "loss.Y")
            yg = gather_speech_rows(Yt_local, B, T, group, state=state, slot=slot)
        lab_all = None if lab is None else gather_labels(lab, B, group)
        loss, logits, cnt, cctx = clip.clip_forward(yg.rows, Zt, temp.detach(), Bm=yg.n, Bn=B, T=T, col0=yg.col0,
                                                    reduction=module.reduction, B_global=yg.n, dist_group=group, ysq=yg.sq,
                                                    labels=lab_all, duplicates=module.duplicates, negatives=neg)
        ctx.z_gather = None
        if want_y and group is not None:
            # the speech-side gradient contracts over the brain rows of ALL ranks: gather them (and their norms) now, behind
            # the rest of the step; backward waits for it
            ctx.z_gather = gather_speech_rows(Zt, B, T, group, async_op=True, state=state, ring_key="loss.Zall", sq=cctx.zsq)
        if group is not None:
            # one collective for both: the rank counts (exact in fp32) and the loss share -> global loss for
            # reporting (backward uses the local share)
            both = torch.cat([cnt.to(torch.float32), loss.reshape(1)])
            dist.all_reduce(both, group=group)
            cnt, loss = both[:-1].round().to(torch.int32), both[-1:]
        ctx.cctx, ctx.shape, ctx.dtype, ctx.group, ctx.y_slot = cctx, (B, F, T), dtype, group, yg.slot
        ctx.set_materialize_grads(False)            # no zero-filled gradient for the (non-differentiable) logits output
        ctx.z_requires_grad = Z.requires_grad
        ctx.y_requires_grad, ctx.y_rows, ctx.y_dtype = want_y, y_rows, Y.dtype
        _cache_ranks(Y, Z, cnt[yg.col0: yg.col0 + B], None if lab is None else lab.key)
        ctx.mark_non_differentiable(logits)
        return loss.reshape(()), logits

    @staticmethod
    def backward(ctx, dloss, _dlogits):
        c = ctx.cctx
        B, F, T = ctx.shape
        dZ = dY = None
        if dloss is None:                           # (the loss itself took no part in what was differentiated)
            return None, None, None, None, None, None
        scale = dloss.to(torch.float32)
        if (ctx.z_requires_grad or ctx.y_requires_grad) and ctx.y_slot is not None and not ctx.y_slot.valid():
            raise L.SdaError(_RECYCLED.format(what="speech"))
        if ctx.z_requires_grad:
            # a buffer of its own per backward (two pending backwards must not share one): the GEMM rewrites every sample's
            # rows, pad rows included (exact zeros), so only the slack behind the last sample needs a fill
            dZt = ops.new_rows_uninit(B, T, c.Zt.shape[1], ctx.dtype, c.Zt.device)
            clip.clip_backward(c, dZt, scale.reshape(1).contiguous())     # dloss folded into the GEMM epilogue
            dZ = ops.rows_view(dZt, B, F, T)
        if ctx.y_requires_grad:
            dYt = _clip_dy(ctx, scale.reshape(1).contiguous())
            dY = ops.rows_view(dYt, B, F, T) if ctx.y_rows else ops.unpack_rows(dYt, B, F, T, ctx.y_dtype)
        dtemp = ops.scalar_mul(c.dtemp, scale.reshape(1))
        return None, dY, dZ, dtemp, None, None


def _clip_dy(ctx, scale: torch.Tensor) -> torch.Tensor:
    """The speech-side gradient of this rank's own rows as a fresh row-layout buffer (the buffer contract of the encoder's
    outputs: pad rows, slack and pad channels zero).  One process: clip.clip_backward_y.  Data parallelism: the coefficient
    block of every rank is all-gathered (Gy rows of the brain samples, partial row sums), and this rank contracts its own
    speech columns against the gathered brain rows — the rows one process would compute on the global batch."""
    c = ctx.cctx
    B, F, T = ctx.shape
    dYt = ops.new_rows_uninit(B, T, c.Yt.shape[1], ctx.dtype, c.Yt.device)
    if ctx.group is None:
        clip.clip_backward_y(c, dYt, scale)
        return dYt
    import torch.distributed as dist
    from .distributed import side_group
    world, rank = dist.get_world_size(ctx.group), dist.get_rank(ctx.group)
    zg = ctx.z_gather
    zg.wait()
    if not zg.slot.valid():
        raise L.SdaError(_RECYCLED.format(what="brain"))
    Bg, sp = c.Bm, L.pad_channels(B)
    Gy, part = clip.clip_grad_y_coeffs(c, zg.sq, ctx.dtype, seg=B, seg_pitch=sp, groups=world)
    Gall = torch.empty((Bg + 1, world * sp), dtype=ctx.dtype, device=Gy.device)
    ops.fill_zero_(Gall[Bg])                        # the zero row behind the contraction
    pall = torch.empty((world * part.shape[0], Bg), dtype=torch.float32, device=Gy.device)
    bulk = side_group("gather", ctx.group)
    dist.all_gather_into_tensor(Gall[:Bg], Gy[:B], group=bulk)
    dist.all_gather_into_tensor(pall, part, group=bulk)
    rscale_y, cscale_y = ops.clip_grad_y_finish(pall, c.ysq, zg.sq, c.temp, c.inv_norm, rank * B, B)
    Yown = c.Yt[rank * B * L.rows_tp(T):]           # this rank's rows of the gathered speech buffer
    ops.clip_dz(Gall[:, rank * sp:(rank + 1) * sp], zg.rows, Yown, dYt, rscale_y, cscale_y, Bm=Bg, Bn=B, row_elems=c.row_elems,
                out_scale=scale)
    return dYt


class CLIPLoss(nn.Module):
    def __init__(self, args):
        super().__init__()
        L.load()
        self.reduction = str(args.reduction)
        if self.reduction not in ("mean", "sum"):
            raise ValueError("reduction must be 'mean' or 'sum'")
        # what a repeated speech segment in a batch counts as when forward() is given labels: a further positive of its
        # partners ("positive") or no negative of them ("mask")
        get = getattr(args, "get", None)
        self.duplicates = str(get("clip_duplicates", "positive") if get else getattr(args, "clip_duplicates", "positive"))
        ops.clip_dup_code(self.duplicates)          # any other value: ValueError
        self.temp = nn.Parameter(torch.tensor([float(args.init_temperature)]))
        self.global_negatives = True
        self.last_logits: Optional[torch.Tensor] = None
        self._state = LossState()           # packed-speech ring + pending prefetch of THIS instance

    def prefetch(self, x: torch.Tensor, compute_dtype=torch.float32):
        """Optional: call with the speech embeddings BEFORE running the encoder (see prefetch_speech)."""
        prefetch_speech(x, compute_dtype, self.global_negatives, state=self._state)

    def drain(self):
        """Wait for (and drop) a prefetch that no forward will consume — call before tearing the process group down."""
        self._state.drain()

    def release_buffers(self):
        """Drop the persistent packed-speech buffers (e.g. between a training and an evaluation phase)."""
        self._state.clear()

    def forward(self, x, y, fast=True, return_logits=False, labels=None, negatives=None):
        """`labels`: the speech id of each local sample (a host sequence, a numpy array or an int32 / int64 tensor of length B):
        samples of the global batch with one id carry the same speech segment and are treated as `self.duplicates` says.
        None: every sample is its own class — the reference's loss.
        `negatives`: a retrieval.WindowBank (typically feed.speech_bank(feed.draw_negatives(...)), which shares the resident
        table) every candidate of which is a further speech negative: it has no brain partner, so it joins the brain -> speech
        soft-max only — B_g + N candidates per brain segment, the direction `retrieve` scores — and the loss stays normalised by
        the global batch.  The windows are read in place (16-bit compute only); they get no gradient.  The caller guarantees
        that none carries the speech id of a sample of the global batch and that every rank is handed the same ones.  The
        returned logits stay the paired block.  None: today's launches."""
        batch_size = x.size(0)
        assert batch_size > 1, "Batch size must be greater than 1."               # loss.py:40
        if negatives is not None:                   # refused before the labels' upload, the first launch of a labelled forward
            negatives = speech_negatives(negatives, y.size(1), y.size(2), y.dtype if y.dtype in ops.COMPUTE_DTYPES else torch.float32,
                                         y.device)
        if labels is not None:
            labels = speech_labels(labels, batch_size, y.device)
        if not fast:
            # loss.py:46-50: logits[i][j] = cos(y_i, x_j) — the fast way's matrix TRANSPOSED and without the learned
            # temperature (which then receives no gradient).  The symmetric loss is the same function of it, so the same
            # kernels run with a zero log-temperature; only the returned logits are turned.
            zero = torch.zeros(1, dtype=torch.float32, device=self.temp.device)
            loss, logits = _ClipFn.apply(self, x, y, zero, labels, negatives)
            self.last_logits = logits
            return (logits.t(), loss) if return_logits else loss
        loss, logits = _ClipFn.apply(self, x, y, self.temp, labels, negatives)
        self.last_logits = logits
        if return_logits:
            return logits, loss
        return loss


class _SigmoidFn(torch.autograd.Function):
    """SigmoidLoss's node: _ClipFn's operands, buffers and gradient forms around clip.sigmoid_forward.  A rank's block of pairs is
    complete on its own, so under data parallelism the forward runs the speech all-gather and the one all-reduce of the loss
    share — no merge of row statistics."""

    @staticmethod
    def forward(ctx, module: "SigmoidLoss", Y, Z, temp, bias, labels=None):
        import torch.distributed as dist
        B, F, T = Z.shape
        lab = speech_labels(labels, B, Z.device)    # refused here, before the first launch, when they are malformed
        dtype = Z.dtype if Z.dtype in ops.COMPUTE_DTYPES else torch.float32
        Zt = as_rows(Z, B, F, T, dtype, "y (brain embeddings)")
        group = _dist_group() if module.global_negatives else None
        state = module._state
        want_y = ctx.needs_input_grad[1]
        y_rows = False
        if want_y:
            y_rows = ops.rows_base(Y, B, F, T, dtype) is not None
            if not y_rows and not Y.is_cuda:
                raise L.SdaError("SigmoidLoss: x (speech embeddings) must live on the MI355X device (there is no CPU path)")
            if not y_rows and Y.dtype not in ops.COMPUTE_DTYPES:
                raise L.SdaError(f"SigmoidLoss: a speech embedding that requires a gradient must be fp32, bf16 or fp16, got {Y.dtype}")
            if group is not None and dist.get_world_size(group) == 1:
                from .distributed import emulated_world
                if emulated_world() > 1:
                    raise L.SdaError("SigmoidLoss: the emulated world (stand-in rows for the other ranks) has no gradient for the "
                                     "speech embeddings; detach x or run real ranks")
        yg = _take_prefetched(state, Y, dtype)
        if yg is None:
            Yt_local, slot = _pack_ring(state, Y, B, F, T, dtype, "x (speech embeddings)", "loss.Y")
            yg = gather_speech_rows(Yt_local, B, T, group, state=state, slot=slot)
        lab_all = None if lab is None else gather_labels(lab, B, group)
        loss, a, cnt, cctx = clip.sigmoid_forward(yg.rows, Zt, temp.detach(), bias.detach(), Bm=yg.n, Bn=B, T=T, col0=yg.col0,
                                                  reduction=module.reduction, B_global=yg.n, ysq=yg.sq, labels=lab_all,
                                                  duplicates=module.duplicates)
        ctx.z_gather = None
        if want_y and group is not None:            # the brain rows of all ranks, for the speech-side gradient (as in _ClipFn)
            ctx.z_gather = gather_speech_rows(Zt, B, T, group, async_op=True, state=state, ring_key="loss.Zall", sq=cctx.zsq)
        ranks_known = True
        if group is not None:
            # the loss share -> global loss for reporting (backward uses the local share).  The rank counts of a row need its
            # positive's logit, which lives on one rank: with more than one real rank they are left to the Classifier's own pass
            # instead of a second collective here
            ranks_known = dist.get_world_size(group) == 1
            loss = loss.clone()
            dist.all_reduce(loss, group=group)
        ctx.cctx, ctx.shape, ctx.dtype, ctx.group, ctx.y_slot = cctx, (B, F, T), dtype, group, yg.slot
        ctx.set_materialize_grads(False)
        ctx.z_requires_grad = Z.requires_grad
        ctx.y_requires_grad, ctx.y_rows, ctx.y_dtype = want_y, y_rows, Y.dtype
        if ranks_known:
            _cache_ranks(Y, Z, cnt[yg.col0: yg.col0 + B], None if lab is None else lab.key)
        ctx.mark_non_differentiable(a)
        return loss.reshape(()), a

    @staticmethod
    def backward(ctx, dloss, _da):
        c = ctx.cctx
        B, F, T = ctx.shape
        dZ = dY = None
        if dloss is None:
            return None, None, None, None, None, None
        scale = dloss.to(torch.float32)
        if (ctx.z_requires_grad or ctx.y_requires_grad) and ctx.y_slot is not None and not ctx.y_slot.valid():
            raise L.SdaError(_RECYCLED.format(what="speech").replace("CLIPLoss", "SigmoidLoss"))
        if ctx.z_requires_grad:
            dZt = ops.new_rows_uninit(B, T, c.Zt.shape[1], ctx.dtype, c.Zt.device)
            clip.clip_backward(c, dZt, scale.reshape(1).contiguous())     # dloss folded into the GEMM epilogue
            dZ = ops.rows_view(dZt, B, F, T)
        if ctx.y_requires_grad:
            dYt = _clip_dy(ctx, scale.reshape(1).contiguous())
            dY = ops.rows_view(dYt, B, F, T) if ctx.y_rows else ops.unpack_rows(dYt, B, F, T, ctx.y_dtype)
        dtemp = ops.scalar_mul(c.dtemp, scale.reshape(1))
        dbias = ops.scalar_mul(c.dbias, scale.reshape(1))
        return None, dY, dZ, dtemp, dbias, None


class SigmoidLoss(nn.Module):
    """The pairwise sigmoid contrastive loss (SigLIP): every (speech i, brain j) pair of the global batch is its own binary
    decision on l_ij = cos(x_i, y_j) exp(temp) + bias — the positive pairs towards +, all others towards - :
        loss = (1 / B, or 1 for reduction="sum") * sum_ij softplus(-z_ij l_ij),   z_ij = +1 for a positive pair, else -1.
    forward(x, y, return_logits=False, labels=None): x = speech, y = brain embeddings (B, F, T), as CLIPLoss takes them (rows
    views of encoder outputs or plain tensors; fp32 / bf16 / fp16); gradients reach y, x (when it requires one), temp and bias.
    `labels`: the speech id of each local sample; two samples with one id are a further positive pair
    (clip_duplicates="positive") or a pair that is left out ("mask").  No row or column couples its entries: under data
    parallelism a rank's block of pairs is complete on its own and the loss is the sum of the blocks."""

    def __init__(self, args):
        super().__init__()
        L.load()
        self.reduction = str(args.reduction)
        if self.reduction not in ("mean", "sum"):
            raise ValueError("reduction must be 'mean' or 'sum'")
        get = getattr(args, "get", None) or (lambda k, d: getattr(args, k, d))
        self.duplicates = str(get("clip_duplicates", "positive"))
        ops.clip_dup_code(self.duplicates)          # any other value: ValueError
        self.temp = nn.Parameter(torch.tensor([float(get("sigmoid_init_temperature", np.log(10.0)))]))
        self.bias = nn.Parameter(torch.tensor([float(get("sigmoid_init_bias", -10.0))]))
        self.global_negatives = True
        self.last_logits: Optional[torch.Tensor] = None      # the scaled cosines a of the last forward (the logits less the bias)
        self._state = LossState()           # packed-speech ring + pending prefetch of THIS instance

    def prefetch(self, x: torch.Tensor, compute_dtype=torch.float32):
        """Optional: call with the speech embeddings BEFORE running the encoder (see prefetch_speech)."""
        prefetch_speech(x, compute_dtype, self.global_negatives, state=self._state)

    def drain(self):
        """Wait for (and drop) a prefetch that no forward will consume — call before tearing the process group down."""
        self._state.drain()

    def release_buffers(self):
        """Drop the persistent packed-speech buffers (e.g. between a training and an evaluation phase)."""
        self._state.clear()

    def forward(self, x, y, return_logits=False, labels=None):
        batch_size = x.size(0)
        if labels is not None:
            labels = speech_labels(labels, batch_size, y.device)
        loss, a = _SigmoidFn.apply(self, x, y, self.temp, self.bias, labels)
        self.last_logits = a
        if return_logits:                           # made on request only: the hot path stores a alone
            return a + self.bias.detach(), loss
        return loss


@torch.no_grad()
def retrieval_ranks(Y: torch.Tensor, Z: torch.Tensor, global_candidates: bool = True, labels=None) -> torch.Tensor:
    """Rank of each speech row's own brain column (0 = top-1).  Reuses the ranks computed by the last
    CLIPLoss forward on the same tensors; otherwise runs the similarity GEMM + rank kernel.  With `labels` (the local samples'
    speech ids, as CLIPLoss.forward takes them) a column that carries the row's own speech never counts against it."""
    B, F, T = Z.shape
    lab = speech_labels(labels, B, Z.device)
    hit = _cached_ranks(Y, Z, None if lab is None else lab.key)
    if hit is not None:
        return hit
    dtype = Z.dtype if Z.dtype in ops.COMPUTE_DTYPES else torch.float32
    Zt = as_rows(Z, B, F, T, dtype, "Z")
    Yt = as_rows(Y, B, F, T, dtype, "Y")
    temp = torch.zeros(1, dtype=torch.float32, device=Zt.device)
    group = _dist_group() if global_candidates else None     # under data parallelism: the GLOBAL batch
    yg = gather_speech_rows(Yt, B, T, group)
    lab_all = None if lab is None else gather_labels(lab, B, group)
    _, _, cnt, _ = clip.clip_forward(yg.rows, Zt, temp, Bm=yg.n, Bn=B, T=T, col0=yg.col0, B_global=yg.n, dist_group=group,
                                     ysq=yg.sq, labels=lab_all)
    if group is not None:
        import torch.distributed as dist
        dist.all_reduce(cnt, group=group)
    return cnt[yg.col0: yg.col0 + B]


# ------------------------------------------------------------------------------------------------------------------------------
# MSELoss (speech_decoding/utils/loss.py:15-25) and the reference's two clamped helpers (loss.py:8-13)
# ------------------------------------------------------------------------------------------------------------------------------
def torch_exp(x: torch.Tensor) -> torch.Tensor:
    """exp of x clamped from above at 10 (no overflow for large logits).  Plain torch, off the hot path."""
    return torch.clamp(x, max=10.0).exp()


def torch_log(x: torch.Tensor) -> torch.Tensor:
    """log of x clamped from below at 1e-10 (finite at 0).  Plain torch, off the hot path."""
    return torch.clamp(x, min=1e-10).log()


def _mse_operand(t: torch.Tensor, B: int, F: int, T: int, name: str):
    """(operand, is_rows): the row-layout buffer behind a rows_view (zero copy), else the plain tensor made contiguous."""
    if t.dtype in ops.COMPUTE_DTYPES:
        base = ops.rows_base(t, B, F, T, t.dtype)
        if base is not None:
            return base, True
    if not t.is_cuda:
        raise L.SdaError(f"MSELoss: {name} must live on the MI355X device (there is no CPU path)")
    ops.dt_code(t.dtype)                      # fp32 / bf16 / fp16 only
    return t.detach().contiguous(), False


class _MseFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, module: "MSELoss", Y, Z):
        if Y.dim() != 3 or tuple(Y.shape) != tuple(Z.shape):
            raise ValueError(f"MSELoss: Y and Z must both be (B, F, T) of one shape, got {tuple(Y.shape)} and {tuple(Z.shape)}")
        B, F, T = Z.shape
        Zo, z_rows = _mse_operand(Z, B, F, T, "Z (brain embeddings)")
        Yo, y_rows = _mse_operand(Y, B, F, T, "Y (speech embeddings)")
        if Yo.device != Zo.device:
            raise L.SdaError(f"MSELoss: Y is on {Yo.device}, Z on {Zo.device}")
        group = _dist_group() if module.global_batch else None
        B_global = B
        if group is not None:
            import torch.distributed as dist
            B_global = B * dist.get_world_size(group)
        # the local share sum_local / B_global: summed over ranks it is the global mean, and its gradient summed over ranks
        # is the single-process gradient on the global batch
        loss = ops.mse_forward(Zo, Yo, B, F, T, B_global)
        if group is not None:
            dist.all_reduce(loss.reshape(1), group=group)
        ctx.set_materialize_grads(False)
        ctx.operands = (Zo, z_rows, Yo, y_rows)
        ctx.dims = (B, F, T, B_global)
        return loss

    @staticmethod
    def backward(ctx, dloss):
        want_y, want_z = ctx.needs_input_grad[1], ctx.needs_input_grad[2]
        if dloss is None or not (want_y or want_z):
            return None, None, None
        Zo, z_rows, Yo, y_rows = ctx.operands
        B, F, T, B_global = ctx.dims

        def new_grad(src, rows):
            # a buffer of its own per backward; the kernel writes every valid row, pad channels included
            return ops.new_rows_uninit(B, T, src.shape[1], src.dtype, src.device) if rows else torch.empty_like(src)

        dZ = new_grad(Zo, z_rows) if want_z else None
        dY = new_grad(Yo, y_rows) if want_y else None
        ops.mse_backward(Zo, Yo, B, F, T, B_global, dloss.detach().to(torch.float32).reshape(1).contiguous(), dZ, dY)
        if dZ is not None and z_rows:
            dZ = ops.rows_view(dZ, B, F, T)
        if dY is not None and y_rows:
            dY = ops.rows_view(dY, B, F, T)
        return None, dY, dZ


class MSELoss(nn.Module):
    """forward(Y, Z) = ((Y - Z) ** 2).sum(dim=(1, 2)).mean(): summed over features and time, averaged over the batch, as a
    0-dim fp32 tensor.  Y (speech) and Z (brain) may each be an encoder output in row layout or a plain (B, F, T) tensor of
    fp32 / bf16 / fp16; both get gradients when they require them.  Under torch.distributed with `global_batch` (the default)
    the mean is over the GLOBAL batch: the forward returns it (one all-reduce), the backward gives this rank's share, so the
    summed gradients are those of one process on the whole batch.  Shapes must match exactly (no broadcasting)."""

    def __init__(self):
        super().__init__()
        L.load()
        self.global_batch = True

    def forward(self, Y, Z):
        return _MseFn.apply(self, Y, Z)
