"""Host-side orchestration of the HIP kernels for one encoder forward / backward.

Mirrors the data flow of the reference's `BrainEncoder.forward` (models.py:191-196) and of the
backward pass autograd derives from it, but every stage is a libsdamd.so kernel launched on the
current HIP stream over channels-last "row layout" buffers that stay resident in HBM between
forward and backward.  torch supplies memory and streams only.
"""
from __future__ import annotations

from dataclasses import dataclass, field
from typing import Dict, List, Optional

import ast
from collections import namedtuple
import os

import numpy as np
import torch

from . import lib as L
from . import layers
from . import ops
from .clip import ClipBlockStats, ClipCtx, clip_backward, clip_backward_y, clip_block_finish, clip_block_stats, clip_forward  # noqa: F401


@dataclass
class EncoderDims:
    C: int
    S: int
    D1: int
    D2: int
    F: int
    K: int

    @property
    def Cp(self): return L.pad_channels(self.C)
    @property
    def D1p(self): return L.pad_channels(self.D1)
    @property
    def D2p(self): return L.pad_channels(self.D2)
    @property
    def F1(self): return 2 * self.D2
    @property
    def F1p(self): return L.pad_channels(2 * self.D2)
    @property
    def Fp(self): return L.pad_channels(self.F)


@dataclass
class EncoderCtx:
    """Everything the backward needs; buffers are owned by the engine's workspace."""
    B: int
    T: int
    gen: int
    training: bool
    bufs: Dict[str, torch.Tensor] = field(default_factory=dict)
    packed: Dict[str, torch.Tensor] = field(default_factory=dict)
    bn: Dict[str, tuple] = field(default_factory=dict)
    mask: Optional[torch.Tensor] = None
    widx: Optional[torch.Tensor] = None
    subj_perm: Optional[torch.Tensor] = None
    subj_seg: Optional[torch.Tensor] = None
    subj_slices: int = 1                                  # K-segments per subject in the per-subject weight gradient
    W_sa: Optional[torch.Tensor] = None
    packed_T: Dict[str, torch.Tensor] = field(default_factory=dict)
    packed_T_ready: Optional[torch.cuda.Event] = None     # side-stream packing of packed_T has finished
    glu_fused: bool = False                               # F.glu ran in conv2's epilogue: bufs hold the gate, not [value | gate]
    composed: Optional[tuple] = None                      # composed SubjectBlock: (Wd, T1aug, Ws) fp32 factors kept for backward
    param_grads: bool = True                              # backward computes the parameters' gradients (False: a frozen encoder)
    x_dtype: Optional[torch.dtype] = None                 # X requires a gradient: dX comes back in this dtype ...
    W_x: Optional[torch.Tensor] = None                    # ... through the matrix the forward applied to X (its own copy)


@dataclass
class _Forward:
    """What the stages of one EncoderEngine.forward call share."""
    eng: "EncoderEngine"
    P: Dict[str, torch.Tensor]
    ctx: EncoderCtx
    dev: torch.device
    main: torch.cuda.Stream
    need_grad: bool
    need_dx: bool
    eps: float
    momentum: float
    k3_flags: int
    count: float                                          # rows behind a BatchNorm statistic
    packed_ready: Optional[torch.cuda.Event] = None       # side-stream packing of ctx.packed and Xt has finished
    flip: Dict[int, int] = field(default_factory=dict)

    def rows(self, name, Cp):
        B, T = self.ctx.B, self.ctx.T
        if not self.need_grad:           # inference: two ping-pong buffers per width are enough
            name = f"pp{self.flip.setdefault(Cp, 0) % 3}"
            self.flip[Cp] += 1
        return self.eng._rows(name, B, T, Cp, self.dev, "train" if self.need_grad else "eval")


class _Backward:
    """What the stages of one EncoderEngine.backward call share: the two streams, the gradients so far and the all-reduces in
    flight, with the helpers that place work on the weight-gradient stream."""
    __slots__ = ("eng", "P", "ctx", "B", "T", "dev", "pg", "main", "side", "grads", "pending", "scratch", "overlap", "world")

    def __init__(self, eng: "EncoderEngine", P, ctx: EncoderCtx, dev, main):
        d = eng.d
        self.eng, self.P, self.ctx, self.B, self.T, self.dev, self.main = eng, P, ctx, ctx.B, ctx.T, dev, main
        self.grads: Dict[str, torch.Tensor] = {}
        self.pg = ctx.param_grads             # False: the data-gradient chain only (no weight gradient, bias sum or collective of them)
        self.scratch = ops.reduce_scratch(max(d.Fp, 2 * d.D2p, d.F1p), dev)
        self.pending = []                     # in-flight gradient all-reduces
        self.overlap = eng.group is not None and eng.overlap_grad_allreduce
        self.side = eng._side_stream(dev) if eng.wgrad_side_stream else None
        self.world = eng.world

    def flush(self, names):
        """Pack the named gradients into one flat bucket, start its SUM all-reduce asynchronously and
        re-point the gradients at views of the bucket (no copy back)."""
        if not self.overlap or not self.pg:
            return
        import torch.distributed as dist
        from .distributed import side_group
        grads, side = self.grads, self.side
        flats = [torch.view_as_real(grads[n]).reshape(-1) if grads[n].is_complex() else grads[n].reshape(-1) for n in names]

        def pack_and_reduce():
            # on the SIDE stream, where the weight gradients of this group are produced: the main stream (the
            # critical path) never waits for them; on_side() makes the side stream wait for the few gradients
            # that come from the main stream (biases, BatchNorm affine)
            b = torch.cat(flats)
            if side is not None:
                for f in flats:               # sources made on the main stream are read here, on the side stream
                    f.record_stream(side)
            self.pending.append(dist.all_reduce(b, op=dist.ReduceOp.SUM, group=side_group("grads", self.eng.group), async_op=True))
            return b
        bucket = self.on_side(pack_and_reduce)
        off = 0
        for n, f in zip(names, flats):
            v = bucket[off: off + f.numel()]
            grads[n] = torch.view_as_complex(v.view(*grads[n].shape, 2)) if grads[n].is_complex() else v.view(grads[n].shape)
            off += f.numel()

    def tmp(self, name, Cp):
        return self.eng._rows("bw." + name, self.B, self.T, Cp, self.dev, "train")

    def on_side(self, fn):
        """Run `fn` (launches + allocations) on the side stream once everything queued on the main stream
        so far is done; outputs are handed back to the main stream by join_side()."""
        side, main = self.side, self.main
        if side is None:
            return fn()
        ev = torch.cuda.Event()
        ev.record(main)
        side.wait_event(ev)
        # (set_stream both ways instead of the torch.cuda.stream() context: ~40 calls per backward, and the context
        # manager costs the host 15-20 us a time; backward() is entered on `main` and nothing in `fn` leaves a third stream current)
        torch.cuda.set_stream(side)
        try:
            out = fn()
        finally:
            torch.cuda.set_stream(main)
        for t in (out if isinstance(out, (tuple, list)) else (out,)):
            t.record_stream(main)
        return out

    def join_side(self):
        if self.side is not None:
            ev = torch.cuda.Event()
            ev.record(self.side)
            self.eng._wait("weight-gradient stream joined", self.main, ev)

    def wgrad(self, dy, x, KS, dil, Cout, Cin, **glu):
        if not self.pg:
            return None
        B, T, eng = self.B, self.T, self.eng
        nseg = layers.uniform_nseg(B, dy.shape[1], x.shape[1])
        _, seg = eng._uniform_segments(B, nseg, self.dev)
        if self.side is not None and not eng.reuse_workspace:
            # without the persistent workspace, dy is a buffer of this backward that is freed as soon as the loop moves on,
            # and the next main-stream allocation may take its memory before the side stream has read it
            dy.record_stream(self.side)
            x.record_stream(self.side)
        return self.on_side(lambda: layers.conv_wgrad(dy, x, B, T, KS, dil, Cout, Cin, seg, nseg, **glu))

    def dgrad(self, dy, key, out, KS, dil, res=None, widx=None, bn=None):
        """Data-gradient conv of the layer whose weight is P[key].  bn = (h, coef): `out` is the gradient entering
        GELU(BN(h)); the conv's epilogue then also emits the per-tile BatchNorm-backward sums (returned as second value) —
        the separate reduction pass over (out, h) is not needed."""
        # (the 128-row tile kernel, 40 KB of LDS per workgroup: the flat kernel's two 76 KB workgroups fill a CU's LDS and the
        # weight-gradient GEMMs of the side stream wait instead of running beside it; at s_setprio 3, so that the chain wins
        # each SIMD's issue arbitration against those GEMMs)
        bflags = L.CONV_WAVE_PRIO
        B, T, w, wT = self.B, self.T, self.P[key], self.ctx.packed_T[key]
        alg = (w.shape[-3], w.shape[-2])
        if bn is None or bn[1] is None:
            return ops.conv_gemm(dy, wT, out, B=B, T=T, KS=KS, dil=dil, res=res, widx=widx, alg_dims=alg, flags=bflags), None
        st = torch.empty((ops.conv_stats_rows(B, T, KS, out.shape[1], bflags), 2, out.shape[1]), dtype=torch.float32, device=self.dev)
        ops.conv_gemm(dy, wT, out, B=B, T=T, KS=KS, dil=dil, res=res, widx=widx, stats=st, bn_x=bn[0], bn_coef=bn[1],
                      alg_dims=alg, flags=bflags)
        return out, st


_Routes = namedtuple("_Routes", "conv2_glu_flat f2_wide f2_dgrad_gelu_flat")


class EncoderEngine:
    def __init__(self, dims: EncoderDims, dtype: torch.dtype = torch.float32, group=None):
        L.load()                          # fail loudly if the HIP extension is missing
        self.d = dims
        self.dtype = dtype
        self.group = group                # torch.distributed group for synchronised BatchNorm statistics
        self.overlap_grad_allreduce = True   # under DP: SUM all-reduce each layer group's gradients as soon as
                                             # they exist, on RCCL's stream, overlapped with the rest of backward
        self._ws: Dict[tuple, torch.Tensor] = {}
        self._ws_shapes: List[tuple] = []    # (space, B, T) groups in least-recently-used order
        self.max_workspace_shapes = 2        # per space: a ragged last batch gets a second set, a third shape evicts the oldest
        self._seg_cache: Dict[tuple, tuple] = {}
        self._gen = 0                        # generation of the TRAIN workspace (bumped by grad-mode forwards only)
        self.reuse_workspace = True
        # weight-gradient chains (wgrad_gemm -> reduce_slabs -> unpack) depend only on dy and a saved
        # activation, never on each other or on the data-gradient chain: run them on a second HIP stream
        self.wgrad_side_stream = True
        self.probe = None                    # diagnostics (tools/stream_waits.py): a list collects (label, event, event) around
                                             # every point where the main stream waits for another stream
        self.pack_on_side_stream = True      # per-step operand packing runs beside the first layers, not in front
        self.flat_tiles_forward = True       # k = 3 convs on the 256-row flat-tile kernel (conv3_flat.hip) where it applies (fp32
                                             # storage too: that instantiation runs 128-row tiles only — 80 accumulator registers
                                             # per wave, no scratch)
        self.fuse_glu_forward = True         # F.glu in conv2's epilogue (where conv2 routes to the flat-tile kernel): no [value | gate] buffer
        self.compose_subject_block = True    # SpatialAttention, the shared 1x1 conv and the per-subject 1x1 conv as ONE per-subject
                                             # matrix (needs a spare padding channel for the folded bias: C < Cp)
        self._side = {}
        self._const = {}                     # persistent operand buffers (composed SubjectBlock matrices)
        self._plan_key = None                # (device, dtype, glu_fused, composed) the cached pack plans were built for
        self._route_key = None               # storage type the cached kernel routes were asked for

        # diagnostics: SDA_ENGINE_<switch>=<python literal> overrides one of the SWITCHES above (plain bool / int / float
        # attributes set in this constructor: never a property, a buffer table or the dims)
        switches = {k for k, v in vars(self).items() if not k.startswith("_") and isinstance(v, (bool, int, float))}
        for key, val in os.environ.items():
            if not key.startswith("SDA_ENGINE_"):
                continue
            name = key[11:]
            if name not in switches:
                raise L.SdaError(f"{key}: no such engine switch (known: {', '.join(sorted(switches))})")
            try:
                lit = ast.literal_eval(val)
            except (ValueError, SyntaxError) as e:
                raise L.SdaError(f"{key}={val!r} is not a Python literal: {e}") from None
            if not isinstance(lit, (bool, int, float)):
                raise L.SdaError(f"{key}={val!r}: a switch takes a bool, int or float")
            setattr(self, name, lit)

    def _side_stream(self, dev) -> torch.cuda.Stream:
        """The weight-gradient / packing stream of `dev`, made on first use."""
        side = self._side.get(str(dev))
        if side is None:
            side = self._side[str(dev)] = torch.cuda.Stream(device=dev, priority=0)
        return side

    @property
    def world(self) -> int:
        if self.group is None:
            return 1
        import torch.distributed as dist
        return dist.get_world_size(self.group)

    def _allreduce(self, t: torch.Tensor):
        import torch.distributed as dist
        dist.all_reduce(t, op=dist.ReduceOp.SUM, group=self.group)

    # ------------------------------------------------------------------ workspace
    def _rows(self, name: str, B: int, T: int, Cp: int, device, space: str) -> torch.Tensor:
        key = (space, name, B, T, Cp, self.dtype, str(device))
        if self.reuse_workspace and key in self._ws:
            return self._ws[key]
        buf = ops.new_rows(B, T, Cp, self.dtype, device)
        if self.reuse_workspace:
            self._ws[key] = buf
        return buf

    def _touch_shape(self, space: str, B: int, T: int):
        """LRU over (space, B, T) buffer sets: a training run sees one batch shape plus, with drop_last=False, one
        ragged last batch; anything beyond `max_workspace_shapes` per space releases the least recently used set
        (a pending backward keeps its own buffers alive through its ctx)."""
        g = (space, B, T)
        if g in self._ws_shapes:
            self._ws_shapes.remove(g)
        self._ws_shapes.append(g)
        mine = [x for x in self._ws_shapes if x[0] == space]
        while len(mine) > self.max_workspace_shapes:
            old = mine.pop(0)
            self._ws_shapes.remove(old)
            for k in [k for k in self._ws if (k[0], k[2], k[3]) == old]:
                del self._ws[k]

    def release_workspace(self):
        self._ws.clear()
        self._ws_shapes.clear()
        self._seg_cache.clear()

    def _uniform_segments(self, B: int, nseg: int, device):
        """(perm, seg_start) on `device` of `nseg` runs of consecutive samples (perm None: no permutation table), made once."""
        key = (B, nseg, str(device))
        if key not in self._seg_cache:
            self._seg_cache[key] = (None, torch.from_numpy(layers.uniform_segment_edges(B, nseg)).to(device))
        return self._seg_cache[key]

    @property
    def composed(self) -> bool:
        return bool(self.compose_subject_block and self.d.C < self.d.Cp)

    @property
    def glu_fused(self) -> bool:
        return bool(self.fuse_glu_forward and self.flat_forward and self._routes().conv2_glu_flat)

    @property
    def flat_forward(self) -> bool:
        """Forward k = 3 convs on conv3_flat.hip (every storage type)."""
        return bool(self.flat_tiles_forward)

    def _wait(self, label: str, stream, event):
        """stream.wait_event(event); with a probe attached, bracketed by timing events (how long the stream sat idle)."""
        if self.probe is None:
            stream.wait_event(event)
            return
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(stream)
        stream.wait_event(event)
        e1.record(stream)
        self.probe.append((label, e0, e1))

    # ------------------------------------------------------------------ kernel routes and operand packing plans
    def _routes(self):
        """What depends on the kernel the library routes a conv to (ops.conv_kernel), asked once per storage type: conv2 with
        F.glu in its epilogue runs on conv3_flat, conv_final2 with the row sums of squares on conv1_wide, conv_final2's data
        gradient with conv_final1's GELU backward in its epilogue on conv1_flat."""
        if self._route_key != self.dtype:
            d, dt = self.d, self.dtype
            self._route = _Routes(ops.conv_kernel(3, 2 * d.D2p, L.CONV_FLAT_TILES | L.EPI_GLU, dt) == L.CONV_KERNEL_FLAT3,
                                  ops.conv_kernel(1, d.Fp, L.CONV_WIDE_TILES | L.EPI_ROW_SUMSQ, dt) == L.CONV_KERNEL_WIDE,
                                  ops.conv_kernel(1, d.F1p, L.CONV_FLAT_TILES | L.EPI_GELU_BWD, dt) == L.CONV_KERNEL_FLAT1)
            self._route_key = dt
        return self._route

    def _plans(self, P, dev):
        key = (str(dev), self.dtype, self.glu_fused, self.composed)
        if self._plan_key == key:
            return self._fwd_plan, self._bwd_plan
        d = self.d
        f, b = ops.PackPlan(self.dtype, dev), ops.PackPlan(self.dtype, dev)
        glu_tile = 80 if self.glu_fused else 0      # SDA_EPI_GLU's 80 value + 80 gate channels per tile
        if not self.composed:                # (the composed SubjectBlock builds its per-subject operand itself)
            layers.add_subject_block_packs(f, b, P["sb_w"], P["sb_b"], P["subj_w"], d.D1p)
        for k in range(5):
            layers.add_conv_block_packs(f, b, f"b{k}.", [(P[f"b{k}.c{j}w"], P[f"b{k}.c{j}b"]) for j in range(3)], d.D2,
                                        d.D1p if k == 0 else d.D2p, glu_tile)
        f.add_weight("f1w", P["f1w"], d.F1p, d.D2p)
        f.add_vector("f1b", P["f1b"], d.F1p)
        f.add_weight("f2w", P["f2w"], d.Fp, d.F1p)
        f.add_vector("f2b", P["f2b"], d.Fp)
        b.add_weight("f1w", P["f1w"], d.F1p, d.D2p, mode=1)
        b.add_weight("f2w", P["f2w"], d.Fp, d.F1p, mode=1)
        self._fwd_plan, self._bwd_plan, self._plan_key = f, b, key
        return f, b

    # ------------------------------------------------------------------ forward
    def forward(self, P: Dict[str, torch.Tensor], X: torch.Tensor, subject_idxs, *, training: bool,
                mask: Optional[torch.Tensor], need_grad: bool, momentum: float = 0.1, eps: float = 1e-5,
                need_dx: bool = False, param_grads: bool = True) -> EncoderCtx:
        """need_dx: the backward also returns the gradient of X (needs need_grad); param_grads = False (a frozen encoder, with
        need_dx): the backward runs the data-gradient chain only, and this forward builds nothing the weight gradients read."""
        B, Cc, T = X.shape
        assert Cc == self.d.C, f"expected {self.d.C} channels, got {Cc}"          # models.py:78
        dev = X.device
        if need_grad:                    # no-grad forwards live in the "eval" buffers: they leave a pending backward intact
            self._gen += 1
        self._touch_shape("train" if need_grad else "eval", B, T)
        ctx = EncoderCtx(B=B, T=T, gen=self._gen, training=training)
        ctx.glu_fused = self.glu_fused
        if need_dx and not need_grad:
            raise L.SdaError("EncoderEngine.forward: need_dx needs need_grad")
        ctx.param_grads = bool(param_grads or not need_dx)
        ctx.x_dtype = X.dtype if need_dx else None
        ctx.mask = mask
        # forward k = 3 convs (nothing competes for the CU's LDS there): two tiles per workgroup share each weight slab
        k3_flags = L.CONV_PAIR_TILES
        if self.flat_forward:
            k3_flags |= L.CONV_FLAT_TILES | L.CONV_FLAT_STAGGER     # a CU's second workgroup takes its 128-row tile first
        f = _Forward(self, P, ctx, dev, torch.cuda.current_stream(dev), need_grad, need_dx, eps, momentum, k3_flags,
                     count=float(B) * T * self.world)       # BatchNorm statistics span the GLOBAL batch under data parallelism

        self._fwd_subjects(f, subject_idxs)
        Xt = ctx.bufs["Xt"] = self._fwd_pack(f, X)
        x = self._fwd_subject_block(f, Xt)                   # models.py:111-117
        for k in range(5):                                   # models.py:152-166
            x = self._fwd_conv_block(f, k, x)
        Zt = self._fwd_projections(f, x)                     # models.py:194-195
        if not need_grad:
            ctx.bufs = {"Z": Zt}
            ctx.packed = {}
        return ctx

    def _fwd_subjects(self, f: _Forward, subject_idxs):
        """Validates the subject indices, uploads them and, for a backward with parameter gradients, the segments of the
        per-subject weight gradient."""
        d, ctx = self.d, f.ctx
        B = ctx.B
        sidx = layers.subject_indices(subject_idxs, B, d.S)
        up = ops.UPLOADER.upload                # pinned staging: no implicit host<->stream synchronisation
        ctx.widx = up(("widx", "train" if f.need_grad else "eval"), sidx.astype(np.int32), f.dev)
        if not (f.need_grad and ctx.param_grads):
            return
        tiles = layers.subject_tiles_composed(d.D2p, d.Cp) if self.composed else layers.subject_tiles_three_conv(d.D1p)
        plan = layers.subject_plan(sidx, d.S, *tiles)
        ctx.subj_perm = up("subj_perm", plan.perm, f.dev)
        ctx.subj_seg = up("subj_seg", plan.seg_start, f.dev)
        ctx.subj_slices = plan.r

    def _fwd_pack(self, f: _Forward, X):
        """Operand packing (fp32 master weights -> compute dtype, K-contiguous, zero padded): ONE launch per plan, and X's layout
        change; on the side stream (pack_on_side_stream) or in place.  Returns Xt."""
        d, ctx, P = self.d, f.ctx, f.P
        fwd_plan, bwd_plan = self._plans(P, f.dev)
        side = self._side_stream(f.dev) if self.pack_on_side_stream else None
        Xt = f.rows("Xt", d.Cp)                  # (before the event: a first-use buffer is zero-filled on the MAIN stream)
        if side is not None:
            ev = torch.cuda.Event()
            ev.record(f.main)                    # the optimiser's update of P is on the main stream
            side.wait_event(ev)
        with torch.cuda.stream(side):            # (None: stays on the main stream)
            ctx.packed.update(fwd_plan.run(P))
            # the input's layout change rides on the same stream: the main stream meanwhile computes the SpatialAttention
            # weights and composes the SubjectBlock matrices (parameter-sized work that needs neither)
            ops.pack_rows(X, Xt, ones_channel=d.C if self.composed else None)
            if side is not None:
                X.record_stream(side)
                f.packed_ready = torch.cuda.Event()
                f.packed_ready.record(side)
            if f.need_grad:
                ctx.packed_T = bwd_plan.run(P)      # [tap][ci][co] operands of the data-gradient convs
                if side is not None:
                    ctx.packed_T_ready = torch.cuda.Event()
                    ctx.packed_T_ready.record(side)
        return Xt

    def _fwd_subject_block(self, f: _Forward, Xt):
        """SubjectBlock (models.py:111-117), composed or as its three convs.  Returns x0."""
        d, ctx, P, dev = self.d, f.ctx, f.P, f.dev
        B, T, pk = ctx.B, ctx.T, ctx.packed
        composed = self.composed
        # (composed SubjectBlock: the SpatialAttention weights are wanted in fp32 — the "packed operand" W * mask then IS the
        # fp32 matrix the composition below multiplies)
        ctx.W_sa, Wp = ops.sa_weights_forward(P["z"], P["cos"], P["sin"], ctx.mask, d.D1p, d.Cp,
                                              torch.float32 if composed else self.dtype, fwd_table=P.get("sa_tab_f"))
        if not composed:
            ctx.W_x = Wp if f.need_dx else None          # (sa_weights_forward returns a fresh matrix per forward)
            if f.packed_ready is not None:
                self._wait("packed operands (forward)", f.main, f.packed_ready)
            h_sa = ops.conv_gemm(Xt, Wp, f.rows("h_sa", d.D1p), B=B, T=T, KS=1, dil=0, alg_dims=(d.C, d.D1))
            h_c = ops.conv_gemm(h_sa, pk["sb_w"], f.rows("h_c", d.D1p), B=B, T=T, KS=1, dil=0, bias=pk["sb_b"],
                                alg_dims=(d.D1, d.D1))
            x = ops.conv_gemm(h_c, pk["subj_w"], f.rows("x0", d.D1p), B=B, T=T, KS=1, dil=0, widx=ctx.widx, alg_dims=(d.D1, d.D1))
            ctx.bufs.update(h_sa=h_sa, h_c=h_c, x0=x)
            return x
        # models.py:111-117 is three linear maps in a row with nothing between them: x0 = W_subj[s] (W_sb (W_sa X) + b_sb).
        # Composed per subject in fp32 parameter space — (S, D1, C + 1) with the bias riding on Xt's constant channel —
        # one per-sample-weight GEMM replaces three, and the backward needs no data gradient at all here (X is an input):
        # one per-subject weight gradient, then the chain rule on (S, D1, C)-sized matrices.  All of these small products
        # run on ops.param_gemm (exact-fp32 MFMA on strided views: no padding, packing, cat or copy around them).
        Wd = Wp[0, 0, : d.D1, : d.C]                                                         # W_sa * mask, (D1, C) view
        Ws = P["subj_w"][..., 0]                                                             # (S, D1, D1) view
        T1aug = torch.empty((d.D1, d.C + 1), dtype=torch.float32, device=dev)               # [W_sb W_d | b_sb]
        ops.param_gemm(P["sb_w"][..., 0], Wd, out=T1aug[:, : d.C])
        ops.copy3d(T1aug[:, d.C:], P["sb_b"][:, None])
        key = ("wtot", str(dev), self.dtype)
        Wtot = self._const.get(key)
        if f.need_dx:
            # the backward contracts dx0 with THIS matrix: a copy of the forward's own, which a later forward (a no-grad one
            # between this forward and its backward included) cannot rewrite
            Wtot = ctx.W_x = ops.zeros((d.S, 1, d.D1p, d.Cp), self.dtype, dev)
        elif Wtot is None:
            Wtot = self._const[key] = torch.zeros((d.S, 1, d.D1p, d.Cp), dtype=self.dtype, device=dev)
        ops.param_gemm(Ws, T1aug, out=Wtot[:, 0, : d.D1, : d.C + 1])                      # rounded to the compute dtype on the way out
        if f.need_grad:
            ctx.composed = (Wd, T1aug, Ws)
        if f.packed_ready is not None:
            self._wait("packed operands (forward)", f.main, f.packed_ready)
        x = ctx.bufs["x0"] = ops.conv_gemm(Xt, Wtot, f.rows("x0", d.D1p), B=B, T=T, KS=1, dil=0, widx=ctx.widx,
                                           alg_dims=(d.C, d.D1))
        return x

    def _fwd_conv_block(self, f: _Forward, k: int, x):
        """ConvBlock k (models.py:152-166) on input x.  Returns its output."""
        d, ctx, P, dev = self.d, f.ctx, f.P, f.dev
        B, T, pk, bufs, k3_flags, count = ctx.B, ctx.T, ctx.packed, ctx.bufs, f.k3_flags, f.count
        dil = layers.block_dilations(k)
        for j in (0, 1):
            alg = (d.D1 if (k == 0 and j == 0) else d.D2, d.D2)
            pre = f"b{k}.c{j}"
            w, bias = pk[pre + "w"], pk[pre + "b"]
            res = x if (j == 1 or k > 0) else None
            h = f.rows(f"b{k}.h{j}", d.D2p)
            bnp = f"b{k}.bn{j}"
            if ctx.training:
                nt = ops.conv_stats_rows(B, T, 3, d.D2p, k3_flags)
                stats = torch.empty((nt, 2, d.D2p), dtype=torch.float32, device=dev)
                ops.conv_gemm(x, w, h, B=B, T=T, KS=3, dil=dil[j], bias=bias, res=res, stats=stats, alg_dims=alg,
                              flags=k3_flags)
                if self.group is not None:   # one 2*Cp-float all-reduce per BatchNorm
                    # (the column-sum kernel, ~10 us; the generic slab sum took 34 us per BatchNorm on this chain)
                    stats = ops.reduce_stats(stats).view(1, 2, d.D2p)
                    self._allreduce(stats)
                    nt = 1
                mean, rstd, scale, shift, bcoef = ops.bn_finalize(stats, nt, count, P[bnp + "w"], P[bnp + "b"],
                                                                  P[bnp + "rm"], P[bnp + "rv"], d.D2p, True, f.eps, f.momentum,
                                                                  want_bwd_coef=True, batches_tracked=P.get(bnp + "nbt"))
            else:
                ops.conv_gemm(x, w, h, B=B, T=T, KS=3, dil=dil[j], bias=bias, res=res, alg_dims=alg, flags=k3_flags)
                # (the backward coefficient table only when a backward may follow: eval-mode BatchNorm is then a fixed
                # per-channel affine map on the running statistics)
                mean, rstd, scale, shift, *rest = ops.bn_finalize(None, 0, count, P[bnp + "w"], P[bnp + "b"], P[bnp + "rm"],
                                                                  P[bnp + "rv"], d.D2p, False, f.eps, f.momentum,
                                                                  want_bwd_coef=f.need_grad)
                bcoef = rest[0] if rest else None
            ctx.bn[bnp] = (mean, rstd, bcoef)
            a = ops.bn_gelu_forward(h, f.rows(f"b{k}.a{j}", d.D2p), scale, shift, B, T)
            bufs[f"b{k}.h{j}"], bufs[f"b{k}.a{j}"] = h, a
            x = a
        w, bias = pk[f"b{k}.c2w"], pk[f"b{k}.c2b"]
        if ctx.glu_fused:        # F.glu in the conv's epilogue: only the product and (for backward) the gate are stored
            gate = f.rows(f"b{k}.g", d.D2p) if f.need_grad else None
            x = ops.conv_gemm(x, w, f.rows(f"x{k + 1}", d.D2p), B=B, T=T, KS=3, dil=dil[2], bias=bias, y_pre=gate,
                              alg_dims=(d.D2, 2 * d.D2), flags=k3_flags | L.EPI_GLU)
            bufs[f"b{k}.g"], bufs[f"x{k + 1}"] = gate, x
        else:
            c2 = ops.conv_gemm(x, w, f.rows(f"b{k}.c2", 2 * d.D2p), B=B, T=T, KS=3, dil=dil[2], bias=bias,
                               alg_dims=(d.D2, 2 * d.D2), flags=k3_flags)
            x = ops.glu_forward(c2, f.rows(f"x{k + 1}", d.D2p), B, T)
            bufs[f"b{k}.c2"], bufs[f"x{k + 1}"] = c2, x
        return x

    def _fwd_projections(self, f: _Forward, x):
        """The two 1x1 projections with GELU (models.py:194-195).  Returns Zt."""
        d, dt, ctx, dev = self.d, self.dtype, f.ctx, f.dev
        B, T, pk, need_grad = ctx.B, ctx.T, ctx.packed, f.need_grad
        u1, g1 = f.rows("u1", d.F1p), f.rows("g1", d.F1p)
        f2_wide = self._routes().f2_wide         # conv_final2 on conv1_wide.hip's 256-row tiles where storage type and width allow
        ops.conv_gemm(x, pk["f1w"], g1, B=B, T=T, KS=1, dil=0, bias=pk["f1b"], y_pre=u1 if need_grad else None,
                      gelu=True, alg_dims=(d.D2, d.F1))
        # Z is handed to the caller: a FRESH buffer per forward (the reference returns a new tensor each call), so
        # embeddings kept across forwards stay valid; everything else lives in the reused workspace
        u2, Zt = f.rows("u2", d.Fp), ops.new_rows_uninit(B, T, d.Fp, dt, dev)
        # ||Z_b||^2 for the loss comes out of the epilogue's sums: no separate pass over Z (loss.py:65)
        if f2_wide:
            zparts = torch.empty((B * L.rows_tp(T), d.Fp // 128), dtype=torch.float32, device=dev)
            ops.conv_gemm(g1, pk["f2w"], Zt, B=B, T=T, KS=1, dil=0, bias=pk["f2b"], y_pre=u2 if need_grad else None,
                          gelu=True, row_sumsq=zparts, alg_dims=(d.F1, d.F), flags=L.CONV_WIDE_TILES)
            ops.ROW_NORMS.put(Zt, ops.rows_sumsq_from_row_parts(zparts, B, T))
        else:
            zstats = torch.empty((B * ops.n_t_tiles(T), 2, d.Fp), dtype=torch.float32, device=dev)
            ops.conv_gemm(g1, pk["f2w"], Zt, B=B, T=T, KS=1, dil=0, bias=pk["f2b"], y_pre=u2 if need_grad else None,
                          gelu=True, stats=zstats, alg_dims=(d.F1, d.F))
            ops.ROW_NORMS.put(Zt, ops.rows_sumsq_from_stats(zstats, B))
        ctx.bufs.update(u1=u1, g1=g1, u2=u2, Z=Zt)
        return Zt

    # ------------------------------------------------------------------ backward
    def backward(self, P: Dict[str, torch.Tensor], ctx: EncoderCtx, dZt: torch.Tensor) -> Dict[str, torch.Tensor]:
        """The parameters' gradients by name (none for a frozen encoder: ctx.param_grads False) and, when the forward had
        need_dx, grads["X"] = dL/dX as a contiguous (B, C, T) tensor of X's dtype."""
        if ctx.gen != self._gen and self.reuse_workspace:
            raise L.SdaError("the activation workspace of this forward was overwritten by a later forward of the same "
                             "encoder; call backward before the next training-mode forward, or set "
                             "engine.reuse_workspace = False")
        d, dev = self.d, dZt.device
        main = torch.cuda.current_stream(dev)
        if ctx.packed_T_ready is not None:
            self._wait("packed operands (backward)", main, ctx.packed_T_ready)
        b = _Backward(self, P, ctx, dev, main)
        composed = ctx.composed is not None
        w0cat = self._bwd_w0cat(b) if composed and b.pg else None
        dx = self._bwd_projections(b, dZt)
        # the gradient of the ten biases that feed a training-mode BatchNorm (identically zero): rows of ONE fresh zero buffer
        # per backward — autograd hands these views to the parameters' .grad, so a buffer kept across steps would alias
        # engine-owned memory into .grad (an in-place clip with a non-finite factor would poison every later step)
        null_bias = ops.zeros((10, d.D2), torch.float32, dev) if ctx.training and b.pg else None
        for k in range(4, -1, -1):
            dx, dh0 = self._bwd_conv_block(b, k, dx, null_bias)
        if composed:
            self._bwd_subject_composed(b, dx, dh0, w0cat)
        else:
            self._bwd_subject_three_conv(b, dx)
        # (a frozen encoder, pg False, has nothing to flush and nothing pending: it only joins the side stream)
        b.flush(["subj_w", "sb_w", "sb_b", "z"])
        b.join_side()
        for work in b.pending:
            work.wait()                       # makes the current stream wait for RCCL's; no host sync
        return b.grads

    def _bwd_w0cat(self, b: _Backward):
        """Block 0's conv0 weights as [d][tap][o] (o zero-padded to D2p; the padding is written once), the left operand of the
        composed SubjectBlock's gradient at the END of backward: a parameter-only copy, so it is made at the start, on the
        weight-gradient stream while that has nothing to do, not in the serial tail of the step.  Returns (W0cat, event)."""
        d = self.d
        key = ("w0cat", str(b.dev))
        W0cat = self._const.get(key)
        if W0cat is None:
            W0cat = self._const[key] = torch.zeros((d.D1, 3, d.D2p), dtype=torch.float32, device=b.dev)
        b.on_side(lambda: ops.copy3d(W0cat[:, :, : d.D2], b.P["b0.c0w"].permute(1, 2, 0)))
        # its reader (the G product at the end of backward) runs on the MAIN stream: an event of the side stream right
        # behind the copy, waited for just before that product (long complete by then: the wait costs nothing, and the
        # result no longer depends on how far the side stream has got)
        ready = None
        if b.side is not None:
            ready = torch.cuda.Event()
            ready.record(b.side)
        return W0cat, ready

    def _bwd_projections(self, b: _Backward, dZt):
        """Backward of the two 1x1 projections: f2w, f2b, f1w, f1b.  Returns the gradient entering block 4's F.glu."""
        d, bufs, grads, pg = self.d, b.ctx.bufs, b.grads, b.pg
        B, T, dev, scratch, packed_T = b.B, b.T, b.dev, b.scratch, b.ctx.packed_T
        du2 = b.tmp("du2", d.Fp)
        if pg:
            grads["f2b"] = ops.bias_grad(ops.gelu_backward_colsum(bufs["u2"], dZt, du2, B, T, scratch), d.F)
        else:
            ops.gelu_backward(bufs["u2"], dZt, du2, B, T)
        # the 1x1 data gradients on conv1_flat.hip's 256-row flat tiles
        du1 = b.tmp("du1", d.F1p)
        if self._routes().f2_dgrad_gelu_flat:
            # conv_final2's data gradient with conv_final1's GELU backward in its epilogue: du1 directly, plus per-unit column sums
            gst = torch.empty((ops.conv_stats_rows(B, T, 1, d.F1p, L.CONV_FLAT_TILES | L.EPI_GELU_BWD), 2, d.F1p),
                              dtype=torch.float32, device=dev)
            ops.conv_gemm(du2, packed_T["f2w"], du1, B=B, T=T, KS=1, dil=0, gelu_bwd_u=bufs["u1"], stats=gst,
                          alg_dims=(d.F, d.F1), flags=L.CONV_FLAT_TILES)
            grads["f2w"] = b.wgrad(du2, bufs["g1"], 1, 0, d.F, d.F1)
            if pg:
                if b.side is not None:
                    gst.record_stream(b.side)     # a buffer of this stage, read on the side stream after the stage has returned
                grads["f1b"] = b.on_side(lambda: ops.bias_grad(ops.reduce_stats(gst)[:d.F1p], d.F1))
        else:
            dg1, _ = b.dgrad(du2, "f2w", b.tmp("dg1", d.F1p), 1, 0)
            grads["f2w"] = b.wgrad(du2, bufs["g1"], 1, 0, d.F, d.F1)
            if pg:
                grads["f1b"] = ops.bias_grad(ops.gelu_backward_colsum(bufs["u1"], dg1, du1, B, T, scratch), d.F1)
            else:
                ops.gelu_backward(bufs["u1"], dg1, du1, B, T)
        dx = ops.conv_gemm(du1, packed_T["f1w"], b.tmp("dxA", d.D2p), B=B, T=T, KS=1, dil=0, alg_dims=(d.F1, d.D2),
                           flags=L.CONV_FLAT_TILES)
        grads["f1w"] = b.wgrad(du1, bufs["x5"], 1, 0, d.F1, d.D2)
        b.flush(["f2w", "f2b", "f1w", "f1b"])
        return dx

    def _bwd_conv_block(self, b: _Backward, k: int, dx, null_bias):
        """Backward of ConvBlock k from dx, the gradient of its output.  Returns (gradient of its input, dh of conv0): for block 0
        of a composed SubjectBlock the first is None unless X wants a gradient."""
        d, ctx, P, grads, pg = self.d, b.ctx, b.P, b.grads, b.pg
        B, T, bufs, scratch, world = b.B, b.T, ctx.bufs, b.scratch, b.world
        cin, cin_p = (d.D1, d.D1p) if k == 0 else (d.D2, d.D2p)
        dil = layers.block_dilations(k)
        glu = dict(glu_half=d.D2, glu_half_p=d.D2p)       # (c2's bias gradient: a kernel when D2 is not a multiple of 64)
        dc2 = b.tmp(f"dc2.{k}", 2 * d.D2p)      # per-layer buffers: a side-stream wgrad may still read them
        if not pg:
            if ctx.glu_fused:
                ops.glu_backward_og(bufs[f"x{k + 1}"], bufs[f"b{k}.g"], dx, dc2, B, T)
            else:
                ops.glu_backward(bufs[f"b{k}.c2"], dx, dc2, B, T)
        elif ctx.glu_fused:
            grads[f"b{k}.c2b"] = ops.bias_grad(ops.glu_backward_colsum_og(bufs[f"x{k + 1}"], bufs[f"b{k}.g"], dx, dc2, B, T, scratch),
                                               2 * d.D2, **glu)
        else:
            grads[f"b{k}.c2b"] = ops.bias_grad(ops.glu_backward_colsum(bufs[f"b{k}.c2"], dx, dc2, B, T, scratch), 2 * d.D2, **glu)
        da1, tstats = b.dgrad(dc2, f"b{k}.c2w", b.tmp("da", d.D2p), 3, dil[2], bn=(bufs[f"b{k}.h1"], ctx.bn[f"b{k}.bn1"][2]))
        # the weight-gradient chain is queued AFTER the data-gradient conv: on the side stream it then runs
        # beside the HBM-bound BatchNorm backward kernels that follow, not beside the MFMA-bound conv
        grads[f"b{k}.c2w"] = b.wgrad(dc2, bufs[f"b{k}.a1"], 3, dil[2], 2 * d.D2, d.D2, **glu)
        for j in (1, 0):
            bnp = f"b{k}.bn{j}"
            mean, rstd, _ = ctx.bn[bnp]
            dh = b.tmp(f"dh.{k}.{j}", d.D2p)
            # eval-mode BatchNorm (running statistics) has no batch-statistics terms in its input gradient: an infinite
            # count zeroes them (dbeta / N, dgamma / N) while dgamma / dbeta themselves stay the plain sums, rank-local
            sync = self.group is not None and ctx.training
            dgam, dbet = ops.bn_gelu_backward(da1, bufs[f"b{k}.h{j}"], mean, rstd, P[bnp + "w"], P[bnp + "b"], dh, B, T,
                                              scratch, count=float(B) * T * world if ctx.training else float("inf"),
                                              allreduce=self._allreduce if sync else None, tile_stats=tstats)
            # under DP the sums are already global on every rank; the gradient all-reduce (SUM) follows
            if sync and pg:
                # (one launch for both rows, on the weight-gradient stream: only the optimiser reads these)
                both = dgam._base if dgam._base is not None else torch.stack([dgam, dbet])
                if b.side is not None:
                    both.record_stream(b.side)
                scaled = b.on_side(lambda: both / world)
                dgam, dbet = scaled[0], scaled[1]
            if pg:
                grads[bnp + "w"], grads[bnp + "b"] = dgam[: d.D2], dbet[: d.D2]
                # conv0/conv1 feed a training-mode BatchNorm, which removes any per-channel constant: the bias
                # gradient is identically zero (the reference's autograd reports rounding noise there)
                grads[f"b{k}.c{j}b"] = null_bias[2 * k + j] if ctx.training else ops.bias_grad(ops.colsum(dh, B, T, scratch), d.D2)
            src, ci, ci_p = (bufs[f"b{k}.a0"], d.D2, d.D2p) if j == 1 else (bufs[f"x{k}"], cin, cin_p)
            key = f"b{k}.c{j}w"
            res = dh if (j == 1 or k > 0) else None
            # (the blocks' input gradients alternate between two buffers: block k reads the one block k + 1 wrote, and the
            # projections wrote dxA for block 4)
            out = b.tmp("da", d.D2p) if j == 1 else b.tmp("dxB" if k % 2 == 0 else "dxA", ci_p)
            if k == 0 and j == 0 and ctx.composed is not None and ctx.x_dtype is None:
                # the composed SubjectBlock takes its weight gradient straight from dh0 and X: the gradient with
                # respect to x0 is needed only for X's gradient, and this data-gradient conv runs only then
                da1 = None
            else:
                da1, tstats = b.dgrad(dh, key, out, 3, dil[j], res=res,
                                      bn=(bufs[f"b{k}.h0"], ctx.bn[f"b{k}.bn0"][2]) if j == 1 else None)
            grads[key] = b.wgrad(dh, src, 3, dil[j], d.D2, ci)
        b.flush([f"b{k}.c2w", f"b{k}.c2b", f"b{k}.c1w", f"b{k}.c1b", f"b{k}.bn1w", f"b{k}.bn1b",
                 f"b{k}.c0w", f"b{k}.c0b", f"b{k}.bn0w", f"b{k}.bn0b"])
        return da1, dh

    def _bwd_subject_composed(self, b: _Backward, dx, dh0, w0cat):
        """Backward of the composed SubjectBlock: X's gradient from dx (block 0's input gradient) when asked for; subj_w, sb_w,
        sb_b and z from dh0 (block 0's conv0 output gradient) and X."""
        d, ctx, P, grads = self.d, b.ctx, b.P, b.grads
        B, T, dev = b.B, b.T, b.dev
        if ctx.x_dtype is not None:
            # dX[b] = Wtot[s_b]^T dx0[b]: columns < C of the forward's own matrix (the bias column C and the pad columns
            # are not read out), stored straight into a plain (B, C, T) tensor of X's dtype
            grads["X"] = ops.input_grad(dx, ctx.W_x, ctx.widx, B, d.C, T, ctx.x_dtype)
        if not b.pg:
            return
        Wd, T1aug, Ws = ctx.composed
        W0cat, w0cat_ready = w0cat
        r = ctx.subj_slices
        # x0 = W_tot[s] X feeds block 0's conv0 and nothing else, and h0 = sum_tap W0[tap] x0[t + (tap - 1) dil], so
        #   dL/dW_tot[s] = sum_tap W0[tap]^T M[s][tap],   M[s][tap] = sum_{b in s, t} dh0[b, t] (x) X[b, t + (tap - 1) dil]
        # = the per-subject kernel-3 weight gradient of (dh0, X) followed by one batched (D1 x 3 D2) . (3 D2 x C+1) product:
        # neither conv0's data gradient (a 320 -> 320 kernel-3 conv) nor a weight gradient over dx0 is computed.
        M = ops.wgrad_gemm(dh0, ctx.bufs["Xt"], B=B, T=T, KS=3, dil=layers.block_dilations(0)[0], perm=ctx.subj_perm,
                           seg_start=ctx.subj_seg, nseg=r * d.S, flat_rows=True)     # (r*S, 3, D2p, Cp); column C: the folded bias
        if r > 1:
            M = ops.reduce_slabs(M.view(r, -1))
        if w0cat_ready is not None:
            self._wait("W0cat copy (side stream)", b.main, w0cat_ready)
        G = ops.param_gemm(W0cat.view(d.D1, 3 * d.D2p), M.view(d.S, 3 * d.D2p, d.Cp)[:, :, : d.C + 1])   # (S, D1, C + 1)
        # The chain to the last gradient of the step is M -> G -> W_subj^T G -> dT1 -> dWd -> dz; the products that only
        # the optimiser reads (subj_w, sb_w, sb_b) leave it for the weight-gradient stream
        grads["subj_w"] = b.on_side(lambda: ops.param_gemm(G, T1aug.t()).view(d.S, d.D1, d.D1, 1))   # W_tot[s] = W_subj[s] T1aug
        part = ops.param_gemm(Ws.transpose(1, 2), G)                                         # W_subj[s]^T G[s] per subject ...
        dT1f = ops.reduce_slabs(part.view(d.S, -1)).view(d.D1, d.C + 1)                      # ... summed in subject order
        dT1 = dT1f[:, : d.C]
        grads["sb_b"], grads["sb_w"] = b.on_side(lambda: (
            ops.copy3d(torch.empty(d.D1, dtype=torch.float32, device=dev), dT1f[:, d.C]),
            ops.param_gemm(dT1, Wd.t()).unsqueeze(-1)))
        dWd = ops.param_gemm(P["sb_w"][..., 0].t(), dT1)
        # (inside this stage: G, dT1f and dT1 are read on the side stream and stay alive until the main stream's last allocation)
        grads["z"] = ops.sa_weights_backward(dWd, ctx.W_sa, ctx.mask, P["cosT"], P["sinT"], P["z"].shape[1],
                                             bwd_table=P.get("sa_tab_b"))

    def _bwd_subject_three_conv(self, b: _Backward, dhs):
        """Backward of the SubjectBlock run as its three convs, from dhs (rows, D1p), block 0's input gradient."""
        d, ctx, P, grads, pg = self.d, b.ctx, b.P, b.grads, b.pg
        B, T, bufs = b.B, b.T, ctx.bufs
        if pg:
            grads["subj_w"] = b.on_side(lambda: layers.subject_wgrad(dhs, bufs["h_c"], B, T, ctx.subj_perm, ctx.subj_seg,
                                                                     ctx.subj_slices, d.S, d.D1))
        dh_c, _ = b.dgrad(dhs, "subj_w", b.tmp("dh_c", d.D1p), 1, 0, widx=ctx.widx)
        if pg:
            grads["sb_w"] = b.wgrad(dh_c, bufs["h_sa"], 1, 0, d.D1, d.D1)
            grads["sb_b"] = ops.bias_grad(ops.colsum(dh_c, B, T, b.scratch), d.D1)
        dh_sa, _ = b.dgrad(dh_c, "sb_w", b.tmp("dh_sa", d.D1p), 1, 0)
        if ctx.x_dtype is not None:
            # dX[b] = Wp^T dh_sa[b]: Wp is the forward's packed W_sa * mask (one matrix for every sample)
            grads["X"] = ops.input_grad(dh_sa, ctx.W_x, None, B, d.C, T, ctx.x_dtype)
        if not pg:
            return
        nseg = layers.uniform_nseg(B, d.D1p, d.Cp)
        _, seg = self._uniform_segments(B, nseg, b.dev)
        grads["z"] = layers.sa_z_grad(dh_sa, bufs["Xt"], B, T, seg, nseg, ctx.W_sa, ctx.mask, P["cosT"], P["sinT"], P["z"].shape[1],
                                      P.get("sa_tab_b"))

