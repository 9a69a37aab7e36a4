"""Stage schedules of the standalone `SpatialAttention`, `SubjectBlock` and `ConvBlock` (models.py:14-166): forward and
backward of one module call as plain serial launches of libsdamd.so kernels on the current stream.

These are NOT the encoder's step.  `EncoderEngine` runs the same stages fused into one node (composed SubjectBlock, GLU in
the conv epilogue, side streams, overlapped all-reduce) over a reused workspace; the schedules here take none of that and
share none of its state: every call allocates its own row-layout (RL) buffers, packs its own operands through a plan owned
by the module, and issues no collective (BatchNorm statistics stay local to the rank, as with a plain nn.BatchNorm1d).

Activations travel as RL buffers (rows of Cp channels).  An input that is an RL view made by this package in
the compute dtype is consumed with no copy; any other (B, C, T) device tensor is packed in one pass by ops.pack_rows.
"""
from __future__ import annotations

from dataclasses import dataclass, field
from typing import Dict, Optional

import numpy as np
import torch

from . import lib as L
from . import layers
from . import ops

FWD_FLAGS = L.CONV_PAIR_TILES            # the forward k = 3 convs of the encoder: two tiles per workgroup share a weight slab
BWD_FLAGS = L.CONV_WAVE_PRIO             # the data-gradient convs of the encoder's backward


# ------------------------------------------------------------------------------------------------------------- operands
def rows_in(X: torch.Tensor, Cc: int, dtype):
    """ops.rows_of for a module input: (RL buffer, True) for a row-layout view of `dtype` made by this package (zero copy); else
    (X packed into a fresh RL buffer of `dtype`, False).  X: a (B, C, T) device tensor of fp32 / bf16 / fp16."""
    if X.dtype not in ops.COMPUTE_DTYPES:
        raise L.SdaError(f"input of dtype {X.dtype}: the modules take float32, bfloat16 or float16")
    return ops.rows_of(X, Cc, dtype, ops.new_rows_uninit)


def grad_rows(dY: torch.Tensor, Cc: int, dtype) -> torch.Tensor:
    """The incoming gradient of a module output as an RL buffer of `dtype` (zero copy when it already is one)."""
    return ops.rows_of(dY, Cc, dtype, ops.new_rows_uninit)[0]


def _new(B: int, T: int, Cp: int, dtype, dev) -> torch.Tensor:
    # every valid row (channel padding included) is written by the producing kernel; the pad rows are zeroed here
    return ops.new_rows_uninit(B, T, Cp, dtype, dev)


def _segments(B: int, dy, x):
    """Sample segments of the weight-gradient launch of (dy, x): consecutive samples, a multiple of 8 segments (one per XCD round)."""
    nseg = layers.uniform_nseg(B, dy.shape[1], x.shape[1])
    return ops.UPLOADER.upload("blocks.seg", layers.uniform_segment_edges(B, nseg), dy.device), nseg


def _wgrad(dy, x, B, T, KS, dil, Cout, Cin, glu_half=0, glu_half_p=0) -> torch.Tensor:
    """Parameter-layout weight gradient (Cout, Cin, KS) fp32 of a conv with output gradient dy and input x (RL buffers)."""
    return layers.conv_wgrad(dy, x, B, T, KS, dil, Cout, Cin, *_segments(B, dy, x), glu_half=glu_half, glu_half_p=glu_half_p)


def _plans(module, dev, build):
    """The module's own (forward, backward) operand pack plans for device `dev` and its compute dtype, built once by `build`."""
    key = (str(dev), module.compute_dtype)
    plans = module.__dict__.setdefault("_block_plans", {})
    if key not in plans:
        plans[key] = build(ops.PackPlan(module.compute_dtype, dev), ops.PackPlan(module.compute_dtype, dev))
    return plans[key]


def _check_versions(ctx):
    if [p._version for p in ctx.params] != ctx.versions:
        raise RuntimeError("a parameter of this module was modified in place between its forward and its backward")


# ----------------------------------------------------------------------------------------------------- SpatialAttention
@dataclass
class SACtx:
    B: int
    T: int
    Xt: torch.Tensor
    W: torch.Tensor                     # fp32 softmax weights (D1, C), without the mask
    Wp: torch.Tensor                    # the packed (W * mask) operand the forward applied (compute dtype)
    mask: Optional[torch.Tensor]
    x_dtype: torch.dtype


def sa_forward(sa, Xt: torch.Tensor, B: int, T: int, mask, dtype):
    """models.py:45-65 + SpatialDropout: returns (RL output (D1p wide), W, Wp)."""
    D1, Cc = sa.z.shape[0], sa.cos.shape[1]
    D1p, Cp = L.pad_channels(D1), L.pad_channels(Cc)
    tab_f, _ = sa.gemm_tables()
    W, Wp = ops.sa_weights_forward(sa.z.detach(), sa.cos, sa.sin, mask, D1p, Cp, dtype, fwd_table=tab_f)
    y = ops.conv_gemm(Xt, Wp, _new(B, T, D1p, dtype, Xt.device), B=B, T=T, KS=1, dil=0, alg_dims=(Cc, D1))
    return y, W, Wp


def sa_backward(sa, c: SACtx, dY: torch.Tensor, want_x: bool, want_z: bool):
    """dY: RL gradient of the output (D1p wide, compute dtype).  Returns (dX contiguous of X's dtype or None, dz or None)."""
    Cc = sa.cos.shape[1]
    dX = ops.input_grad(dY, c.Wp, None, c.B, Cc, c.T, c.x_dtype) if want_x else None
    dz = None
    if want_z:
        dz = layers.sa_z_grad(dY, c.Xt, c.B, c.T, *_segments(c.B, dY, c.Xt), c.W, c.mask, *sa.transposed_tables(), sa.z.shape[1],
                              sa.gemm_tables()[1])
    return dX, dz


def spatial_attention_forward(sa, X: torch.Tensor, mask, need_grad: bool):
    B, Cc, T = X.shape
    Xt, _ = rows_in(X, Cc, sa.compute_dtype)
    y, W, Wp = sa_forward(sa, Xt, B, T, mask, sa.compute_dtype)
    return y, (SACtx(B, T, Xt, W, Wp, mask, X.dtype) if need_grad else None)


# --------------------------------------------------------------------------------------------------------- SubjectBlock
@dataclass
class SBCtx:
    sa: SACtx
    h_sa: torch.Tensor
    h_c: torch.Tensor
    widx: torch.Tensor
    subj: Optional[tuple] = None        # (perm, seg_start, slices) of the per-subject weight gradient
    params: list = field(default_factory=list)
    versions: list = field(default_factory=list)


def _sb_plans(sb):
    D1p = L.pad_channels(sb.D1)

    def build(f, b):
        layers.add_subject_block_packs(f, b, sb.conv.weight, sb.conv.bias, sb.subject_layer.weight, D1p)
        return f, b
    return _plans(sb, sb.conv.weight.device, build)


def _sb_sources(sb) -> Dict[str, torch.Tensor]:
    return {"sb_w": sb.conv.weight.detach(), "sb_b": sb.conv.bias.detach(), "subj_w": sb.subject_layer.weight.detach()}


def subject_block_forward(sb, X: torch.Tensor, sidx: np.ndarray, mask, need_grad: bool, want_subj_grad: bool):
    """models.py:111-117 as three maps: SpatialAttention GEMM, the shared 1x1 conv with bias, the per-subject 1x1 conv
    (sample b through weight matrix sidx[b])."""
    B, Cc, T = X.shape
    dt, dev, D1, S = sb.compute_dtype, X.device, sb.D1, sb.num_subjects
    D1p = L.pad_channels(D1)
    widx = ops.UPLOADER.upload("blocks.widx", sidx.astype(np.int32), dev)
    Xt, _ = rows_in(X, Cc, dt)
    h_sa, W, Wp = sa_forward(sb.spatial_attention, Xt, B, T, mask, dt)
    pk = _sb_plans(sb)[0].run(_sb_sources(sb))
    h_c = ops.conv_gemm(h_sa, pk["sb_w"], _new(B, T, D1p, dt, dev), B=B, T=T, KS=1, dil=0, bias=pk["sb_b"], alg_dims=(D1, D1))
    y = ops.conv_gemm(h_c, pk["subj_w"], _new(B, T, D1p, dt, dev), B=B, T=T, KS=1, dil=0, widx=widx, alg_dims=(D1, D1))
    if not need_grad:
        return y, None
    c = SBCtx(SACtx(B, T, Xt, W, Wp, mask, X.dtype), h_sa, h_c, widx)
    if want_subj_grad:
        plan = layers.subject_plan(sidx, S, *layers.subject_tiles_blocks(D1p))
        c.subj = (ops.UPLOADER.upload("blocks.subj_perm", plan.perm, dev), ops.UPLOADER.upload("blocks.subj_seg", plan.seg_start, dev),
                  plan.r)
    return y, c


def subject_block_backward(sb, c: SBCtx, dY: torch.Tensor, want: Dict[str, bool]) -> Dict[str, torch.Tensor]:
    """want: X, z, sb_w, sb_b, subj_w -> the gradients asked for (subj_w: (S, D1, D1, 1), zero for absent subjects)."""
    _check_versions(c)
    B, T, dt, dev = c.sa.B, c.sa.T, sb.compute_dtype, dY.device
    D1, S = sb.D1, sb.num_subjects
    D1p = L.pad_channels(D1)
    g: Dict[str, torch.Tensor] = {}
    if want["subj_w"]:
        g["subj_w"] = layers.subject_wgrad(dY, c.h_c, B, T, *c.subj, S, D1)
    if not (want["sb_w"] or want["sb_b"] or want["z"] or want["X"]):
        return g
    pkT = _sb_plans(sb)[1].run(_sb_sources(sb))
    dh_c = ops.conv_gemm(dY, pkT["subj_w"], _new(B, T, D1p, dt, dev), B=B, T=T, KS=1, dil=0, widx=c.widx, alg_dims=(D1, D1),
                         flags=BWD_FLAGS)
    if want["sb_w"]:
        g["sb_w"] = _wgrad(dh_c, c.h_sa, B, T, 1, 0, D1, D1)
    if want["sb_b"]:
        g["sb_b"] = ops.colsum(dh_c, B, T, ops.reduce_scratch(D1p, dev))[:D1]
    if want["z"] or want["X"]:
        dh_sa = ops.conv_gemm(dh_c, pkT["sb_w"], _new(B, T, D1p, dt, dev), B=B, T=T, KS=1, dil=0, alg_dims=(D1, D1),
                              flags=BWD_FLAGS)
        g["X"], g["z"] = sa_backward(sb.spatial_attention, c.sa, dh_sa, want["X"], want["z"])
    return g


# ------------------------------------------------------------------------------------------------------------ ConvBlock
CB_PARAMS = ("c0w", "c0b", "bn0w", "bn0b", "c1w", "c1b", "bn1w", "bn1b", "c2w", "c2b")


def cb_params(cb):
    """The ten parameters of a ConvBlock in CB_PARAMS order."""
    return [cb.conv0.weight, cb.conv0.bias, cb.batchnorm0.weight, cb.batchnorm0.bias, cb.conv1.weight, cb.conv1.bias,
            cb.batchnorm1.weight, cb.batchnorm1.bias, cb.conv2.weight, cb.conv2.bias]


@dataclass
class CBCtx:
    B: int
    T: int
    x: torch.Tensor                     # the input's RL buffer
    x_rows: bool                        # the input was an RL view: its gradient goes back as one
    x_dtype: torch.dtype
    h: list                             # conv0 / conv1 outputs (BatchNorm inputs)
    a: list                             # GELU(BatchNorm) outputs
    bn: list                            # (mean, rstd, training) per BatchNorm
    c2: torch.Tensor                    # conv2 output [value | gate]
    params: list = field(default_factory=list)
    versions: list = field(default_factory=list)


def _cb_plans(cb):
    def build(f, b):
        layers.add_conv_block_packs(f, b, "", [(c.weight, c.bias) for c in (cb.conv0, cb.conv1, cb.conv2)], cb.D2,
                                    L.pad_channels(cb.in_channels))
        return f, b
    return _plans(cb, cb.conv0.weight.device, build)


def _cb_sources(cb) -> Dict[str, torch.Tensor]:
    return {n: p.detach() for n, p in zip(CB_PARAMS, cb_params(cb)) if not n.startswith("bn")}


def conv_block_forward(cb, X: torch.Tensor, need_grad: bool):
    """models.py:152-166: conv0 (+ residual for k > 0) -> BatchNorm -> GELU -> conv1 + residual -> BatchNorm -> GELU -> conv2 ->
    GLU.  A BatchNorm in training mode normalises with the batch statistics over (B, T) and moves its running statistics
    (sda_bn_finalize, num_batches_tracked included); in eval mode it applies the running statistics."""
    B, Cc, T = X.shape
    dt, dev, D2 = cb.compute_dtype, X.device, cb.D2
    D2p = L.pad_channels(D2)
    dil = layers.block_dilations(cb.k)
    x, x_rows = rows_in(X, Cc, dt)
    pk = _cb_plans(cb)[0].run(_cb_sources(cb))
    hs, as_, bns = [], [], []
    inp = x
    for j, bn in ((0, cb.batchnorm0), (1, cb.batchnorm1)):
        if bn.momentum is None:
            raise L.SdaError("ConvBlock: BatchNorm with momentum=None (cumulative average) is not supported")
        res = inp if (j == 1 or cb.k > 0) else None
        h = _new(B, T, D2p, dt, dev)
        alg = (Cc if j == 0 else D2, D2)
        gamma, beta = bn.weight.detach(), bn.bias.detach()
        if bn.training:
            nt = ops.conv_stats_rows(B, T, 3, D2p, FWD_FLAGS)
            stats = torch.empty((nt, 2, D2p), dtype=torch.float32, device=dev)
            ops.conv_gemm(inp, pk[f"c{j}w"], h, B=B, T=T, KS=3, dil=dil[j], bias=pk[f"c{j}b"], res=res, stats=stats, alg_dims=alg,
                          flags=FWD_FLAGS)
            mean, rstd, scale, shift = ops.bn_finalize(stats, nt, float(B) * T, gamma, beta, bn.running_mean, bn.running_var, D2p,
                                                       True, bn.eps, bn.momentum, batches_tracked=bn.num_batches_tracked)
        else:
            ops.conv_gemm(inp, pk[f"c{j}w"], h, B=B, T=T, KS=3, dil=dil[j], bias=pk[f"c{j}b"], res=res, alg_dims=alg, flags=FWD_FLAGS)
            mean, rstd, scale, shift = ops.bn_finalize(None, 0, float(B) * T, gamma, beta, bn.running_mean, bn.running_var, D2p,
                                                       False, bn.eps, bn.momentum)
        a = ops.bn_gelu_forward(h, _new(B, T, D2p, dt, dev), scale, shift, B, T)
        hs.append(h)
        as_.append(a)
        bns.append((mean, rstd, bn.training))
        inp = a
    c2 = ops.conv_gemm(inp, pk["c2w"], _new(B, T, 2 * D2p, dt, dev), B=B, T=T, KS=3, dil=dil[2], bias=pk["c2b"],
                       alg_dims=(D2, 2 * D2), flags=FWD_FLAGS)
    y = ops.glu_forward(c2, _new(B, T, D2p, dt, dev), B, T)
    if not need_grad:
        return y, None
    return y, CBCtx(B, T, x, x_rows, X.dtype, hs, as_, bns, c2)


def conv_block_backward(cb, c: CBCtx, dY: torch.Tensor, want: Dict[str, bool]) -> Dict[str, torch.Tensor]:
    """want: X and the names of CB_PARAMS -> the gradients asked for.  g["X"] is an RL buffer (the caller shapes it)."""
    _check_versions(c)
    B, T, dt, dev, D2 = c.B, c.T, cb.compute_dtype, dY.device, cb.D2
    D2p, cin, cin_p = L.pad_channels(D2), cb.in_channels, L.pad_channels(cb.in_channels)
    dil = layers.block_dilations(cb.k)
    scratch = ops.reduce_scratch(2 * D2p, dev)
    g: Dict[str, torch.Tensor] = {}
    dc2 = _new(B, T, 2 * D2p, dt, dev)
    if want["c2b"]:
        cs = ops.glu_backward_colsum(c.c2, dY, dc2, B, T, scratch)           # [sum d value | sum d gate], D2p apart
        g["c2b"] = ops.bias_grad(cs, 2 * D2, glu_half=D2, glu_half_p=D2p)
    else:
        ops.glu_backward(c.c2, dY, dc2, B, T)
    if want["c2w"]:
        g["c2w"] = _wgrad(dc2, c.a[1], B, T, 3, dil[2], 2 * D2, D2, glu_half=D2, glu_half_p=D2p)
    if not any(want[n] for n in ("X",) + CB_PARAMS[:8]):
        return g
    pkT = _cb_plans(cb)[1].run(_cb_sources(cb))
    da = ops.conv_gemm(dc2, pkT["c2w"], _new(B, T, D2p, dt, dev), B=B, T=T, KS=3, dil=dil[2], alg_dims=(2 * D2, D2), flags=BWD_FLAGS)
    for j, bn in ((1, cb.batchnorm1), (0, cb.batchnorm0)):
        mean, rstd, training = c.bn[j]
        dh = _new(B, T, D2p, dt, dev)
        # eval-mode BatchNorm is a fixed per-channel affine map: an infinite count drops the batch-statistics terms
        dgam, dbet = ops.bn_gelu_backward(da, c.h[j], mean, rstd, bn.weight.detach(), bn.bias.detach(), dh, B, T, scratch,
                                          count=float(B) * T if training else float("inf"))
        if want[f"bn{j}w"]:
            g[f"bn{j}w"] = dgam[:D2]
        if want[f"bn{j}b"]:
            g[f"bn{j}b"] = dbet[:D2]
        if want[f"c{j}b"]:
            # a training-mode BatchNorm removes any per-channel constant: the bias gradient is identically zero
            g[f"c{j}b"] = ops.zeros((D2,), torch.float32, dev) if training else ops.colsum(dh, B, T, scratch)[:D2]
        src, ci = (c.a[0], D2) if j == 1 else (c.x, cin)
        if want[f"c{j}w"]:
            g[f"c{j}w"] = _wgrad(dh, src, B, T, 3, dil[j], D2, ci)
        if j == 1:
            if not any(want[n] for n in ("X",) + CB_PARAMS[:4]):
                return g
            da = ops.conv_gemm(dh, pkT["c1w"], _new(B, T, D2p, dt, dev), B=B, T=T, KS=3, dil=dil[1], res=dh, alg_dims=(D2, D2),
                               flags=BWD_FLAGS)
        elif want["X"]:
            g["X"] = ops.conv_gemm(dh, pkT["c0w"], _new(B, T, cin_p, dt, dev), B=B, T=T, KS=3, dil=dil[0],
                                   res=dh if cb.k > 0 else None, alg_dims=(D2, cin), flags=BWD_FLAGS)
    return g
