"""Host-side facts about the reference's layers that the encoder's step (engine.py), the stand-alone modules (blocks.py) and
the tools must agree on: dilations, the subject-index check, how a weight-gradient launch is cut into sample segments, the
launch chains on top of those segments and the operand-pack entries of a ConvBlock and of the SubjectBlock's two convs.

The segment plans decide slab counts and therefore summation order (result bits).  Callers keep deciding the stream a chain
runs on and how a plan's arrays reach the device; every kernel wrapper is called through `ops` (tests count launches there).
"""
from __future__ import annotations

from typing import NamedTuple

import numpy as np
import torch

from . import lib as L
from . import ops


def block_dilations(k: int):
    """models.py:133,141,149"""
    return 2 ** ((2 * k) % 5), 2 ** ((2 * k + 1) % 5), 2


def subject_indices(subject_idxs, B: int, S: int) -> np.ndarray:
    """subject_idxs (a CPU int tensor in the reference, train.py:189) validated like ModuleList indexing."""
    sidx = torch.as_tensor(subject_idxs).detach().to("cpu").to(torch.int64).numpy()
    if sidx.shape != (B,):
        raise ValueError("subject_idxs must have shape (B,)")
    if (sidx < 0).any() or (sidx >= S).any():
        raise IndexError("subject index out of range")                # ModuleList semantics, models.py:115
    return sidx


# ------------------------------------------------------------------------------------ weight-gradient segment planning
WGRAD_TARGET_WGS = 256      # workgroups per weight-gradient launch, split over sample segments: one per CU, a sharp optimum
                            # (160 +0.37 ms, 512 +0.2)


def wgrad_ntiles(Cout_p: int, Cin_p: int, tile_n: int = 64) -> int:
    """Output tiles of one segment AS THE CALLER'S PLANNING COUNTS THEM: row tiles x (Cin_p / tile_n).  The kernel's own column
    tile is 64 for kernel size 3 and 128 for kernel size 1 (Cin_p % 128 == 0)."""
    return (Cout_p // ops.wgrad_tile_m(Cout_p)) * (Cin_p // tile_n)


def uniform_segment_count(B: int, ntiles: int) -> int:
    """Sample segments of a weight-gradient launch with `ntiles` tiles per segment."""
    # segments are dealt round-robin to the 8 XCDs (wgrad_gemm's block order), so use a multiple of 8
    nseg = 8 * max(1, round(WGRAD_TARGET_WGS / (8 * max(1, ntiles))))
    return int(min(B, nseg)) if B >= 8 else int(max(1, min(B, nseg)))


def uniform_segment_edges(B: int, nseg: int) -> np.ndarray:
    """int32 [nseg + 1] edges of `nseg` nearly equal runs of consecutive samples (no permutation: the kernel then needs no index
    load in its chunk loop)."""
    return np.floor(np.linspace(0, B, nseg + 1)).astype(np.int32)


def subject_slices(B: int, present: int, ntiles: int) -> int:
    """Slices r each subject's samples are cut into for the per-subject weight gradient (`present` subjects in the batch, `ntiles`
    tiles per segment): with many subjects one slice each fills the GPU; with few, r slices keep ~WGRAD_TARGET_WGS workgroups."""
    return int(max(1, min(max(1, B // present), round(WGRAD_TARGET_WGS / max(1, ntiles * present)))))


def subject_segments(sidx: np.ndarray, S: int, r: int):
    """K-segments of the per-subject weight gradient: samples sorted by subject (stable), each subject's run cut
    into `r` nearly equal slices, segments listed slice-major (segment j*S + s = slice j of subject s) so that the
    r slabs of one subject are `r` equally strided blocks for the ordered slab sum.
    Returns (perm int32 [B], seg_start int32 [r*S + 1])."""
    order = np.argsort(sidx, kind="stable").astype(np.int32)
    bounds = np.searchsorted(sidx[order], np.arange(S + 1)).astype(np.int64)
    lo, hi = bounds[:-1], bounds[1:]
    cuts = [lo + ((hi - lo) * j) // r for j in range(r + 1)]              # r + 1 arrays of S cut points
    seg = np.empty(r * S + 1, dtype=np.int32)
    parts, pos = [], 0
    for j in range(r):
        for s in range(S):
            a_, b_ = int(cuts[j][s]), int(cuts[j + 1][s])
            seg[j * S + s] = pos
            parts.append(order[a_:b_])
            pos += b_ - a_
    seg[r * S] = pos
    perm = np.concatenate(parts).astype(np.int32) if parts else order
    return perm, seg


def uniform_nseg(B: int, Cout_p: int, Cin_p: int, tile_n: int = 64) -> int:
    """Segments of consecutive samples (edges: uniform_segment_edges) of the weight-gradient launch of a Cout_p x Cin_p layer.
    The column tile counted is a planning convention (below): 64 for every kernel size; only a tool that sweeps the kernel
    itself passes the kernel's own."""
    return uniform_segment_count(B, wgrad_ntiles(Cout_p, Cin_p, tile_n))


# The column tile a plan COUNTS need not be the one the kernel runs: the count only sizes the launch (segments, slices), and each
# call site keeps the count it was first measured and verified with, because a different count means other slabs, another
# summation order and other result bits.  So uniform plans count 64 columns for kernel size 1 as well (the kernel takes 128
# there), and the per-subject plan has three conventions, (Cout_p, Cin_p, tile_n) each, which happen to differ where D1p is a
# multiple of 128.  Making them agree changes results and is a change of its own.
def subject_tiles_composed(D2p, Cp): return D2p, Cp, 64      # engine, composed SubjectBlock: the k = 3 gradient of (dh0, X)
def subject_tiles_three_conv(D1p): return D1p, D1p, 128 if D1p % 128 == 0 else 64    # engine, three convs: the kernel's own tile
def subject_tiles_blocks(D1p): return D1p, D1p, 64           # blocks.py: the same 1x1 gradient in 64-column tiles


class SubjectPlan(NamedTuple):
    perm: np.ndarray            # int32 [B]: samples sorted by subject, slice-major
    seg_start: np.ndarray       # int32 [r*S + 1]
    r: int                      # slices per subject: the launch has r*S segments, and r slabs per subject to sum


def subject_plan(sidx: np.ndarray, S: int, Cout_p: int, Cin_p: int, tile_n: int) -> SubjectPlan:
    """Per-subject weight gradient of a batch with (validated) subject indices sidx: one K-segment per (slice j, subject s).
    With many subjects one slice each is enough (the S segments already fill the GPU); with few (S = 1 in configs 1/4) every
    subject's samples are cut into r slices so that the launch still has ~WGRAD_TARGET_WGS workgroups."""
    # (sized by the subjects PRESENT in the batch: a batch drawn from a few recordings — 8 of 27 subjects — otherwise
    # runs the launch on a third of its workgroups: +0.3 ms per step, measured with the resident feed in round 5)
    r = subject_slices(sidx.shape[0], max(1, int(np.unique(sidx).size)), wgrad_ntiles(Cout_p, Cin_p, tile_n))
    return SubjectPlan(*subject_segments(sidx, S, r), r)


# ------------------------------------------------------------------------------------------------------- launch chains
# (seg / perm: device arrays of a plan above; the caller picks the stream)
def conv_wgrad(dy, x, B, T, KS, dil, Cout, Cin, seg, nseg, glu_half=0, glu_half_p=0) -> torch.Tensor:
    """Parameter-layout weight gradient (Cout, Cin, KS) fp32 of a conv with output gradient dy and input x (RL buffers)."""
    slabs = ops.wgrad_gemm(dy, x, B=B, T=T, KS=KS, dil=dil, seg_start=seg, nseg=nseg, alg_dims=(Cin, Cout), flat_rows=True)
    return ops.reduce_unpack_wgrad(slabs, Cout, Cin, KS, glu_half=glu_half, glu_half_p=glu_half_p)


def subject_wgrad(dy, h_c, B, T, perm, seg, r, S, D1) -> torch.Tensor:
    """(S, D1, D1, 1) fp32 gradient of the per-subject 1x1 weight (zero for absent subjects) over a SubjectPlan's segments."""
    D1p = dy.shape[1]
    slabs = ops.wgrad_gemm(dy, h_c, B=B, T=T, KS=1, dil=0, perm=perm, seg_start=seg, nseg=r * S, flat_rows=True)
    if r > 1:                   # (r*S, 1, D1p, D1p), slice-major: a subject's r slabs summed in fixed order
        slabs = ops.reduce_slabs(slabs.view(r, -1)).view(S, 1, D1p, D1p)
    return ops.unpack_conv_wgrad(slabs, S, D1, D1, 1, D1p, D1p)


def sa_z_grad(dy, Xt, B, T, seg, nseg, W, mask, cosT, sinT, K, bwd_table) -> torch.Tensor:
    """Gradient of SpatialAttention's z from dy, the gradient of its output, and its input Xt (RL buffers)."""
    dWd = ops.reduce_slabs(ops.wgrad_gemm(dy, Xt, B=B, T=T, KS=1, dil=0, seg_start=seg, nseg=nseg))
    return ops.sa_weights_backward(dWd, W, mask, cosT, sinT, K, bwd_table=bwd_table)


# -------------------------------------------------------------------------------------------------- operand pack plans
def add_conv_block_packs(f, b, prefix: str, convs, D2: int, cin_p: int, glu_tile: int = 0):
    """A ConvBlock's nine entries on a (forward, backward) ops.PackPlan pair, keys prefix + c{j}w / c{j}b.  convs: the three
    (weight, bias) pairs; glu_tile: value + gate channels interleaved per tile for a forward with F.glu in conv2's epilogue."""
    D2p = L.pad_channels(D2)
    glu = dict(glu_half=D2, glu_half_p=D2p)
    for j in (0, 1):
        w, bias = convs[j]
        ci_p = cin_p if j == 0 else D2p
        f.add_weight(f"{prefix}c{j}w", w, D2p, ci_p)
        f.add_vector(f"{prefix}c{j}b", bias, D2p)
        b.add_weight(f"{prefix}c{j}w", w, D2p, ci_p, mode=1)
    w, bias = convs[2]
    f.add_weight(prefix + "c2w", w, 2 * D2p, D2p, glu_tile=glu_tile, **glu)
    f.add_vector(prefix + "c2b", bias, 2 * D2p, glu_tile=glu_tile, **glu)
    b.add_weight(prefix + "c2w", w, 2 * D2p, D2p, mode=1, **glu)


def add_subject_block_packs(f, b, sb_w, sb_b, subj_w, D1p: int):
    """The SubjectBlock's shared and per-subject 1x1 convs on a (forward, backward) ops.PackPlan pair."""
    f.add_weight("sb_w", sb_w, D1p, D1p)
    f.add_vector("sb_b", sb_b, D1p)
    f.add_weight("subj_w", subj_w, D1p, D1p)
    b.add_weight("sb_w", sb_w, D1p, D1p, mode=1)
    b.add_weight("subj_w", subj_w, D1p, D1p, mode=1)
