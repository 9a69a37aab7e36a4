"""The CLIP loss's launch schedule on row-layout embeddings: one rank's logits block with its soft-max statistics, then
(after the cross-rank merge of the row statistics) the loss share, the gradient coefficient matrix and the rank counts, and
the two embedding gradients.  `loss.py` owns the buffers, the gathers and the autograd node around it.
"""
from __future__ import annotations

from dataclasses import dataclass, replace
from typing import Optional

import torch

from . import lib as L
from . import ops


@dataclass
class ClipCtx:
    Bm: int
    Bn: int
    col0: int
    G: torch.Tensor
    rscale: torch.Tensor
    Yt: torch.Tensor
    Zt: torch.Tensor
    row_elems: int
    dtemp: torch.Tensor
    cscale: Optional[torch.Tensor] = None     # per-column factor taken out of G (see sda_clip_grad): the dZ GEMM's acc_scale
    # what the speech-side gradient (clip_backward_y) needs besides: the block's logits and softmax statistics, the norms
    logits: Optional[torch.Tensor] = None
    row_lse: Optional[torch.Tensor] = None
    col_lse: Optional[torch.Tensor] = None
    ysq: Optional[torch.Tensor] = None
    zsq: Optional[torch.Tensor] = None
    temp: Optional[torch.Tensor] = None
    inv_norm: float = 0.0
    # speech labels of the global batch and their class sizes (None: the unlabelled loss), and what a repeat counts as
    labels: Optional[torch.Tensor] = None
    counts: Optional[torch.Tensor] = None
    duplicates: str = "positive"
    # the pairwise sigmoid loss (sigmoid_forward): its bias and this block's share of d loss / d bias; `logits` then holds the
    # scaled cosines a (the logits less the bias) and there are no lse
    bias: Optional[torch.Tensor] = None
    dbias: Optional[torch.Tensor] = None
    # extra speech negatives read in place from a resident table (None: none): the candidates, their coefficient matrix G^n
    # (sda_clip_neg_grad) and the per-column factor taken out of it — the second pass of clip_backward
    negatives: Optional["ClipNegatives"] = None
    Gn: Optional[torch.Tensor] = None
    cscale_n: Optional[torch.Tensor] = None


@dataclass
class ClipNegatives:
    """N speech negatives that are windows of a resident table of plain rows (every candidate of a retrieval.WindowBank):
    negative n is the T rows from table row starts[n] on.  `lo`, `hi`: the smallest and largest start, from the host copy —
    the span one launch addresses is checked against them before anything runs.  `bank` keeps the table alive."""
    bank: object
    table: torch.Tensor          # (L_total, pad64(F)) of the compute dtype
    starts: torch.Tensor         # int32 [N] on the device
    wsq: torch.Tensor            # fp32 [N] squared norms
    N: int
    lo: int
    hi: int

    @classmethod
    def of(cls, bank) -> "ClipNegatives":
        host = bank.starts_host
        return cls(bank, bank.table, bank.starts, bank.norms_sq, len(bank), int(host.min()), int(host.max()))


def clip_forward(Yt: torch.Tensor, Zt: torch.Tensor, temp: torch.Tensor, *, Bm: int, Bn: int, T: int, col0: int = 0,
                 reduction: str = "mean", B_global: Optional[int] = None, dist_group=None, want_grad: bool = True,
                 ysq: Optional[torch.Tensor] = None, labels: Optional[torch.Tensor] = None, duplicates: str = "positive",
                 negatives: Optional[ClipNegatives] = None):
    """CLIP loss (loss.py:58-79) on RL embeddings: Yt holds the Bm (global) speech rows, Zt the Bn local
    brain rows.  Returns (loss_local_share, logits, ranks_count, ctx).  With `dist_group`, row statistics
    and the diagonal are merged across ranks so that the negatives span the global batch.
    `labels` (device int32 [Bm], one per global sample): samples with one label carry the same speech and are matches of one
    another: extra positives (duplicates="positive") or left out of the soft-max denominators ("mask").  None: the unlabelled
    loss, launch for launch.
    `negatives`: further speech candidates without a brain partner, scored in place against this rank's brain rows; they widen
    the brain -> speech soft-max (the column direction) only.  The caller guarantees that none carries the speech of a sample of
    the global batch and, under data parallelism, that every rank is handed the same ones.  None: today's launches, one for one."""
    st = clip_block_stats(Yt, Zt, temp, Bm=Bm, Bn=Bn, T=T, col0=col0, ysq=ysq, labels=labels, duplicates=duplicates,
                          negatives=negatives)
    if dist_group is None:                       # one process: the block IS the whole matrix, its row lse came with the logits
        row_lse, diag = st.row_lse, st.diag
    else:
        from .distributed import merge_row_softmax_stats
        row_lse, diag = merge_row_softmax_stats(st.row_max, st.row_sum, dist_group, diag=st.diag)   # diag: zero where not owned
    return clip_block_finish(st, row_lse, diag, reduction=reduction, B_global=B_global)


@dataclass
class ClipBlockStats:
    """One rank's column block before the cross-rank merge: logits (Bm, Bn) and what the merge needs."""
    Yt: torch.Tensor
    Zt: torch.Tensor
    temp: torch.Tensor
    Bm: int
    Bn: int
    col0: int
    row_elems: int
    ysq: torch.Tensor
    zsq: torch.Tensor
    logits: torch.Tensor
    row_max: torch.Tensor
    row_sum: torch.Tensor
    col_lse: torch.Tensor
    diag: torch.Tensor
    row_lse: torch.Tensor          # lse of each row over this block's columns only
    labels: Optional[torch.Tensor] = None
    duplicates: str = "positive"
    negatives: Optional[ClipNegatives] = None
    neg_logits: Optional[torch.Tensor] = None      # (Bn, N) fp32, brain-major; col_lse already holds their share


def clip_block_stats(Yt, Zt, temp, *, Bm: int, Bn: int, T: int, col0: int = 0, ysq=None, labels=None,
                     duplicates: str = "positive", negatives: Optional[ClipNegatives] = None) -> ClipBlockStats:
    """First half of clip_forward: norms, the (Bm x Bn) logits block of this rank's brain columns, per-row (max, sum exp)
    over the block, per-column lse over all rows, the positives' logits.  Rank-local: no collective.  With labels and
    duplicates="mask" the statistics leave out the repeats of a sample's own speech; "positive" keeps the unlabelled ones."""
    if labels is not None:
        ops.clip_dup_code(duplicates)             # refused before the first launch
    Fp = Zt.shape[1]
    row_elems = L.rows_tp(T) * Fp
    if ysq is None:                              # (under DP the caller gathers the per-rank norms instead)
        ysq = ops.rows_sumsq(Yt, Bm, row_elems, row_elems)
    zsq = ops.ROW_NORMS.get(Zt, Bn)              # left by the encoder's last conv when Zt is its output buffer
    if zsq is None:
        zsq = ops.rows_sumsq(Zt, Bn, row_elems, row_elems)
    S = ops.matmul_nt_splitk(Yt, Zt, Bm, Bn, row_elems, row_elems)
    if labels is not None and duplicates == "mask":
        logits, row_max, row_sum, col_lse, diag, row_lse = ops.clip_logits_stats_masked(S, ysq, zsq, temp, labels, Bm, Bn, col0)
    else:
        logits, row_max, row_sum, col_lse, diag, row_lse = ops.clip_logits_stats(S, ysq, zsq, temp, Bm, Bn, col0)
    neg_logits = None
    if negatives is not None:
        # the negatives' raw scores against this block's brain rows (their data rows: the windowed GEMM's X with the sample
        # pitch), then their logits and their share of the column lse (the masked one in mask mode).  Rank-local: no collective
        ng, K = negatives, T * Fp
        Sn = torch.empty((Bn, L.pad_channels(ng.N)), dtype=torch.float32, device=Zt.device)
        ks = L.load().sda_sim_gemm_ksplit(Bn, ng.N, K, ops.dt_code(Zt.dtype))
        partial = torch.empty(ks * Sn.numel() if ks > 1 else 0, dtype=torch.float32, device=Zt.device)
        ops.sim_gemm_windows_into(Zt.reshape(-1)[L.ROW_PAD * Fp:], row_elems, ng.table.reshape(-1), ng.starts, ng.lo, ng.hi, Fp,
                                  Bn, ng.N, K, ks, partial, Sn)
        neg_logits = ops.clip_neg_stats(Sn, ng.wsq, zsq, temp, col_lse, Bn, ng.N)
    return ClipBlockStats(Yt, Zt, temp, Bm, Bn, col0, row_elems, ysq, zsq, logits, row_max, row_sum, col_lse, diag, row_lse,
                          labels, duplicates, negatives, neg_logits)


def clip_block_finish(st: ClipBlockStats, row_lse, diag, *, reduction: str = "mean", B_global: Optional[int] = None,
                      labels: Optional[torch.Tensor] = None, duplicates: Optional[str] = None):
    """Second half, given the row lse over the columns of ALL ranks and the positives' logits (after the merge): this rank's
    share of the loss and of d loss / d temp, the gradient coefficient matrix, the retrieval rank counts.  `labels` /
    `duplicates`: default to those the statistics were taken with (they must be the same in mask mode)."""
    if labels is not None or duplicates is not None:
        st = replace(st, labels=st.labels if labels is None else labels, duplicates=duplicates or st.duplicates)
    Yt, Zt, temp, Bm, Bn, col0, row_elems = st.Yt, st.Zt, st.temp, st.Bm, st.Bn, st.col0, st.row_elems
    logits, col_lse, ysq, zsq = st.logits, st.col_lse, st.ysq, st.zsq
    Bg = B_global if B_global is not None else Bm
    inv_norm = 1.0 / (2.0 * Bg) if reduction == "mean" else 0.5
    # G is an MFMA operand (16-bit in the 16-bit modes): it holds the O(1) part of dL/dlogits * exp(temp) / (|Y||Z|), the
    # rest — 1e-8 at the 8-GPU shapes, far outside fp16 — comes back as a per-column fp32 factor in the dZ GEMM's epilogue
    labels, counts = st.labels, None
    if labels is None:
        G, rscale, cscale, scalars = ops.clip_grad(logits, row_lse, col_lse, ysq, zsq, temp, inv_norm, col0, Yt.dtype)
        cnt = ops.clip_ranks(logits, diag, col0)
    else:
        counts = ops.clip_label_counts(labels)     # the one extra launch; the others replace their siblings one for one
        G, rscale, cscale, scalars = ops.clip_grad_labels(logits, row_lse, col_lse, ysq, zsq, temp, labels, counts, st.duplicates,
                                                          inv_norm, col0, Yt.dtype)
        cnt = ops.clip_ranks_labels(logits, diag, labels, col0)
    Gn = cscale_n = None
    if st.negatives is not None:                   # behind clip_grad: it adds the negatives' shares to rscale and d loss / d temp
        Gn, cscale_n = ops.clip_neg_grad(st.neg_logits, col_lse, st.negatives.wsq, zsq, temp, inv_norm, rscale, scalars, Yt.dtype)
    ctx = ClipCtx(Bm=Bm, Bn=Bn, col0=col0, G=G, rscale=rscale, Yt=Yt, Zt=Zt, row_elems=row_elems, dtemp=scalars[1:2],
                  cscale=cscale, logits=logits, row_lse=row_lse, col_lse=col_lse, ysq=ysq, zsq=zsq, temp=temp, inv_norm=inv_norm,
                  labels=labels, counts=counts, duplicates=st.duplicates, negatives=st.negatives, Gn=Gn, cscale_n=cscale_n)
    return scalars[0:1], logits, cnt, ctx


def clip_backward(ctx: ClipCtx, dZt: torch.Tensor, dloss: Optional[torch.Tensor] = None) -> torch.Tensor:
    """dZ = dloss * (diag(c) G^T Y - diag(r) Z)  (gradient of the loss share w.r.t. the local brain embeddings); with negatives
    a second pass adds dloss * diag(c^n) G^n^T W, contracted over their windows in place (r already holds their share)."""
    ops.clip_dz(ctx.G, ctx.Yt, ctx.Zt, dZt, ctx.rscale, ctx.cscale, Bm=ctx.Bm, Bn=ctx.Bn, row_elems=ctx.row_elems, out_scale=dloss)
    ng = ctx.negatives
    if ng is not None:
        T = ctx.row_elems // ctx.Zt.shape[1] - L.ROW_PAD
        ops.clip_dz_windows(ctx.Gn, ng.table, ng.starts, ng.lo, ng.hi, dZt, ctx.cscale_n, N=ng.N, Bn=ctx.Bn, T=T, out_scale=dloss)
    return dZt


def clip_grad_y_coeffs(ctx: ClipCtx, zsq_all: torch.Tensor, dtype, **layout):
    """(Gy, part) of the block behind `ctx`: the labelled twin when the forward had labels, the sigmoid loss's twin behind
    sigmoid_forward."""
    if ctx.bias is not None:
        return ops.sigmoid_grad_y(ctx.logits, ctx.bias, ctx.zsq, zsq_all, ctx.col0, dtype, ctx.labels, ctx.duplicates, **layout)
    if ctx.labels is None:
        return ops.clip_grad_y(ctx.logits, ctx.row_lse, ctx.col_lse, ctx.zsq, zsq_all, ctx.col0, dtype, **layout)
    return ops.clip_grad_y_labels(ctx.logits, ctx.row_lse, ctx.col_lse, ctx.zsq, zsq_all, ctx.labels, ctx.counts, ctx.duplicates,
                                  ctx.col0, dtype, **layout)


def clip_backward_y(ctx: ClipCtx, dYt: torch.Tensor, dloss: Optional[torch.Tensor] = None, labels: Optional[torch.Tensor] = None,
                    duplicates: Optional[str] = None) -> torch.Tensor:
    """dY = dloss * (diag(c_y) Gy^T Z - diag(r_y) Y) on one GPU (the block is the whole matrix): the dZ product with the roles of
    the two embeddings exchanged, on the same GEMM family (no new GEMM kernel).  `labels` / `duplicates`: default to the
    forward's, which `ctx` carries with their class sizes."""
    if labels is not None and labels is not ctx.labels:
        ctx = replace(ctx, labels=labels, counts=None if ctx.bias is not None else ops.clip_label_counts(labels))
    if duplicates is not None:
        ctx = replace(ctx, duplicates=duplicates)
    Gy, part = clip_grad_y_coeffs(ctx, ctx.zsq, ctx.Zt.dtype)
    rscale_y, cscale_y = ops.clip_grad_y_finish(part, ctx.ysq, ctx.zsq, ctx.temp, ctx.inv_norm, 0, ctx.Bm)
    return ops.clip_dz(Gy, ctx.Zt, ctx.Yt, dYt, rscale_y, cscale_y, Bm=ctx.Bn, Bn=ctx.Bm, row_elems=ctx.row_elems, out_scale=dloss)


def sigmoid_forward(Yt: torch.Tensor, Zt: torch.Tensor, temp: torch.Tensor, bias: torch.Tensor, *, Bm: int, Bn: int, T: int,
                    col0: int = 0, reduction: str = "mean", B_global: Optional[int] = None, ysq: Optional[torch.Tensor] = None,
                    labels: Optional[torch.Tensor] = None, duplicates: str = "positive"):
    """The pairwise sigmoid loss on RL embeddings: Yt holds the Bm (global) speech rows, Zt the Bn local brain rows from global
    sample col0.  Every pair is its own binary decision, so the block is complete on its own: there is no merge across ranks
    and the loss is the sum of the blocks' shares.  Returns (loss_local_share, a, ranks_count, ctx) — a = the scaled cosines,
    the logits less the bias; ctx serves clip_backward and clip_backward_y as the CLIP loss's does.
    The tail is three launches (pairs, finish, ranks) against the CLIP loss's five."""
    ops.clip_dup_code(duplicates)                 # refused before the first launch
    Fp = Zt.shape[1]
    row_elems = L.rows_tp(T) * Fp
    if ysq is None:
        ysq = ops.rows_sumsq(Yt, Bm, row_elems, row_elems)
    zsq = ops.ROW_NORMS.get(Zt, Bn)
    if zsq is None:
        zsq = ops.rows_sumsq(Zt, Bn, row_elems, row_elems)
    S = ops.matmul_nt_splitk(Yt, Zt, Bm, Bn, row_elems, row_elems)
    Bg = B_global if B_global is not None else Bm
    inv_norm = 1.0 / Bg if reduction == "mean" else 1.0
    a, diag, G, part = ops.sigmoid_pairs(S, ysq, zsq, temp, bias, Bm, Bn, col0, Yt.dtype, labels, duplicates)
    rscale, cscale, scalars = ops.sigmoid_finish(part, ysq, zsq, temp, inv_norm)
    # the bias moves every entry of a row alike: the order within a row, and so the ranks, are those of a
    cnt = ops.clip_ranks(a, diag, col0) if labels is None else ops.clip_ranks_labels(a, diag, labels, col0)
    ctx = ClipCtx(Bm=Bm, Bn=Bn, col0=col0, G=G, rscale=rscale, Yt=Yt, Zt=Zt, row_elems=row_elems, dtemp=scalars[1:2], cscale=cscale,
                  logits=a, ysq=ysq, zsq=zsq, temp=temp, inv_norm=inv_norm, labels=labels, duplicates=duplicates, bias=bias,
                  dbias=scalars[2:3])
    return scalars[0:1], a, cnt, ctx
