"""Inputs, float64 references, tolerances and plain-torch fp32 emulations for the tests of csrc/clip_negatives.hip: the CLIP
loss with extra speech negatives that are windows of a resident table (the negatives' logits and the merged column lse, their
coefficient matrix G^n with the shares added to rscale and d loss / d temp, the windowed dZ product), and the float64 autograd
reference of the whole loss.  tests/test_clip_negatives_cpu.py proves on the CPU that the cases reach their edges and catch the
planted bugs; tests/test_clip_negatives_gpu.py holds the HIP kernels to the same check_*() functions.  Nothing here needs a GPU.

The conventions are those of tests/sa_loss_cases.py: exact fp32 inputs, float64 references computed from them, tolerances that
never come from a kernel's output.  Where the arithmetic is a sibling's, its constant is reused: C_LOGIT for the negatives' logits
(clip_rows_kernel's expression), C_LSE for their lse over n, C_D for D_nj = exp(m_nj - col_lse_j) (one of D's two exponentials,
no subtraction).  One quantity is new, the merge of the two lse:

      constant   measured on the CPU   chosen     magnitude it multiplies
      C_MERGE    2.04                  10.0       ulp32(max(|lse|, |a|, |b|, 1))   logaddexp(a, b) = M + log(e^(a - M) + e^(b - M))

measured over every stats case x HW below (every exp moved by -1, 0, +1 ulp) with a = the paired column lse and b = the fp32 lse of
the negatives, against float64 on the same fp32 a and b, and held to 4 .. 5 x measured by
test_clip_negatives_cpu.py::test_tolerance_table_matches_the_emulation.  The shares added to rscale and d loss / d temp are block
sums (sum_tol with block_acc) plus one rounding of the addition: no constant of their own.

The whole pipeline (loss, dZ, dtemp on embeddings and a table) is emulated in fp32 by emul_pipeline, the kernels' own
decomposition, and held to float64 autograd of the two-line form (loss_ref) with the project's fp32 bounds (1e-5 on the
loss and the l2 error of a gradient — here relative to the summed norms of dZ's three terms, which cancel in part —, 1e-4 max(1,
|dtemp|)); its mutants are the planted bugs.
"""
import math

import numpy as np
import torch

from tests.sa_loss_cases import (C_D, C_LOGIT, C_LSE, DTYPES, F32, F64, FTZ, HW, SENT, U32, _exp, _gen, _log, block_acc, exact, host,  # noqa: F401
                                 lse_tol, pad64, q, ratio, sum_tol, ulp, ulp32)
from tests.clip_label_cases import store

I32 = torch.int32
C_MERGE = 10.0
DTYPES16 = (torch.bfloat16, torch.float16)
ROW_PAD = 16
PIPE_LOSS_REL, PIPE_GRAD_REL_L2, PIPE_DTEMP = 1e-5, 1e-5, 1e-4          # the project's fp32 bounds

# (Bn, N): brain columns of the block x negatives — both sides of a 32-row K-step, of the 256-thread stride and of a 256 tile
STATS_SHAPES = ((1, 1), (2, 31), (5, 32), (64, 33), (65, 255), (3, 256), (70, 257), (257, 289))
STATS_REGIMES = ("flat", "trained", "dominant", "negligible", "norms")


def neg_rows(N):
    return (N + 31) // 32 * 32


# ---------------------------------------------------------------------------------------------------------------
# sda_clip_neg_stats / sda_clip_neg_grad: exact fp32 inputs
# ---------------------------------------------------------------------------------------------------------------
def stats_case(Bn, N, regime):
    """Raw scores S[j][n] of N negatives against Bn brain columns, their norms, the temperature and the paired column lse the
    kernel merges into.  dominant: the negatives carry the column soft-max (their lse is ~8 above the paired one); negligible:
    ~30 below (the merge must leave col_lse within an ulp of itself); norms: wsq and zsq span 2^16."""
    g = _gen(6113 * Bn + 17 * N + 1000003 * STATS_REGIMES.index(regime))
    rnd = lambda *s: torch.randn(*s, generator=g, dtype=F64)
    nw, nz = 40.0 * torch.exp(0.3 * rnd(N)), 30.0 * torch.exp(0.3 * rnd(Bn))
    if regime == "norms":
        nw = 40.0 * torch.exp2(torch.linspace(-4.0, 4.0, N, dtype=F64)[torch.randperm(N, generator=g)])
        nz = 30.0 * torch.exp2(torch.linspace(-4.0, 4.0, Bn, dtype=F64)[torch.randperm(Bn, generator=g)])
    temp, spread = {"flat": (0.0, 0.2), "trained": (5.1, 0.004), "dominant": (5.1, 0.004), "negligible": (5.1, 0.004),
                    "norms": (5.1, 0.004)}[regime]
    Cn = (spread * rnd(Bn, N)).clamp(-0.95, 0.95)
    S = torch.full((Bn, pad64(N) + 64), math.nan)                           # pitch > N: the padding is never read
    S[:, :N] = (Cn * nz[:, None] * nw[None, :]).float()
    wsq, zsq = (nw * nw).float(), (nz * nz).float()
    temp32 = torch.tensor([temp], dtype=F32)
    m64 = S[:, :N].double() * torch.exp(temp32.double()) / (torch.sqrt(wsq.double())[None, :] * torch.sqrt(zsq.double())[:, None])
    nl = torch.logsumexp(m64, 1)
    shift = {"dominant": -8.0, "negligible": 30.0}.get(regime, 0.5)
    col_lse = (nl + shift + 0.3 * rnd(Bn)).float()                          # the paired lse handed in, exact fp32
    m32 = m64.float()
    merged32 = torch.logaddexp(col_lse.double(), torch.logsumexp(m32.double(), 1)).float()
    Bg = max(Bn, 2)
    inv = float(torch.tensor(1.0 / (2 * Bg), dtype=F32))
    return dict(name=f"neg Bn={Bn} N={N} {regime}", Bn=Bn, N=N, regime=regime, S=S, wsq=wsq, zsq=zsq, temp=temp32, col_lse=col_lse,
                m64=m64, mlog=m32, col_lse_merged=merged32, inv_norm=inv,
                rscale_in=(0.01 * rnd(Bn)).float(), scalars_in=torch.tensor([1.25, -0.375], dtype=F32))


def merge_tol(res, a, b):
    one = torch.ones_like(res)
    return C_MERGE * ulp32(torch.maximum(torch.maximum(res.abs(), a.abs()), torch.maximum(b.abs(), one)))


def neg_stats_ref(c):
    m = c["m64"]
    tol_m = C_LOGIT * m.abs() + FTZ
    nl, mx = torch.logsumexp(m, 1), m.amax(1)
    tol_nl = tol_m.amax(1) + lse_tol(nl, mx, c["N"])
    a = c["col_lse"].double()
    res = torch.logaddexp(a, nl)
    return dict(m=m, tol_m=tol_m, col_lse=res, tol_col_lse=tol_nl + merge_tol(res, a, nl))


def check_neg_stats(c, mlog_buf, col_lse_buf):
    """mlog_buf: (Bn + 1, N) fp32 and col_lse_buf: (Bn + 1,) fp32 handed in as the paired lse, both with a sentinel last row"""
    r = neg_stats_ref(c)
    Bn = c["Bn"]
    mlog, cl = host(mlog_buf), host(col_lse_buf)
    out = {"mlog": ratio(mlog[:Bn], r["m"], r["tol_m"]), "col_lse merged": ratio(cl[:Bn], r["col_lse"], r["tol_col_lse"]),
           "past the outputs untouched": exact(bool((mlog[Bn:] == SENT).all()) and bool((cl[Bn:] == SENT).all()))}
    if c["regime"] == "negligible":
        a = c["col_lse"].double()
        out["negligible negatives leave col_lse within an ulp"] = ratio(cl[:Bn], a, ulp32(a))
    return out


NONFINITE_MUTANTS = ("merge_with_fmaxf", "saturating_store", "colsum_skips_nonfinite", "window_row_outside_times_zero")


def emul_merge(a, b, hw=0, mutant=None):
    """logaddexp(a, b) as the kernel writes it; torch.maximum hands a NaN on.  mutant merge_with_fmaxf: the hand-written form on
    fmaxf / fminf, M + log(1 + exp(min - M)) — both drop a NaN operand, and a NaN paired lse comes out as the negatives' lse + log 2.
    (fmaxf under the kernel's own two exponentials would still meet the NaN in exp(a - M): the two-sided form is the one that
    swallows.)"""
    if mutant == "merge_with_fmaxf":
        skip = lambda x, other: torch.where(torch.isnan(x), other, x)
        M, m = torch.maximum(skip(a, b), skip(b, a)), torch.minimum(skip(a, b), skip(b, a))
        return M + _log(1.0 + _exp(m - M, hw))
    M = torch.maximum(a, b)
    return M + _log(_exp(a - M, hw) + _exp(b - M, hw))


def emul_neg_stats(c, hw=0, mutant=None):
    N = c["N"]
    m = c["S"][:, :N] * (_exp(c["temp"], hw) / torch.sqrt(c["wsq"]))[None, :] / torch.sqrt(c["zsq"])[:, None]
    mx = m.amax(1)
    nl = mx + _log(_exp(m - mx[:, None], hw).sum(1))
    if mutant == "col_lse_not_merged":
        return m, c["col_lse"].clone()
    if mutant == "merge_replaces_col_lse":
        return m, nl
    return m, emul_merge(c["col_lse"], nl, hw, mutant)


def neg_D(c):
    """float64 D_nj [Bn][N] and the magnitude C_D multiplies, from the fp32 mlog and merged col_lse the grad kernel is handed"""
    m, cl = c["mlog"].double(), c["col_lse_merged"].double()[:, None]
    D = torch.exp(m - cl)
    mag = ulp32(torch.maximum(torch.maximum(m.abs(), cl.abs().expand_as(m)), torch.ones_like(m))) * D + ulp32(D)
    return D, mag


def neg_grad_ref(c, dtype):
    Bn, N, inv = c["Bn"], c["N"], c["inv_norm"]
    m = c["mlog"].double()
    D, mag = neg_D(c)
    tol_D = C_D * mag + FTZ
    wsq, zsq = c["wsq"].double(), c["zsq"].double()
    wmax = math.sqrt(float(wsq.max()))
    f = (wmax / torch.sqrt(wsq))[:, None]                                  # [N][1]
    G = torch.zeros(neg_rows(N), pad64(Bn), dtype=F64)
    G[:N, :Bn] = D.t() * f
    tol_G = torch.ones_like(G)
    tol_G[:N, :Bn] = f * tol_D.t() + 5 * U32 * G[:N, :Bn].abs() + ulp(G[:N, :Bn], dtype)
    dl = (D * m).sum(1)
    tol_dl = sum_tol(D * m, tol_D * m.abs() + U32 * (D * m).abs(), block_acc(N), dim=1)
    share = inv * dl / zsq
    rscale = c["rscale_in"].double() + share
    cscale = inv * float(torch.exp(c["temp"].double())) / (wmax * torch.sqrt(zsq))
    s1 = c["scalars_in"].double()[1] + inv * dl.sum()
    return dict(D=D, G=G, tol_G=tol_G, rscale=rscale, tol_rscale=inv * tol_dl / zsq + 3 * U32 * share.abs() + ulp32(rscale) + FTZ,
                cscale=cscale, tol_cscale=2 * C_LOGIT * cscale, s1=s1,
                tol_s1=(inv * tol_dl + 2 * U32 * (inv * dl).abs()).sum() + ulp32(s1) + ulp32(c["scalars_in"].double()[1]))


def check_neg_grad(c, dtype, G_buf, cscale_n, rscale, scalars):
    """G_buf: (neg_rows(N) + 1, pad64(Bn)) of dtype, last row sentinel; rscale / scalars were handed in as rscale_in / scalars_in"""
    Bn, N = c["Bn"], c["N"]
    r = neg_grad_ref(c, dtype)
    G = host(G_buf).float()
    nr = neg_rows(N)
    pad = torch.ones(nr, G.shape[1], dtype=torch.bool)
    pad[:N, :Bn] = False
    return {"Gn": ratio(G[:nr], r["G"], r["tol_G"]), "Gn rows from N on and pad columns exactly zero": exact((G[:nr][pad] == 0).all()),
            "Gn past its rows untouched": exact((G[nr:] == SENT).all()),
            "cscale_n": ratio(host(cscale_n), r["cscale"], r["tol_cscale"]), "rscale with the share added": ratio(host(rscale), r["rscale"], r["tol_rscale"]),
            "scalars[1] dtemp with the share added": ratio(host(scalars)[1], r["s1"], r["tol_s1"]),
            "scalars[0] loss untouched": exact(float(host(scalars)[0]) == float(c["scalars_in"][0]))}


def emul_neg_grad(c, dtype, hw=0, mutant=None, colpart=False):
    """(G^n with its sentinel row, cscale_n, rscale, scalars); colpart: also the per-column shares the kernel leaves for the
    scalars kernel behind it"""
    Bn, N = c["Bn"], c["N"]
    m, cl, wsq, zsq = c["mlog"], c["col_lse_merged"], c["wsq"], c["zsq"]
    inv = torch.tensor(c["inv_norm"], dtype=F32)
    d = _exp(m - cl[:, None], hw)
    wmax = torch.sqrt(wsq.max())
    scale = wmax / torch.sqrt(wsq)
    if mutant == "gn_wrong_norm":
        scale = wmax / torch.sqrt(torch.roll(wsq, 1))
    nr = neg_rows(N)
    G = torch.full((nr + 1, pad64(Bn)), SENT)
    G[:nr] = 0.0
    G[:N, :Bn] = store(d.t() * scale[:, None], dtype, mutant)
    dm = d * m
    if mutant == "colsum_skips_nonfinite":
        dm = torch.where(torch.isfinite(dm), dm, torch.zeros(()))
    dl = dm.sum(1) * inv
    rscale = c["rscale_in"].clone() if mutant == "rscale_share_missing" else c["rscale_in"] + dl / zsq
    scal = c["scalars_in"].clone()
    if mutant != "dtemp_share_missing":
        scal[1] = (scal[1].double() + dl.double().sum()).float()
    out = G, inv * _exp(c["temp"], hw) / (wmax * torch.sqrt(zsq)), rscale, scal
    return out + (dl,) if colpart else out


def measure_constants(cases):
    """largest error of the merged lse's emulation against float64 on the same fp32 a, b, in units of C_MERGE's magnitude"""
    worst = 0.0
    for c in cases:
        a = c["col_lse"]
        for hw in HW:
            m, _ = emul_neg_stats(c, hw)
            mx = m.amax(1)
            b = mx + _log(_exp(m - mx[:, None], hw).sum(1))
            ref = torch.logaddexp(a.double(), b.double())
            err = (emul_merge(a, b, hw).double() - ref).abs() / (merge_tol(ref, a.double(), b.double()) / C_MERGE)
            worst = max(worst, float(err.max()))
    return dict(C_MERGE=worst)


# ---------------------------------------------------------------------------------------------------------------
# windows of a table
# ---------------------------------------------------------------------------------------------------------------
START_PATTERNS = ("edges", "overlap", "same", "descending")


def starts_of(N, L, T, pattern):
    """N int32 window starts in a table of L rows: a window at row 0 and one ending at the last row (edges, descending: whenever
    N >= 2), windows one row apart (overlap), every start twice (same), descending order."""
    last = L - T
    g = np.random.RandomState(1009 * N + L + 7 * START_PATTERNS.index(pattern))
    if pattern == "edges":
        s = g.randint(0, last + 1, size=N)
        s[0] = 0
        s[-1] = last if N >= 2 else 0
    elif pattern == "overlap":
        s = np.arange(N) % (last + 1)
    elif pattern == "same":
        s = (np.arange(N) // 2 * 3) % (last + 1)
    elif pattern == "descending":
        s = np.sort(g.randint(0, last + 1, size=N))[::-1].copy()
        s[0] = last
        s[-1] = 0 if N >= 2 else last
    else:
        raise KeyError(pattern)
    return s.astype(np.int32)


def windows_of(table, starts, T, shift=0):
    """(N, T * Fp) the windows as the kernels contract over them; `shift` rows early (-) or late (+), clamped into the table"""
    L = table.shape[0]
    rows = (torch.as_tensor(np.asarray(starts), dtype=torch.int64)[:, None] + shift).clamp(0, L - T) + torch.arange(T)[None, :]
    return table[rows].reshape(len(starts), -1)


# ---- sda_clip_dz_windows
# (Bn, N, T, col0-free): K = T * 64 = 256 (one whole tile), 320 (a partial tile), 576 (more than two tiles)
DZ_SHAPES = ((2, 1, 4), (2, 31, 5), (64, 32, 9), (65, 33, 4), (2, 255, 5), (257, 256, 4), (65, 257, 9), (64, 289, 5))
DZ_FP, DZ_TABLE_ROWS = 64, 40


def dz_case(Bn, N, T, pattern, dtype, exact_ints=False):
    """Operands of one sda_clip_dz_windows launch, already of `dtype` precision (held as fp32): the coefficient matrix
    Gn [neg_rows(N)][pad64(Bn)] with zero rows from N on, the table, starts, the per-column factor, out_scale, and the row-layout
    buffer `out` as sda_clip_dz left it (pad rows and slack zero, data non-zero).  exact_ints: small integers and powers of
    two, so that every product and partial sum is exact in fp32 and the result is the exact sum rounded once."""
    g = _gen(811 * Bn + 13 * N + T + 100003 * START_PATTERNS.index(pattern))
    Fp, L = DZ_FP, DZ_TABLE_ROWS
    Tp = T + ROW_PAD
    rows_alloc = Bn * Tp + ROW_PAD + 128 + 2 * ROW_PAD
    Gn = torch.zeros(neg_rows(N), pad64(Bn))
    out = torch.zeros(rows_alloc, Fp)
    data = torch.zeros(rows_alloc, dtype=torch.bool)
    for j in range(Bn):
        data[j * Tp + ROW_PAD:(j + 1) * Tp] = True
    if exact_ints:
        Gn[:N, :Bn] = torch.randint(-3, 4, (N, Bn), generator=g).float()
        table = torch.randint(-15, 16, (L, Fp), generator=g).float()
        cs = torch.exp2(torch.randint(-2, 2, (Bn,), generator=g).float())
        os_ = torch.tensor([0.5])
        out[data] = torch.randint(-8, 9, (int(data.sum()), Fp), generator=g).float()
    else:
        Gn[:N, :Bn] = q(torch.rand(N, Bn, generator=g) * 1.5, dtype)
        table = q(torch.randn(L, Fp, generator=g), dtype)
        cs = torch.rand(Bn, generator=g) * 1e-3 + 1e-4
        os_ = torch.tensor([0.75])
        out[data] = q(0.05 * torch.randn(int(data.sum()), Fp, generator=g), dtype)
    return dict(name=f"dzw Bn={Bn} N={N} T={T} {pattern}", Bn=Bn, N=N, T=T, Fp=Fp, Gn=Gn, table=table, starts=starts_of(N, L, T, pattern),
                cscale=cs, out_scale=os_, out=out, data_rows=data, exact_ints=exact_ints)


def dz_windows_ref(c, dtype, shift=0, n_used=None):
    """float64 result buffer and tolerance: out + out_scale * cscale_j * sum_n Gn[n][j] W_n on the data rows, `out` elsewhere"""
    Bn, N, T, Fp = c["Bn"], c["N"], c["T"], c["Fp"]
    n_used = N if n_used is None else n_used
    W = windows_of(c["table"], c["starts"], T, shift).double()[:n_used]
    G = c["Gn"][:n_used, :Bn].double()
    acc = G.t() @ W                                                          # (Bn, T * Fp)
    absum = G.abs().t() @ W.abs()
    f = (float(c["out_scale"]) * c["cscale"].double())[:, None]
    ref = c["out"].double().clone()
    add = (f * acc).reshape(Bn * T, Fp)
    ref[c["data_rows"]] += add
    tol = torch.ones_like(ref)
    tol[c["data_rows"]] = ((N + 8) * U32 * f.abs() * absum).reshape(Bn * T, Fp) + 4 * U32 * add.abs() + ulp(ref[c["data_rows"]], dtype)
    return ref, tol


def check_dz_windows(c, dtype, out_buf):
    """out_buf: the whole row-layout buffer of dtype after the launch, with one sentinel row appended behind the allocation"""
    ref, tol = dz_windows_ref(c, dtype)
    n = ref.shape[0]
    got = host(out_buf).float()
    data = c["data_rows"]
    res = {"pad rows and slack exactly zero": exact((got[:n][~data] == 0).all()), "past the buffer untouched": exact((got[n:] == SENT).all())}
    if c["exact_ints"]:
        res["data rows equal the exact sum rounded to nearest even"] = exact(torch.equal(got[:n][data], ref[data].to(dtype).float()))
    else:
        res["data rows"] = ratio(got[:n][data], ref[data], tol[data])
    return res


def emul_dz_windows(c, dtype, mutant=None):
    ref, _ = dz_windows_ref(c, dtype, shift={"window_row_early": -1, "window_row_late": 1}.get(mutant, 0),
                            n_used=c["N"] // 32 * 32 if mutant == "last_partial_kstep_dropped" else None)
    if mutant == "window_row_outside_times_zero":
        # the K-steps past N re-read a window against zero coefficients — here not the last candidate's own (whose elements are in
        # the sum anyway) but the one a row later (earlier at the table's end): 0 * table row outside every term of the sum
        s, L, T = int(c["starts"][-1]), c["table"].shape[0], c["T"]
        s = s + 1 if s + 1 + T <= L else s - 1
        ref[c["data_rows"]] += (0.0 * c["table"][s:s + T].double()).repeat(c["Bn"], 1)
    out = torch.full((ref.shape[0] + 1, c["Fp"]), SENT)
    out[:-1] = q(ref.float(), dtype)
    if mutant == "pad_rows_written":
        out[:ROW_PAD] += 1.0
    return out


# ---- sda_sim_gemm_windows (and sda_sim_gemm on the same windows cut out), for tests/nonfinite_cases.py
def sim_case(M, N, T, Fp, dtype):
    """X (M, T * Fp) and a table whose windows start every third row from row 2 on: with T = 4 a row 2 + 3 n + 3 lies in the
    windows of candidates n and n + 1, the two rows in front of it in candidate n's alone, rows 0 and 1 and the last four in none"""
    g = _gen(523 * M + 29 * N + T)
    starts = (2 + 3 * np.arange(N)).astype(np.int32)
    L = int(starts[-1]) + T + 4
    return dict(name=f"sim M={M} N={N} T={T}", M=M, N=N, T=T, Fp=Fp, K=T * Fp, X=q(torch.randn(M, T * Fp, generator=g), dtype),
                table=q(torch.randn(L, Fp, generator=g), dtype), starts=starts)


def sim_windows_ref(c):
    """float64 S[i][n] = <X_i, window n>, (M, N)"""
    return c["X"].double() @ windows_of(c["table"], c["starts"], c["T"]).double().t()


# ---------------------------------------------------------------------------------------------------------------
# the whole loss in float64, and its fp32 emulation in the kernels' decomposition
# ---------------------------------------------------------------------------------------------------------------
def loss_ref(l, m, labels=None, mode="positive", reduction="mean"):
    """The loss of float64 paired logits l (speech rows x brain columns of the whole batch, B x B) and negatives' logits
    m (N x B) in its two-line form: cross-entropy of every speech row over the brain columns, and of every brain column over the
    B + N speech candidates; (sum of both) / 2, each a mean over B for reduction="mean".  With labels: the labelled forms of
    tests/clip_label_cases.loss_ref, in which the negatives carry fresh ids (no positive, never masked)."""
    ce = torch.nn.functional.cross_entropy
    B, N = l.shape[0], m.shape[0]
    tgt = torch.arange(B)
    wide = torch.cat([l, m], 0).t()                                       # brain j over B + N candidates
    if labels is None:
        return (ce(l, tgt, reduction=reduction) + ce(wide, tgt, reduction=reduction)) / 2
    same = labels[:, None] == labels[None, :]
    if mode == "positive":
        Tm = same.double() / same.sum(1, keepdim=True)
        Tw = torch.cat([Tm, torch.zeros(N, B, dtype=F64)], 0).t()
        return (ce(l, Tm, reduction=reduction) + ce(wide, Tw, reduction=reduction)) / 2
    lm = l.masked_fill(same & ~torch.eye(B, dtype=torch.bool), -math.inf)
    return (ce(lm, tgt, reduction=reduction) + ce(torch.cat([lm, m], 0).t(), tgt, reduction=reduction)) / 2


def loss_ref_embeddings(x, y, w, temp, labels=None, mode="positive", reduction="mean", fast=True):
    """float64 autograd on embeddings x (speech), y (brain), (B, F, T), and negatives w (N, F, T) — constants:
    (loss, dx, dy, dtemp, paired logits)"""
    x = x.detach().double().cpu().requires_grad_(True)
    y = y.detach().double().cpu().requires_grad_(True)
    w = w.detach().double().cpu()
    t = torch.tensor([float(temp)], dtype=F64, requires_grad=True)
    B = x.shape[0]
    X, Y = x.reshape(B, -1), y.reshape(B, -1)
    W = w.reshape(w.shape[0], X.shape[1])
    Yn = Y / Y.norm(dim=1, keepdim=True)
    lg = (X / X.norm(dim=1, keepdim=True)) @ Yn.T
    mg = (W / W.norm(dim=1, keepdim=True)) @ Yn.T
    if fast:
        lg, mg = lg * torch.exp(t), mg * torch.exp(t)
    lab = None if labels is None else torch.as_tensor(labels).cpu().to(torch.int64)
    loss = loss_ref(lg, mg, lab, mode, reduction)
    dx, dy, dt = torch.autograd.grad(loss, [x, y, t], allow_unused=True)
    return loss.detach(), dx, dy, (dt if dt is not None else torch.zeros(1, dtype=F64)), lg.detach()


def bank_windows(table, starts, F, T):
    """(N, F, T) the negatives as embeddings: window n is table rows starts[n] ... + T - 1 (row = time step, column = channel)"""
    return windows_of(table, starts, T).reshape(len(starts), T, table.shape[1])[:, :, :F].permute(0, 2, 1).contiguous()


# (B, N, F, T, start pattern): the pipeline's cases on the CPU
PIPE_CASES = ((2, 1, 3, 4, "edges"), (5, 33, 64, 5, "overlap"), (9, 40, 3, 9, "descending"), (7, 65, 3, 4, "same"), (12, 31, 64, 4, "edges"))
PIPE_MUTANTS = ("negatives_in_the_row_softmax", "col_lse_not_merged", "inv_norm_over_B_plus_N", "gn_scaled_by_ymax", "gn_wrong_norm",
                "rscale_share_missing", "dtemp_share_missing", "window_row_early", "window_row_late", "last_partial_kstep_dropped")


def pipe_case(B, N, F, T, pattern, temp=2.5):
    """speech x, brain y (B, F, T) and a table (rows of pad64(F) channels, the padding zero) whose values are bfloat16-exact; the
    table's scale differs from the speech's so that wmax != ymax"""
    g = _gen(401 * B + 7 * N + F + 31 * T)
    Fp, L = pad64(F), max(DZ_TABLE_ROWS, T + 3)
    x = q(torch.randn(B, F, T, generator=g), torch.bfloat16)
    y = q(0.6 * x + torch.randn(B, F, T, generator=g), torch.bfloat16)
    table = torch.zeros(L, Fp)
    table[:, :F] = q(3.0 * torch.randn(L, F, generator=g) * torch.exp(0.5 * torch.randn(L, 1, generator=g)), torch.bfloat16)
    # the first negatives resemble brain rows: some of them matter in the column soft-max
    starts = starts_of(N, L, T, pattern)
    return dict(name=f"pipe B={B} N={N} F={F} T={T} {pattern}", B=B, N=N, F=F, T=T, x=x, y=y, table=table, starts=starts,
                temp=torch.tensor([temp], dtype=F32))


def emul_pipeline(c, mutant=None, reduction="mean"):
    """fp32, in the kernels' decomposition: (loss, dZ (B, F, T), dtemp, the summed l2 norms of dZ's three terms)"""
    B, N, F, T = c["B"], c["N"], c["F"], c["T"]
    Fp = c["table"].shape[1]
    rows = lambda e: torch.nn.functional.pad(e.permute(0, 2, 1), (0, Fp - F)).reshape(e.shape[0], -1)       # (B, T * Fp): time-major rows
    X, Z = rows(c["x"]), rows(c["y"])
    W = windows_of(c["table"], c["starts"], T)
    ysq, zsq, wsq = (X * X).sum(1), (Z * Z).sum(1), (W * W).sum(1)
    alpha = _exp(c["temp"])
    l = (X @ Z.t()) * (alpha / torch.sqrt(ysq))[:, None] / torch.sqrt(zsq)[None, :]
    m = (Z @ W.t()) * (alpha / torch.sqrt(wsq))[None, :] / torch.sqrt(zsq)[:, None]                        # [j][n]
    lse = lambda t, d: t.amax(d) + _log(_exp(t - t.amax(d, keepdim=True)).sum(d))
    rl = lse(l, 1)
    cl = lse(l, 0)
    if mutant != "col_lse_not_merged":
        cl = emul_merge(cl, lse(m, 1))
    inv = 1.0 / (2 * (B + N if mutant == "inv_norm_over_B_plus_N" else B)) if reduction == "mean" else 0.5
    D = _exp(l - rl[:, None]) + _exp(l - cl[None, :]) - 2.0 * torch.eye(B)
    Dn = _exp(m - cl[:, None])
    loss = inv * ((rl - l.diagonal()) + (cl - l.diagonal())).double().sum()
    if mutant == "negatives_in_the_row_softmax":        # a negative treated as a speech row of the batch: a row soft-max of its own
        rn = lse(m, 0)
        Dn = Dn + _exp(m - rn[None, :])
        loss = loss + inv * rn.double().sum()
    dl, dln = (D * l).sum(0) * inv, (Dn * m).sum(1) * inv
    rscale = dl / zsq + (0.0 if mutant == "rscale_share_missing" else dln / zsq)
    dtemp = dl.double().sum() + (0.0 if mutant == "dtemp_share_missing" else dln.double().sum())
    ymax, wmax = torch.sqrt(ysq.max()), torch.sqrt(wsq.max())
    G, cs = D * (ymax / torch.sqrt(ysq))[:, None], inv * alpha / (ymax * torch.sqrt(zsq))
    wn = torch.roll(wsq, 1) if mutant == "gn_wrong_norm" else wsq
    Gn = Dn.t() * ((ymax if mutant == "gn_scaled_by_ymax" else wmax) / torch.sqrt(wn))[:, None]
    csn = inv * alpha / (wmax * torch.sqrt(zsq))
    if mutant == "last_partial_kstep_dropped":
        Gn = Gn.clone()
        Gn[N // 32 * 32:] = 0.0
    Wg = windows_of(c["table"], c["starts"], T, {"window_row_early": -1, "window_row_late": 1}.get(mutant, 0))
    terms = (cs[:, None] * (G.t() @ X), rscale[:, None] * Z, csn[:, None] * (Gn.t() @ Wg))
    dZ = terms[0] - terms[1] + terms[2]
    return loss.float(), dZ.reshape(B, T, Fp)[:, :, :F].permute(0, 2, 1), dtemp.float(), sum(float(t.double().norm()) for t in terms)


def pipeline_figures(c, mutant=None, reduction="mean"):
    """error / bound of the emulation against float64 autograd, per output.  dZ is the sum of three fp32 products that cancel
    in part (at B = 2 almost wholly): its error is bounded relative to the summed norms of the terms, not to what is left of them"""
    loss, dZ, dt, terms = emul_pipeline(c, mutant, reduction)
    w = bank_windows(c["table"], c["starts"], c["F"], c["T"])
    lr, _, dyr, dtr, _ = loss_ref_embeddings(c["x"], c["y"], w, float(c["temp"]), reduction=reduction)
    return {"loss": abs(float(loss) - float(lr)) / (PIPE_LOSS_REL * abs(float(lr))), "dZ": float((dZ.double() - dyr).norm()) / (PIPE_GRAD_REL_L2 * terms),
            "dtemp": abs(float(dt) - float(dtr)) / (PIPE_DTEMP * max(1.0, abs(float(dtr))))}
