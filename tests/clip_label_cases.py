"""Inputs, float64 references, tolerances and plain-torch fp32 emulations for the kernel-level tests of csrc/clip_labels.hip: the
CLIP loss tail with speech labels (the class sizes, the masked soft-max statistics, the labelled coefficient matrices G and Gy with
the loss scalars, the label-aware ranks), and the float64 autograd reference of the whole labelled loss.
tests/test_clip_labels_cpu.py proves on the CPU that the cases reach their edges and catch the planted bugs;
tests/test_clip_labels_gpu.py holds the HIP kernels to the same check_*() functions.  Nothing here needs a GPU.

The blocks, regimes, Gy layouts and the conventions (exact fp32 inputs, float64 references computed from them, tolerances that
never come from a kernel's output) are those of tests/sa_loss_cases.py; a labelled case is one of its cases plus one int32 label
per global sample.  Where a kernel's arithmetic is its unlabelled sibling's, the sibling's constant is reused (C_LOGIT for the
logits, C_D for D: the labelled D is the same two exponentials and one subtraction).  Two quantities are new:

      constant   measured on the CPU   chosen     magnitude it multiplies
      C_MLSE     2.09                  8.5        ulp32(max(|lse|, |max|, 1))      masked max + log masked sum (+ block_acc u)
      C_PBAR     5.57 u                25 u       sum_same |l| / n                 pbar_j = (sum_i same_ij l_ij) / n_j
                                                                                   (+ block_acc u of the same magnitude, + ulp32(pbar))

measured like sa_loss_cases.measure_constants (every exp moved by -1, 0, +1 ulp) over every shape x pattern x regime below, and
held to 4 .. 5 x measured by test_clip_labels_cpu.py::test_tolerance_table_matches_the_emulation.  The positive mode's D takes
2 / n_j out of a same-label entry instead of 2: the quotient is one more rounding, u (2 / n) and as much to spare.
"""
import math

import numpy as np
import torch

from tests.sa_loss_cases import (C_D, C_LOGIT, C_LSE, CLIP_REGIMES, DTYPES, F32, F64, FTZ, GY_LAYOUT, HW, SENT, U32, _exp, _log,  # noqa: F401
                                 block_acc, clip_case, dot_tol, exact, gy_layout, gy_rows, host, pad64, q, ratio, sum_tol,
                                 tied_entries_equal, ulp, ulp32)

I32 = torch.int32
MODES = ("positive", "mask")
C_MLSE = 8.5
C_PBAR = 25.0 * U32
LOSS_ABS_FLOOR = 1e-6        # |loss| of the all-one-class mask case is 0: the whole-loss tests compare it absolutely, at a few
                             # fp32 ulps of the lse terms that cancel in it (lse ~ 10 at the tested temperatures: ulp 1e-6)

# (Bm, Bn, col0): the smallest blocks that cross each edge — one wave, one full 64 tile, both sides of the 256-thread stride and a
# second pass of it, column blocks with col0 != 0 and their segmented Gy layouts (GY_LAYOUT)
LABEL_SHAPES = ((3, 3, 0), (64, 64, 0), (255, 255, 0), (257, 257, 0), (300, 300, 0), (15, 5, 10), (140, 70, 70), (513, 70, 140))
LABEL_PATTERNS = ("distinct", "pair", "straddle3", "partners_outside", "sizes", "one_class", "extremes")


def labels_of(Bm, Bn, col0, pattern):
    """int32 [Bm] speech labels of the global batch.
    pair              the first and the last sample of the block: in the `ties` regime these two brain columns are identical, so
                      the repeat's logit equals the positive's exactly
    straddle3         a class of three around the block's edges: the sample before col0 (or the first), one inside, the one at
                      col0 + Bn (or the last)
    partners_outside  a class with one member inside the block whose partners all lie outside it (on a block that is the whole
                      matrix: samples 1 and Bm - 1, the `ties` regime's two identical speech rows)
    sizes             one class of half the batch, one of two, singletons
    extremes          ids at both ends of int32, with a pair at each end"""
    lab = torch.arange(Bm, dtype=torch.int64) + 1000
    g = torch.Generator().manual_seed(17 * Bm + Bn + col0)
    lo, hi = col0, col0 + Bn - 1
    if pattern == "distinct":
        pass
    elif pattern == "pair":
        lab[hi] = lab[lo]
    elif pattern == "straddle3":
        members = (max(col0 - 1, 0), col0 + Bn // 2, min(col0 + Bn, Bm - 1))
        for m in members:
            lab[m] = 7
    elif pattern == "partners_outside":
        if Bm > Bn:
            outside = [i for i in range(Bm) if i < lo or i > hi]
            for m in (col0 + Bn // 2, outside[0], outside[-1]):
                lab[m] = 7
        else:
            lab[Bm - 1] = lab[1]
    elif pattern == "sizes":
        perm = torch.randperm(Bm, generator=g)
        lab[perm[: max(Bm // 2, 2)]] = 7
        lab[perm[max(Bm // 2, 2): max(Bm // 2, 2) + 2]] = 8
    elif pattern == "one_class":
        lab[:] = 7
    elif pattern == "extremes":
        half = Bm // 2
        lab[:half] = -2 ** 31 + torch.arange(half)
        lab[half:] = 2 ** 31 - 1 - torch.arange(Bm - half)
        if half >= 2:
            lab[1] = lab[0]                      # a pair at -2^31
        if Bm - half >= 2:
            lab[half + 1] = lab[half]            # a pair at 2^31 - 1
    else:
        raise KeyError(pattern)
    return lab.to(I32)


def label_case(Bm, Bn, col0, regime, pattern, base=None):
    """sa_loss_cases.clip_case plus labels: the class sizes, the same-label matrix of the block, and the masked soft-max
    statistics of the GLOBAL problem as the rounded float64 results a labelled kernel is handed in mask mode"""
    c = dict(base if base is not None else clip_case(Bm, Bn, col0, regime))
    lab = labels_of(Bm, Bn, col0, pattern)
    same_g = lab[:, None] == lab[None, :]
    c.update(name=f"{c['name']} labels={pattern}", pattern=pattern, labels=lab, counts=same_g.sum(1).to(I32), same_g=same_g,
             same=same_g[:, col0:col0 + Bn], pos=torch.arange(Bm)[:, None] == (col0 + torch.arange(Bn))[None, :])
    keep_g = ~same_g | torch.eye(Bm, dtype=torch.bool)
    Lm = torch.where(keep_g, c["Lg32"].double(), torch.full((), -math.inf, dtype=F64))
    c["row_lse_m"] = torch.logsumexp(Lm, 1).float()
    c["col_lse_m"] = torch.logsumexp(Lm, 0).float()[col0:col0 + Bn].clone()
    return c


def block_of(c, b0):
    """another column block [b0, b0 + Bn) of the same global problem and labels (what another rank holds)"""
    Bm, Bn = c["Bm"], c["Bn"]
    cols = slice(b0, b0 + Bn)
    keep_g = ~c["same_g"] | torch.eye(Bm, dtype=torch.bool)
    Lm = torch.where(keep_g, c["Lg32"].double(), torch.full((), -math.inf, dtype=F64))
    ii = torch.arange(Bm)
    d = dict(c, col0=b0, logits=c["Lg32"][:, cols].contiguous(), col_lse=c["col_lse_all"][cols].clone(), zsq=c["zsq_all"][cols].clone(),
             same=c["same_g"][:, cols], pos=ii[:, None] == (b0 + torch.arange(Bn))[None, :], col_lse_m=torch.logsumexp(Lm, 0).float()[cols].clone())
    d["inb"] = (ii >= b0) & (ii < b0 + Bn)
    return d


def lse_inputs(c, mode):
    """the fp32 (row_lse, col_lse) the grad kernels are handed in this mode"""
    return (c["row_lse_m"], c["col_lse_m"]) if mode == "mask" else (c["row_lse"], c["col_lse"])


# ---- sda_clip_label_counts
def emul_counts(c, mutant=None):
    lab = c["labels"]
    if mutant == "counts_over_the_block":
        lab_cmp = lab[c["col0"]:c["col0"] + c["Bn"]]
        return (lab[:, None] == lab_cmp[None, :]).sum(1).to(I32)
    return (lab[:, None] == lab[None, :]).float().sum(1).add(0.5).to(I32)


# ---- sda_clip_logits_stats_masked
def keep_of(c):
    """entries of the block that stay in the soft-max denominators: another label, or the positive itself"""
    return ~c["same"] | c["pos"]


def mlse_tol(lse, mx, n):
    return C_MLSE * ulp32(torch.maximum(torch.maximum(lse.abs(), mx.abs()), torch.ones_like(lse))) + block_acc(n) * U32


def masked_stats_ref(c):
    """float64 from the exact logits l64: the unmasked logits and diag, the masked row (max, sum, lse) and column lse; rows whose
    every local column is a repeat have max = lse = -inf and sum = 0 exactly"""
    from tests.sa_loss_cases import C_SM
    l, keep = c["l64"], keep_of(c)
    tol_l = C_LOGIT * l.abs() + FTZ
    ninf = torch.full((), -math.inf, dtype=F64)
    lm = torch.where(keep, l, ninf)
    empty = ~keep.any(1)
    mx = lm.amax(1)
    tmx = torch.where(keep, tol_l, torch.zeros((), dtype=F64)).amax(1)
    sh = torch.where(empty, torch.zeros_like(mx), mx)[:, None]
    e = torch.where(keep, torch.exp(l - sh), torch.zeros((), dtype=F64))
    rs = e.sum(1)
    tol_rs = (e * (2 * tmx[:, None] + C_SM * (l - sh).abs().clamp(min=1.0))).sum(1) + block_acc(c["Bn"]) * U32 * rs
    rl, cl = torch.logsumexp(lm, 1), torch.logsumexp(lm, 0)
    ii = torch.arange(c["Bm"])
    jj = (ii - c["col0"]).clamp(0, c["Bn"] - 1)
    fin = lambda t: torch.where(empty, torch.zeros_like(t), t)
    return dict(l=l, tol_l=tol_l, empty=empty, row_max=mx, tol_row_max=tmx, row_sum=rs, tol_row_sum=tol_rs, row_lse=rl,
                tol_row_lse=tmx + mlse_tol(fin(rl), fin(mx), c["Bn"]), col_lse=cl,
                tol_col_lse=torch.where(keep, tol_l, torch.zeros((), dtype=F64)).amax(0) + mlse_tol(cl, lm.amax(0), c["Bm"]),
                diag=torch.where(c["inb"], l[ii, jj], torch.zeros(c["Bm"], dtype=F64)), tol_diag=tol_l[ii, jj])


def check_masked_stats(c, logits, row_max, row_sum, col_lse, diag, row_lse):
    r = masked_stats_ref(c)
    logits, row_max, row_sum, col_lse, diag, row_lse = map(host, (logits, row_max, row_sum, col_lse, diag, row_lse))
    inb, emp = c["inb"], r["empty"]
    ok = ~emp
    out = {"logits (unmasked)": ratio(logits, r["l"], r["tol_l"]), "row_max": ratio(row_max[ok], r["row_max"][ok], r["tol_row_max"][ok]),
           "row_sum": ratio(row_sum[ok], r["row_sum"][ok], r["tol_row_sum"][ok]),
           "row_lse": ratio(row_lse[ok], r["row_lse"][ok], r["tol_row_lse"][ok]),
           "row_max + log row_sum": ratio((row_max.double() + torch.log(row_sum.double()))[ok], r["row_lse"][ok], r["tol_row_lse"][ok]),
           "col_lse": ratio(col_lse, r["col_lse"], r["tol_col_lse"]), "diag": ratio(diag[inb], r["diag"][inb], r["tol_diag"][inb]),
           "diag exactly zero outside the block": exact((diag[~inb] == 0).all()),
           "rows without a kept column: max = lse = -inf, sum = 0": exact((row_max[emp] == -math.inf).all() and (row_sum[emp] == 0).all()
                                                                          and (row_lse[emp] == -math.inf).all())}
    return out


def emul_masked_lse(x, keep, dim, hw=0, mutant=None):
    """(max, sum exp(x - max), lse) along dim over the kept entries, fp32; nothing kept: (-inf, 0, -inf).  Every mask is a select:
    an entry that is left out reaches nothing, whatever it holds.  mutant lse_max_skips_nan: the maximum is fmaxf's, which drops a
    NaN operand (the sum still meets it: what the mutant loses is the row's maximum, which the cross-rank merge consumes)"""
    ninf = torch.full((), -math.inf)
    xm = torch.where(keep, x, ninf)
    if mutant == "lse_max_skips_nan":
        xm = torch.where(torch.isnan(xm), ninf, xm)
    mx = xm.amax(dim)
    # nothing kept: no term is added, whatever the shift.  (Decided by the mask, not by the maximum's value: a row whose kept
    # logits are all -inf has exp(-inf - -inf) = NaN in its sum, on the device and in float64 alike.)
    sh = torch.where(keep.any(dim), mx, torch.zeros_like(mx)).unsqueeze(dim)
    s = torch.where(keep, _exp(x - sh, hw), torch.zeros(())).sum(dim)
    return mx, s, mx + _log(s)


def emul_masked_stats(c, hw=0, mutant=None):
    Bm, Bn, col0 = c["Bm"], c["Bn"], c["col0"]
    ri = _exp(c["temp"], hw) / torch.sqrt(c["ysq"])
    l = c["S"][:, :Bn] * ri[:, None] / torch.sqrt(c["zsq"])[None, :]
    keep = keep_of(c)
    if mutant == "mask_on_the_diagonal_too":
        keep = ~c["same"]
    if mutant == "labels_without_col0":
        keep = ~(c["labels"][:, None] == c["labels"][None, :Bn]) | c["pos"]
    mx, s, rl = emul_masked_lse(l, keep, 1, hw, mutant)
    cl = emul_masked_lse(l, torch.ones_like(keep) if mutant == "mask_rows_not_columns" else keep, 0, hw, mutant)[2]
    ii = torch.arange(Bm)
    diag = torch.where(c["inb"], l[ii, (ii - col0).clamp(0, Bn - 1)], torch.zeros(Bm))
    return l, mx, s, cl, diag, rl


# ---- D, sda_clip_grad_labels
def label_D(c, mode, logits=None, row_lse=None, col_lse=None):
    """float64 D of the block and the magnitude C_D multiplies, from the fp32 logits, row_lse, col_lse the kernels are handed"""
    rl0, cl0 = lse_inputs(c, mode)
    l = (c["logits"] if logits is None else logits).double()
    rl = (rl0 if row_lse is None else row_lse).double()[:, None]
    cl = (cl0 if col_lse is None else col_lse).double()[None, :]
    pr, pc = torch.exp(l - rl), torch.exp(l - cl)
    same, pos = c["same"], c["pos"]
    n = c["counts"].double()[c["col0"]:c["col0"] + c["Bn"]][None, :]
    if mode == "positive":
        T2 = torch.where(same, 2.0 / n, torch.zeros((), dtype=F64)).expand_as(l)
        D = pr + pc - T2
        extra = 2 * U32 * T2                     # the quotient 2 / n: one rounding and one to spare
    else:
        D = torch.where(same & ~pos, torch.zeros((), dtype=F64), pr + pc - 2.0 * pos.double())
        extra = torch.zeros_like(l)
    one = torch.ones_like(l)
    mag = ulp32(torch.maximum(torch.maximum(l.abs(), rl.abs().expand_as(l)), one)) * pr + \
        ulp32(torch.maximum(torch.maximum(l.abs(), cl.abs().expand_as(l)), one)) * pc + ulp32(D)
    if mode == "mask":
        mag = torch.where(same & ~pos, torch.zeros((), dtype=F64), mag)
    return D, mag, extra


def pbar_ref(c):
    """float64 pbar_j, its tolerance, from the fp32 logits"""
    l = c["logits"].double()
    n = c["counts"].double()[c["col0"]:c["col0"] + c["Bn"]]
    ls = torch.where(c["same"], l, torch.zeros((), dtype=F64))
    pbar = ls.sum(0) / n
    mag = ls.abs().sum(0) / n
    return pbar, (C_PBAR + block_acc(c["Bm"]) * U32) * mag + ulp32(pbar), mag


def grad_labels_ref(c, mode, dtype):
    Bm, Bn, col0, inv = c["Bm"], c["Bn"], c["col0"], c["inv_norm"]
    l = c["logits"].double()
    D, mag, extra = label_D(c, mode)
    tol_D = C_D * mag + extra + FTZ
    ysq, zsq = c["ysq"].double(), c["zsq"].double()
    ymax = math.sqrt(float(ysq.max()))
    f = (ymax / torch.sqrt(ysq))[:, None]
    G = torch.zeros(Bm + 1, pad64(Bn), dtype=F64)
    drop, zero = dropped(c, mode), torch.zeros((), dtype=F64)          # (selected out, never 0 * l or 0 * f)
    G[:Bm, :Bn] = torch.where(drop, zero, D * f)
    tol_G = torch.ones_like(G)
    tol_G[:Bm, :Bn] = f * tol_D + 5 * U32 * G[:Bm, :Bn].abs() + ulp(G[:Bm, :Bn], dtype)
    Dl = torch.where(drop, zero, D * l)
    dl = Dl.sum(0)
    tol_dl = sum_tol(Dl, tol_D * l.abs() + U32 * Dl.abs(), block_acc(Bm), dim=0)
    rscale = inv * dl / zsq
    alpha = float(torch.exp(c["temp"].double()))
    cscale = inv * alpha / (ymax * torch.sqrt(zsq))
    jj = torch.arange(Bn)
    rl_in, cl_in = lse_inputs(c, mode)
    rl, cl = rl_in.double()[col0 + jj], cl_in.double()
    if mode == "positive":
        pb, tol_pb, _ = pbar_ref(c)
    else:
        pb, tol_pb = l[col0 + jj, jj], torch.zeros(Bn, dtype=F64)
    cp0 = (rl - pb) + (cl - pb)
    tol_cp0 = U32 * ((rl - pb).abs() + (cl - pb).abs() + cp0.abs()) + 2 * tol_pb
    s0, s1 = inv * cp0.sum(), inv * dl.sum()
    return dict(D=D, G=G, tol_G=tol_G, rscale=rscale, tol_rscale=inv * tol_dl / zsq + 3 * U32 * rscale.abs() + FTZ,
                cscale=cscale, tol_cscale=2 * C_LOGIT * cscale, scalars=torch.stack([s0, s1]),
                tol_scalars=torch.stack([inv * tol_cp0.sum() + ulp32(s0), (inv * tol_dl + 2 * U32 * (inv * dl).abs()).sum() + ulp32(s1)]))


def masked_entries_zero(c, mode, M):
    """mask mode: the coefficient of a repeat is exactly zero (M: [speech row][brain column])"""
    if mode != "mask":
        return 0.0
    return exact((M[c["same"] & ~c["pos"]] == 0).all())


def check_grad_labels(c, mode, dtype, G_buf, rscale, cscale, scalars):
    """G_buf: (Bm + 2, pad64(Bn)) of dtype, its last row sentinel"""
    Bm, Bn = c["Bm"], c["Bn"]
    r = grad_labels_ref(c, mode, dtype)
    G = host(G_buf).float()
    pad = torch.ones(Bm + 1, G.shape[1], dtype=torch.bool)
    pad[:Bm, :Bn] = False
    out = {"G": ratio(G[:Bm + 1], r["G"], r["tol_G"]), "G zero row and pad columns exactly zero": exact((G[:Bm + 1][pad] == 0).all()),
           "G past row Bm untouched": exact((G[Bm + 1:] == SENT).all()), "G of a repeat exactly zero (mask)": masked_entries_zero(c, mode, G[:Bm, :Bn]),
           "rscale": ratio(host(rscale), r["rscale"], r["tol_rscale"]), "cscale": ratio(host(cscale), r["cscale"], r["tol_cscale"]),
           "scalars[0] loss": ratio(host(scalars)[0], r["scalars"][0], r["tol_scalars"][0]),
           "scalars[1] dtemp": ratio(host(scalars)[1], r["scalars"][1], r["tol_scalars"][1])}
    return out


NONFINITE_MUTANTS = ("mask_by_multiply", "saturating_store", "colsum_skips_nonfinite")      # (tests/test_nonfinite_cpu.py)


def dropped(c, mode):
    """the entries that take no part under `mode`: the repeats of a column's speech under mask, none under positive"""
    return c["same"] & ~c["pos"] if mode == "mask" else torch.zeros_like(c["same"])


def store(v, dtype, mutant=None):
    """q(), the round-to-nearest store of an fp32 value.  mutant saturating_store: a convert that clamps to the type's largest
    finite value (NaN stays NaN)"""
    if mutant == "saturating_store" and dtype != F32:
        big = torch.finfo(dtype).max
        v = torch.where(torch.isnan(v), v, v.clamp(-big, big))
    return q(v, dtype)


def summed(terms, drop, mutant=None):
    """the terms a column or row sum adds up: a dropped entry is selected out (never multiplied by its zero coefficient).
    mutants: mask_by_multiply leaves the product 0 * l in the sum, colsum_skips_nonfinite adds `isfinite(t) ? t : 0`"""
    if mutant not in ("mask_by_multiply", "masked_entry_leaks_into_sums"):
        terms = torch.where(drop, torch.zeros(()), terms)
    if mutant == "colsum_skips_nonfinite":
        terms = torch.where(torch.isfinite(terms), terms, torch.zeros(()))
    return terms


def emul_D(c, mode, hw=0, mutant=None):
    rl, cl = lse_inputs(c, mode)
    l, same, pos = c["logits"], c["same"], c["pos"]
    col0, Bn = c["col0"], c["Bn"]
    if mutant == "labels_without_col0":
        same = c["labels"][:, None] == c["labels"][None, :Bn]
    d = _exp(l - rl[:, None], hw) + _exp(l - cl[None, :], hw)
    if mode == "positive":
        n = c["counts"][col0:col0 + Bn].float()
        if mutant == "T_by_the_block_local_count":
            n = c["same"][col0:col0 + Bn].float().sum(0)      # the class members among the block's own samples
        d = torch.where(same, d - (2.0 / n)[None, :], d)
        if mutant == "delta_kept_in_positive_mode":
            d = torch.where(pos, d - 2.0, d)
        return d
    d = torch.where(pos, d - 2.0, d)
    if mutant == "masked_entry_leaks_into_sums":
        return d
    return torch.where(same & ~pos, torch.zeros(()), d)


def emul_grad_labels_parts(c, mode, dtype, hw=0, mutant=None):
    """clip_grad_labels_kernel and the scalars kernel behind it: G (with its sentinel row), rscale, cscale, the per-column pairs
    colpart [Bn][2] = (loss share, inv_norm sum_i D l) and scalars"""
    Bm, Bn, col0 = c["Bm"], c["Bn"], c["col0"]
    l, ysq, zsq = c["logits"], c["ysq"], c["zsq"]
    rl, cl = lse_inputs(c, mode)
    inv = torch.tensor(c["inv_norm"], dtype=F32)
    d = emul_D(c, mode, hw, mutant)
    drop = dropped(c, mode)
    ymax = torch.sqrt(ysq.max())
    G = torch.full((Bm + 2, pad64(Bn)), SENT)
    G[:Bm + 1] = 0.0
    coef = d * (ymax / torch.sqrt(ysq))[:, None]
    # (masked_entry_leaks_into_sums: G itself is masked, the sums behind rscale and dtemp are not)
    G[:Bm, :Bn] = store(coef if mutant == "mask_by_multiply" else torch.where(drop, torch.zeros(()), coef), dtype, mutant)
    dl = summed(d * l, drop, mutant).sum(0) * inv
    jj = torch.arange(Bn)
    if mode == "positive":
        n = c["counts"][col0:col0 + Bn].float()
        if mutant == "T_by_the_block_local_count":
            n = c["same"][col0:col0 + Bn].float().sum(0)      # the class members among the block's own samples
        pb = torch.where(c["same"], l, torch.zeros(())).sum(0) / n
    else:
        pb = l[col0 + jj, jj]
    cp0 = (rl[col0 + jj] - pb) + (cl - pb)
    scal = torch.stack([(cp0.double().sum() * float(inv)).float(), dl.double().sum().float()])
    return dict(G=G, rscale=dl / zsq, cscale=inv * _exp(c["temp"], hw) / (ymax * torch.sqrt(zsq)), colpart=torch.stack([cp0, dl], 1), scalars=scal)


def emul_grad_labels(c, mode, dtype, hw=0, mutant=None):
    r = emul_grad_labels_parts(c, mode, dtype, hw, mutant)
    return r["G"], r["rscale"], r["cscale"], r["scalars"]


# ---- sda_clip_grad_y_labels
def grad_y_labels_ref(c, mode, dtype):
    Bm, Bn = c["Bm"], c["Bn"]
    l = c["logits"].double()
    D, mag, extra = label_D(c, mode)
    tol_D = C_D * mag + extra + FTZ
    fz = (math.sqrt(float(c["zsq_all"].double().max())) / torch.sqrt(c["zsq"].double()))[:, None]
    i, ok = gy_rows(c)
    Gy = torch.zeros(Bn + 1, i.numel(), dtype=F64)
    drop, zero = dropped(c, mode), torch.zeros((), dtype=F64)          # (selected out, never 0 * l or 0 * fz)
    Gy[:Bn] = torch.where(ok[None, :], torch.where(drop, zero, D * fz.t())[i].t(), zero)
    tol = torch.ones_like(Gy)
    tol[:Bn] = torch.where(ok[None, :], (tol_D * fz.t())[i].t(), torch.ones((), dtype=F64)) + 5 * U32 * Gy[:Bn].abs() + ulp(Gy[:Bn], dtype)
    nparts = (Bn + 63) // 64
    Dl = torch.where(drop, zero, D * l)
    part = torch.stack([Dl[:, t * 64:(t + 1) * 64].sum(1) for t in range(nparts)])
    tol_part = torch.stack([sum_tol(Dl[:, t * 64:(t + 1) * 64], (tol_D * l.abs() + U32 * Dl.abs())[:, t * 64:(t + 1) * 64], 7, dim=1)
                            for t in range(nparts)])
    return dict(Gy=Gy, tol_Gy=tol, ok=ok, i=i, part=part, tol_part=tol_part)


def check_grad_y_labels(c, mode, dtype, Gy_buf, part_buf):
    """Gy_buf: (Bn + 2, groups * seg_pitch) of dtype, last row sentinel; part_buf: (nparts + 1, Bm) fp32, last row sentinel"""
    Bn = c["Bn"]
    r = grad_y_labels_ref(c, mode, dtype)
    Gy, part = host(Gy_buf).float(), host(part_buf)
    nparts = r["part"].shape[0]
    rep = (c["same"] & ~c["pos"])[r["i"]].t() & r["ok"][None, :]          # [j][column of Gy]
    return {"Gy": ratio(Gy[:Bn + 1], r["Gy"], r["tol_Gy"]), "Gy zero row exactly zero": exact((Gy[Bn] == 0).all()),
            "Gy columns without a row exactly zero": exact((Gy[:Bn][:, ~r["ok"]] == 0).all()),
            "Gy past row Bn untouched": exact((Gy[Bn + 1:] == SENT).all()),
            "Gy of a repeat exactly zero (mask)": 0.0 if mode != "mask" else exact((Gy[:Bn][rep] == 0).all()),
            "part": ratio(part[:nparts], r["part"], r["tol_part"]), "part past its rows untouched": exact((part[nparts:] == SENT).all())}


def emul_grad_y_labels(c, mode, dtype, hw=0, mutant=None):
    Bm, Bn = c["Bm"], c["Bn"]
    l = c["logits"]
    d = emul_D(c, mode, hw, mutant)
    drop = dropped(c, mode)
    zmax = torch.sqrt(c["zsq_all"].max())
    i, ok = gy_rows(c)
    Gy = torch.full((Bn + 2, i.numel()), SENT)
    coef = d * (zmax / torch.sqrt(c["zsq"]))[None, :]
    vals = (coef if mutant == "mask_by_multiply" else torch.where(drop, torch.zeros(()), coef))[i].t()
    Gy[:Bn] = store(torch.where(ok[None, :], vals, torch.zeros(())), dtype, mutant)
    Gy[Bn] = 0.0
    nparts = (Bn + 63) // 64
    part = torch.full((nparts + 1, Bm), SENT)
    dl = summed(d * l, drop, mutant)
    for t in range(nparts):
        part[t] = dl[:, t * 64:(t + 1) * 64].sum(1)
    return Gy, part


# ---- sda_clip_ranks_labels
def ranks_labels_ref(c):
    """cnt_i = #{j : lab_{col0 + j} != lab_i and (l_ij > d_i or (l_ij == d_i and col0 + j < i))}: numpy on the fp32 values as
    float64 (exact), row by row"""
    l, d, lab, col0 = c["logits"].double().numpy(), c["diag"].double().numpy(), c["labels"].numpy(), c["col0"]
    gj = col0 + np.arange(c["Bn"])
    return torch.tensor([int(np.count_nonzero((lab[gj] != lab[i]) & ((l[i] > d[i]) | ((l[i] == d[i]) & (gj < i))))) for i in range(c["Bm"])],
                        dtype=I32)


def emul_ranks_labels(c, mutant=None):
    l, d = c["logits"], c["diag"][:, None]
    ii, jj = torch.arange(c["Bm"])[:, None], torch.arange(c["Bn"])[None, :]
    hit = (l > d) | ((l == d) & (c["col0"] + jj < ii))
    same = c["same"]
    if mutant == "labels_without_col0":
        same = c["labels"][:, None] == c["labels"][None, :c["Bn"]]
    if mutant != "label_blind_ranks":
        hit = hit & ~same
    return hit.float().sum(1).add(0.5).to(I32)


# ---------------------------------------------------------------------------------------------------------------
# the whole loss in float64
# ---------------------------------------------------------------------------------------------------------------
def loss_ref(l, labels, mode, reduction="mean"):
    """The labelled loss of a float64 logits matrix l (speech rows x brain columns of the whole batch) in its two-line autograd
    forms: soft-target cross-entropy both ways, or masked_fill(-inf) plus cross-entropy.  labels None: the reference's loss."""
    ce = torch.nn.functional.cross_entropy
    B = l.shape[0]
    tgt = torch.arange(B)
    if labels is None:
        return (ce(l, tgt, reduction=reduction) + ce(l.t(), tgt, reduction=reduction)) / 2
    same = labels[:, None] == labels[None, :]
    if mode == "positive":
        T = same.double() / same.sum(1, keepdim=True)
        return (ce(l, T, reduction=reduction) + ce(l.t(), T, reduction=reduction)) / 2
    lm = l.masked_fill(same & ~torch.eye(B, dtype=torch.bool), -math.inf)
    return (ce(lm, tgt, reduction=reduction) + ce(lm.t(), tgt, reduction=reduction)) / 2


def loss_ref_embeddings(x, y, temp, labels, mode, reduction="mean", fast=True):
    """float64 autograd of the labelled loss on embeddings x (speech), y (brain), (B, F, T): (loss, dx, dy, dtemp, logits)"""
    x = x.detach().double().cpu().requires_grad_(True)
    y = y.detach().double().cpu().requires_grad_(True)
    t = torch.tensor([float(temp)], dtype=F64, requires_grad=True)
    B = x.shape[0]
    X, Y = x.reshape(B, -1), y.reshape(B, -1)
    lg = (X / X.norm(dim=1, keepdim=True)) @ (Y / Y.norm(dim=1, keepdim=True)).T
    if fast:
        lg = lg * torch.exp(t)
    lab = None if labels is None else torch.as_tensor(labels).cpu().to(torch.int64)
    loss = loss_ref(lg, lab, mode, reduction)
    dx, dy, dt = torch.autograd.grad(loss, [x, y, t], allow_unused=True)
    return loss.detach(), dx, dy, (dt if dt is not None else torch.zeros(1, dtype=F64)), lg.detach()


def global_D_ref(c, mode):
    """autograd's d loss_ref / d l on the global fp32 logits of a case, divided by inv_norm: what D must equal on the block"""
    l = c["Lg32"].double().requires_grad_(True)
    (g,) = torch.autograd.grad(loss_ref(l, c["labels"].to(torch.int64), mode, "mean"), [l])
    return g / c["inv_norm"]


# ---------------------------------------------------------------------------------------------------------------
# measuring the table
# ---------------------------------------------------------------------------------------------------------------
def measure_constants(cases):
    """largest error of the emulations against float64 in units of each new constant's magnitude, over the given cases and HW"""
    m = dict(C_MLSE=0.0, C_PBAR=0.0)
    for c in cases:
        l32 = c["logits"].double()
        keep = keep_of(c)
        ninf = torch.full((), -math.inf, dtype=F64)
        lm = torch.where(keep, l32, ninf)
        rl, cl = torch.logsumexp(lm, 1), torch.logsumexp(lm, 0)
        ok = keep.any(1)
        one, onec = torch.ones_like(rl), torch.ones_like(cl)
        mag_r = ulp32(torch.maximum(torch.maximum(rl.abs(), lm.amax(1).abs()), one))
        mag_c = ulp32(torch.maximum(torch.maximum(cl.abs(), lm.amax(0).abs()), onec))
        for hw in HW:
            er = (emul_masked_lse(c["logits"], keep, 1, hw)[2].double() - rl).abs() / mag_r
            ec = (emul_masked_lse(c["logits"], keep, 0, hw)[2].double() - cl).abs() / mag_c
            m["C_MLSE"] = max(m["C_MLSE"], float(er[ok].max()) if bool(ok.any()) else 0.0, float(ec.max()))
        pb, _, mag = pbar_ref(c)
        n = c["counts"][c["col0"]:c["col0"] + c["Bn"]].float()
        pb32 = torch.where(c["same"], c["logits"], torch.zeros(())).sum(0) / n
        nz = mag > 0
        if bool(nz.any()):
            m["C_PBAR"] = max(m["C_PBAR"], float(((pb32.double() - pb).abs()[nz] / mag[nz]).max()))
    return m
