"""Inputs, float64 references, tolerances and plain-torch fp32 emulations for the kernel-level tests of csrc/sa_loss.hip: the
SpatialAttention weight build and its backward, and the CLIP loss tail (logits and soft-max statistics, the coefficient matrices
G and Gy, the loss scalars, the retrieval ranks, the cross-rank merge).  tests/test_sa_loss_cpu.py proves on the CPU that the
cases reach their edges and catch the planted bugs; tests/test_sa_loss_gpu.py holds the HIP kernels to the same check_*()
functions.  Nothing here needs a GPU.

Every kernel is handed exact fp32 inputs and its float64 reference is computed from those fp32 values, so a comparison sees one
kernel's arithmetic only.  Tolerances follow the convention at the top of tests/elementwise_cases.py (u = 2^-24); none comes
from a kernel's output:
  stored value   ulp(ref, dtype).
  sums           n u sum|t_i| + the terms' own tolerances + one ulp of the sum (sum_tol / dot_tol, the same bound for products
                 too large to keep term by term).  n: 2 K2 + chunks (slabs on the matrix path) for a; ceil(n / 256) + 9 for a
                 256-thread block sum (a thread's strided terms, 6 shuffle levels, 3 adds of the wave partials): block_acc().
  formulas       C x (magnitude); C = 4 x the largest error of this file's fp32 emulation against float64 over every case below,
                 measured on the CPU (x86-64, torch's IEEE fp32) with every exp result moved by -1, 0, +1 ulp.  The factor 4 covers
                 the device's libm and instruction selection.  test_sa_loss_cpu.py::test_tolerance_table_matches_the_emulation
                 measures the middle column again and holds the chosen values to 4 .. 5 x measured.

      constant   measured on the CPU   chosen     magnitude it multiplies
      C_SM       4.03 u                16.5 u     max(1, |a - max|) W              soft-max weight (+ block_acc u W for the sum, + 2^-126)
      C_LOGIT    5.95 u                24 u       |l|                              l = S e^temp / (sqrt ysq sqrt zsq)
      C_LSE      2.09                  8.5        ulp32(max(|lse|, |max|, 1))      max + log sum (+ block_acc u for the sum)
      C_D        1.13                  4.6        ulp32(max(|l|, |lse_i|, 1)) p_row + ulp32(max(|l|, |lse_j|, 1)) p_col + ulp32(D)
"""
import math

import torch

from speech_decoding_amd import lib as L
from tests.elementwise_cases import DTYPES, FTZ, SENT, U32, _nudge, q, ratio, sum_tol, ulp  # noqa: F401

F32, F64 = torch.float32, torch.float64
SA_R, SA_MC = 8, 128                 # csrc/sa_loss.hip: rows per workgroup, Fourier modes per chunk
HW = (-1, 0, 1)                      # ulps every exp result of an emulation is moved by
pad64 = L.pad_channels

C_SM = 16.5 * U32
C_LOGIT = 24.0 * U32
C_LSE = 8.5
C_D = 4.6


def _gen(seed):
    return torch.Generator().manual_seed(seed)


def _exp(x, hw=0):
    return _nudge(torch.exp(x.double()).float(), hw)


def _log(x):
    return torch.log(x.double()).float()


def ulp32(x):
    return ulp(x, F32)


def block_acc(n):
    """additions an fp32 accumulator of a 256-thread block reduction over n terms sees at most"""
    return (n + 255) // 256 + 9


def dot_tol(absum, s, n_acc, term_tol_sum=0.0):
    """sum_tol() for a contraction given as sum|t_i| (absum) and the exact sum s, without the terms themselves"""
    return term_tol_sum + n_acc * U32 * absum + ulp32(s)


def exact(ok):
    """an exact comparison as an error / tolerance figure"""
    return 0.0 if bool(ok) else math.inf


def host(t):
    return t.detach().cpu()


# ---------------------------------------------------------------------------------------------------------------
# SpatialAttention
# ---------------------------------------------------------------------------------------------------------------
# (D1, K2, C, matrix path).  D1: one row, SA_R, one past it, a ragged last group.  K2 stand-alone: one chunk, SA_MC, one past, a
# second blockIdx.y of the backward (257).  K2 matrix path: 2 K2 % 64 == 0.  C: both sides of the 256-thread stride and the cap.
SA_SHAPES = ((1, 1, 1, False), (8, 36, 60, False), (8, 128, 208, False), (9, 128, 256, False), (20, 129, 257, False),
             (9, 257, 306, False), (20, 257, 512, False), (20, 32, 208, True), (9, 1024, 306, True), (20, 1024, 512, True))
SA_REGIMES = ("o1", "saturated", "zero")
SA_MASKS = ("none", "dropped", "zero")
# largest a of row r in the saturated regime (the smallest is about minus that): about +-80.  e^88.7 is fp32's overflow threshold, so the rows above it are the ones
# that need the max subtraction; a - max reaches -190, where exp underflows to zero.
SAT_AMPS = (80.0, 95.0, 70.0, 90.0)


def sa_case(D1, K2, C, regime, mask_kind):
    g = _gen(100003 * D1 + 101 * K2 + C)
    th = torch.rand(K2, C, generator=g, dtype=F64) * 2 * math.pi
    cos, sin = torch.cos(th).float(), torch.sin(th).float()
    z = torch.randn(D1, K2, 2, generator=g, dtype=F64) * (2.0 / math.sqrt(2 * K2))            # a = O(1)
    dWd = torch.randn(D1, C, generator=g)
    drop = (torch.rand(C, generator=g) > 0.3).float()
    drop[0] = 0.0
    if regime == "zero":
        z = torch.zeros_like(z)
    elif regime == "saturated":
        a = z[..., 0] @ cos.double() + z[..., 1] @ sin.double()
        amp = torch.tensor([SAT_AMPS[r % 4] for r in range(D1)], dtype=F64)
        z = z * (amp / a.amax(1).abs())[:, None, None]              # the row's largest score is +amp
    mask = {"none": None, "dropped": drop, "zero": torch.zeros(C)}[mask_kind]
    return dict(name=f"sa D1={D1} K2={K2} C={C} {regime} mask={mask_kind}", D1=D1, K2=K2, C=C, regime=regime, mask_kind=mask_kind,
                z=z.float(), cos=cos, sin=sin, mask=mask, dWd=dWd, D1p=pad64(D1), Cp=pad64(C))


def sm_tol(a, W, C):
    """the soft-max of exact fp32 scores a: float64 a, W"""
    return C_SM * (a - a.amax(1, keepdim=True)).abs().clamp(min=1.0) * W + block_acc(C) * U32 * W + FTZ


def sa_forward_ref(case, gemm):
    """float64 a, W and their tolerances from the fp32 z and tables"""
    zr, zi = case["z"][..., 0].double(), case["z"][..., 1].double()
    co, si = case["cos"].double(), case["sin"].double()
    K2, C = case["K2"], case["C"]
    a = zr @ co + zi @ si
    n_acc = 2 * K2 + ((2 * K2) // 32 if gemm else (K2 + SA_MC - 1) // SA_MC)
    tol_a = dot_tol(zr.abs() @ co.abs() + zi.abs() @ si.abs(), a, n_acc)
    W = torch.softmax(a, 1)
    tol_W = W * (tol_a + (W * tol_a).sum(1, keepdim=True)) + sm_tol(a, W, C)
    return dict(a=a, tol_a=tol_a, W=W, tol_W=tol_W)


def mask_of(case):
    return torch.ones(case["C"]) if case["mask"] is None else case["mask"]


def packed_ref(W, tol_W, case, dtype):
    """(D1p, Cp) float64 image of the packed operand and the tolerance of its [D1, C] corner"""
    ref = torch.zeros(case["D1p"], case["Cp"], dtype=F64)
    ref[:case["D1"], :case["C"]] = W * mask_of(case).double()
    tol = torch.ones_like(ref)
    tol[:case["D1"], :case["C"]] = tol_W * mask_of(case).double() + ulp(ref[:case["D1"], :case["C"]], dtype)
    return ref, tol


def check_sa_forward(case, dtype, W_buf, Wp_buf, W_ref, tol_W):
    """W_buf: (D1 + 1, C) fp32 whose last row the kernel must leave at the sentinel; Wp_buf: (D1p, Cp) of dtype"""
    D1, C = case["D1"], case["C"]
    W_buf, Wp = host(W_buf), host(Wp_buf).float()
    ref, tol = packed_ref(W_ref, tol_W, case, dtype)
    corner = torch.zeros_like(ref, dtype=torch.bool)
    corner[:D1, :C] = True
    out = {"W": ratio(W_buf[:D1], W_ref, tol_W), "W outside [D1, C] untouched": exact((W_buf[D1:] == SENT).all()),
           "Wp": ratio(Wp, ref, tol), "Wp padding exactly zero": exact((Wp[~corner] == 0).all())}
    if case["regime"] == "zero":
        third = torch.full((D1, C), 1.0 / C, dtype=F64)
        out["W within one ulp of 1/C"] = ratio(W_buf[:D1], third, ulp32(third))
    if case["mask_kind"] == "zero":
        out["Wp exactly zero under an all-zero mask"] = exact((Wp == 0).all())
    return out


def emul_softmax_pack(a, case, dtype, hw=0, mutant=None):
    """sa_fwd_final_kernel on fp32 scores a (D1, C): (W buffer (D1 + 1, C), Wp buffer (D1p, Cp) as fp32 of dtype)"""
    D1, C = case["D1"], case["C"]
    W_buf = torch.full((D1 + 1, C), SENT)
    Wp = torch.full((case["D1p"], case["Cp"]), SENT)
    Wp[D1:] = 0.0
    n = min(C, 256) if mutant == "sa_drop_sensors_ge_256" else C
    a = a[:, :n]
    if mutant == "sa_no_max_subtraction":
        ex = _exp(a, hw)
    else:
        ex = _exp(a - a.amax(1, keepdim=True), hw)
    w = ex * (1.0 / ex.sum(1, keepdim=True))
    m = mask_of(case)[:n]
    W_buf[:D1, :n] = w * m if mutant == "sa_mask_on_W" else w
    Wp[:D1, :n] = q(w * m, dtype)
    Wp[:D1, C:] = 0.0
    return W_buf, Wp


def emul_sa_scores(case, mutant=None):
    """sa_fwd_partial_kernel + the ordered chunk sum: fp32 a (D1, C)"""
    zr, zi = case["z"][..., 0], case["z"][..., 1]
    nchunk = (case["K2"] + SA_MC - 1) // SA_MC
    a = torch.zeros(case["D1"], case["C"])
    for j in range(nchunk - 1 if (mutant == "sa_drop_last_chunk" and nchunk > 1) else nchunk):
        s = slice(j * SA_MC, (j + 1) * SA_MC)
        a = a + (zr[:, s] @ case["cos"][s] + zi[:, s] @ case["sin"][s])
    return a


def sa_backward_ref(case, W32, gemm):
    """float64 da (D1, C) and dz (D1, K2, 2) from the fp32 W handed to the kernel, with tolerances"""
    C = case["C"]
    W = W32.double()
    dw = case["dWd"].double() * mask_of(case).double()
    dot = (dw * W).sum(1, keepdim=True)
    tol_dot = sum_tol(dw * W, U32 * (dw * W).abs(), block_acc(C), dim=1)[:, None]
    da = W * (dw - dot)
    tol_da = W * tol_dot + 2 * U32 * W * (dw.abs() + dot.abs()) + FTZ
    Cq = pad64(C)
    n_acc = Cq + Cq // 32 if gemm else C
    co, si = case["cos"].double().t(), case["sin"].double().t()                # (C, K2)
    dz = torch.stack([da @ co, da @ si], -1)
    tol_dz = torch.stack([dot_tol(da.abs() @ co.abs(), dz[..., 0], n_acc, tol_da @ co.abs()),
                          dot_tol(da.abs() @ si.abs(), dz[..., 1], n_acc, tol_da @ si.abs())], -1)
    return dict(da=da, tol_da=tol_da, dz=dz, tol_dz=tol_dz)


def dwd_padded(case):
    """dWd as the kernels get it: (D1p, pitch > C) fp32 with NaN in the pad columns and in the rows >= D1 (never read)"""
    out = torch.full((case["D1p"], pad64(case["C"] + 1)), math.nan)
    out[:case["D1"], :case["C"]] = case["dWd"]
    return out


def check_sa_backward(case, dz_buf, ref):
    """dz_buf: (D1 + 1, K2, 2) fp32, last row sentinel"""
    dz = host(dz_buf)
    out = {"dz": ratio(dz[:case["D1"]], ref["dz"], ref["tol_dz"]), "dz outside [D1] untouched": exact((dz[case["D1"]:] == SENT).all())}
    if case["mask_kind"] == "zero":
        out["dz exactly zero under an all-zero mask"] = exact((dz[:case["D1"]] == 0).all())
    return out


def check_sa_softmax_backward(case, da_buf, ref):
    """da_buf: (D1 + 1, pitch) fp32, last row sentinel; pad columns [C, pitch) exact zeros"""
    da, D1, C = host(da_buf), case["D1"], case["C"]
    return {"da": ratio(da[:D1, :C], ref["da"], ref["tol_da"]), "da pad columns exactly zero": exact((da[:D1, C:] == 0).all()),
            "da outside [D1] untouched": exact((da[D1:] == SENT).all())}


def emul_sa_softmax_backward(case, W32, pitch, mutant=None):
    D1, C = case["D1"], case["C"]
    dWd = dwd_padded(case)[:D1, :C]
    dw = dWd * mask_of(case)
    dot = ((dWd if mutant == "sa_dot_without_mask" else dw) * W32).sum(1, keepdim=True)
    buf = torch.full((D1 + 1, pitch), SENT)
    buf[:D1, :C] = W32 * (dw - dot)
    if mutant != "sa_da_pads_unwritten":
        buf[:D1, C:] = 0.0
    return buf


def emul_sa_backward(case, W32, mutant=None):
    D1, C, K2 = case["D1"], case["C"], case["K2"]
    da = emul_sa_softmax_backward(case, W32, C, mutant)[:D1]
    re, im = da @ case["cos"].t(), da @ case["sin"].t()
    if mutant == "sa_dz_re_im_swapped":
        re, im = im, re
    buf = torch.full((D1 + 1, K2, 2), SENT)
    m = min(K2, 256) if mutant == "sa_backward_drop_m_ge_256" else K2
    buf[:D1, :m] = torch.stack([re, im], -1)[:, :m]
    return buf


# ---------------------------------------------------------------------------------------------------------------
# CLIP tail
# ---------------------------------------------------------------------------------------------------------------
# (Bm, Bn, col0): the block of local brain columns [col0, col0 + Bn) of a global batch of Bm speech rows
CLIP_SHAPES = ((1, 1, 0), (3, 3, 0), (64, 64, 0), (255, 255, 0), (257, 257, 0), (300, 300, 0), (513, 70, 140), (140, 70, 70), (15, 5, 10),
               (512, 256, 256))
# segmented Gy layouts (seg, seg_pitch, groups); every other block: the plain layout (Bm, pad64(Bm), 1)
GY_LAYOUT = {(15, 5, 10): (5, 64, 3), (140, 70, 70): (70, 128, 2), (512, 256, 256): (256, 256, 2)}
CLIP_REGIMES = ("flat", "trained", "saturated", "hot", "ties", "norms")


def gy_layout(Bm, Bn, col0):
    return GY_LAYOUT.get((Bm, Bn, col0), (Bm, pad64(Bm), 1))


def clip_case(Bm, Bn, col0, regime):
    """The global problem (Bg = Bm speech rows and as many brain columns, positives on the diagonal) is built in float64 and rounded
    once to fp32; the block is its column slice.  Every later kernel's fp32 inputs are the rounded float64 results of the stage
    before it."""
    Bg = Bm
    g = _gen(7919 * Bm + 31 * Bn + col0 + 1000003 * CLIP_REGIMES.index(regime))
    rnd = lambda *s: torch.randn(*s, generator=g, dtype=F64)
    ny = 30.0 * torch.exp(0.3 * rnd(Bg))
    nz = 30.0 * torch.exp(0.3 * rnd(Bg))
    if regime == "norms":
        # ysq and zsq span 2^16, the norms 2^8.  The stored O(1) part |D| ymax / |Y_i| <= 2 x 1.5 x 2^8 = 768 < 65504, fp16's
        # largest finite value: the factor ymax / |Y_i| is what can leave fp16's range, and it is not tested beyond it.
        e = torch.linspace(-4.0, 4.0, Bg, dtype=F64)
        ny = 30.0 * torch.exp2(e[torch.randperm(Bg, generator=g)])
        nz = 30.0 * torch.exp2(e[torch.randperm(Bg, generator=g)])
    if Bm > Bn:                                                        # the largest norms lie outside the local block
        out = col0 + Bn if col0 + Bn < Bm else 0
        ny[out], nz[out] = 1.5 * float(ny.max()), 1.5 * float(nz.max())
    temp, pos, neg = {"flat": (0.0, None, 0.2), "trained": (5.1, 0.02, 0.002), "saturated": (5.1, 0.999, 0.002), "hot": (9.0, 0.5, 0.05),
                      "ties": (5.1, 0.02, 0.002), "norms": (5.1, 0.02, 0.002)}[regime]
    Cg = (neg * rnd(Bg, Bg)).clamp(-0.95, 0.95)
    if pos is not None:
        Cg[torch.arange(Bg), torch.arange(Bg)] = pos
    Sg = (Cg * ny[:, None] * nz[None, :]).float()
    ysq, zsq_all = (ny * ny).float(), (nz * nz).float()
    if regime == "ties":
        if Bm >= 3:                                                    # two identical rows
            Sg[Bm - 1], ysq[Bm - 1] = Sg[1], ysq[1]
        if Bn >= 2:                                                    # two identical columns: the first and the last of the block,
            Sg[:, col0 + Bn - 1], zsq_all[col0 + Bn - 1] = Sg[:, col0], zsq_all[col0]     # each the other's positive's equal
    temp32 = torch.tensor([temp], dtype=F32)
    alpha = torch.exp(temp32.double())
    Lg = Sg.double() * alpha / (torch.sqrt(ysq.double())[:, None] * torch.sqrt(zsq_all.double())[None, :])
    cols = slice(col0, col0 + Bn)
    S = torch.full((Bm, pad64(Bn)), math.nan)                          # pitch > Bn, the padding is never read
    S[:, :Bn] = Sg[:, cols]
    Lg32 = Lg.float()
    c = dict(name=f"clip Bm={Bm} Bn={Bn} col0={col0} {regime}", Bm=Bm, Bn=Bn, col0=col0, regime=regime, S=S, ysq=ysq, zsq=zsq_all[cols].clone(),
             zsq_all=zsq_all, temp=temp32, inv_norm=float(torch.tensor(1.0 / (2 * Bg), dtype=F32)), l64=Lg[:, cols],
             Lg32=Lg32, logits=Lg32[:, cols].contiguous(), row_lse=torch.logsumexp(Lg32.double(), 1).float(),
             col_lse_all=torch.logsumexp(Lg32.double(), 0).float())
    c["col_lse"] = c["col_lse_all"][cols].clone()
    ii = torch.arange(Bm)
    inb = (ii >= col0) & (ii < col0 + Bn)
    c["inb"] = inb
    c["diag"] = torch.where(inb, c["logits"][ii, (ii - col0).clamp(0, Bn - 1)], torch.zeros(Bm))
    return c


def lse_tol(lse, mx, n):
    return C_LSE * ulp32(torch.maximum(torch.maximum(lse.abs(), mx.abs()), torch.ones_like(lse))) + block_acc(n) * U32


# ---- clip_logits_stats
def logits_stats_ref(c):
    l = c["l64"]
    tol_l = C_LOGIT * l.abs() + FTZ
    mx, tmx = l.amax(1), tol_l.amax(1)
    e = torch.exp(l - mx[:, None])
    rs = e.sum(1)
    tol_rs = (e * (2 * tmx[:, None] + C_SM * (l - mx[:, None]).abs().clamp(min=1.0))).sum(1) + block_acc(c["Bn"]) * U32 * rs
    rl, cl = torch.logsumexp(l, 1), torch.logsumexp(l, 0)
    ii = torch.arange(c["Bm"])
    jj = (ii - c["col0"]).clamp(0, c["Bn"] - 1)
    return dict(l=l, tol_l=tol_l, row_max=mx, tol_row_max=tmx, row_sum=rs, tol_row_sum=tol_rs, row_lse=rl,
                tol_row_lse=tmx + lse_tol(rl, mx, c["Bn"]), col_lse=cl, tol_col_lse=tol_l.amax(0) + lse_tol(cl, l.amax(0), c["Bm"]),
                diag=torch.where(c["inb"], l[ii, jj], torch.zeros(c["Bm"], dtype=F64)), tol_diag=tol_l[ii, jj])


def check_logits_stats(c, logits, row_max, row_sum, col_lse, diag, row_lse):
    r = logits_stats_ref(c)
    logits, row_max, row_sum, col_lse, diag, row_lse = map(host, (logits, row_max, row_sum, col_lse, diag, row_lse))
    inb = c["inb"]
    return {"logits": ratio(logits, r["l"], r["tol_l"]), "row_max": ratio(row_max, r["row_max"], r["tol_row_max"]),
            "row_sum": ratio(row_sum, r["row_sum"], r["tol_row_sum"]), "row_lse": ratio(row_lse, r["row_lse"], r["tol_row_lse"]),
            "row_max + log row_sum": ratio(row_max.double() + torch.log(row_sum.double()), r["row_lse"], r["tol_row_lse"]),
            "col_lse": ratio(col_lse, r["col_lse"], r["tol_col_lse"]), "diag": ratio(diag[inb], r["diag"][inb], r["tol_diag"][inb]),
            "diag exactly zero outside the block": exact((diag[~inb] == 0).all())}


def emul_lse(x, dim, hw=0, mutant=None):
    """(max, sum exp(x - max), lse) along dim, fp32"""
    mx = x.amax(dim)
    s = _exp(x - mx.unsqueeze(dim), hw).sum(dim)
    if mutant == "clip_lse_without_max":
        return mx, s, _log(_exp(x, hw).sum(dim))
    return mx, s, mx + _log(s)


def emul_logits_stats(c, hw=0, mutant=None):
    Bm, Bn, col0 = c["Bm"], c["Bn"], c["col0"]
    ri = _exp(c["temp"], hw) / torch.sqrt(c["ysq"])
    l = c["S"][:, :Bn] * ri[:, None] / torch.sqrt(c["zsq"])[None, :]
    mx, s, rl = emul_lse(l, 1, hw, mutant)
    cl = emul_lse(l, 0, hw, mutant)[2]
    ii = torch.arange(Bm)
    diag = torch.where(c["inb"], l[ii, (ii - col0).clamp(0, Bn - 1)], torch.full((Bm,), SENT if mutant == "clip_diag_not_zeroed" else 0.0))
    return l, mx, s, cl, diag, rl


def tied_entries_equal(c, M, transposed=False, row_of_col=None):
    """the ties regime: the two identical brain columns and the two identical speech rows give the same bits wherever the -2 of
    a positive is not involved.  M: [speech row][brain column] (G), or transposed with the speech row of every column (Gy)."""
    Bm, Bn, col0 = c["Bm"], c["Bn"], c["col0"]
    if c["regime"] != "ties":
        return 0.0
    M = M.t() if transposed else M
    ok = True
    if row_of_col is None:
        idx = torch.arange(Bm)
        sel = lambda i: idx == i
    else:
        i_of, valid = row_of_col
        sel = lambda i: valid & (i_of == i)
        M = M[:i_of.numel()]
    if Bn >= 2:
        rows = ~(sel(col0) | sel(col0 + Bn - 1))
        if row_of_col is not None:
            rows = rows & row_of_col[1]
        ok = ok and torch.equal(M[rows][:, 0], M[rows][:, Bn - 1])
    if Bm >= 3:
        cols = torch.ones(Bn, dtype=torch.bool)
        for i in (1, Bm - 1):
            if col0 <= i < col0 + Bn:
                cols[i - col0] = False
        a, b = M[sel(1)], M[sel(Bm - 1)]
        ok = ok and a.shape[0] == 1 and b.shape[0] == 1 and torch.equal(a[:, cols], b[:, cols])
    return exact(ok)


# ---- D, clip_grad
def clip_D(c, logits=None, row_lse=None, col_lse=None, col0=None):
    """float64 D and its tolerance from the fp32 logits, row_lse, col_lse the kernels are handed (default: the block's)"""
    l = (c["logits"] if logits is None else logits).double()
    rl = (c["row_lse"] if row_lse is None else row_lse).double()[:, None]
    cl = (c["col_lse"] if col_lse is None else col_lse).double()[None, :]
    col0 = c["col0"] if col0 is None else col0
    pr, pc = torch.exp(l - rl), torch.exp(l - cl)
    D = pr + pc
    jj = torch.arange(l.shape[1])
    D[col0 + jj, jj] -= 2.0
    one = torch.ones_like(l)
    mag = ulp32(torch.maximum(torch.maximum(l.abs(), rl.abs().expand_as(l)), one)) * pr + \
        ulp32(torch.maximum(torch.maximum(l.abs(), cl.abs().expand_as(l)), one)) * pc + ulp32(D)
    return D, mag


def clip_grad_ref(c, dtype):
    Bm, Bn, col0, inv = c["Bm"], c["Bn"], c["col0"], c["inv_norm"]
    l = c["logits"].double()
    D, mag = clip_D(c)
    tol_D = C_D * mag + FTZ
    ysq, zsq = c["ysq"].double(), c["zsq"].double()
    ymax = math.sqrt(float(ysq.max()))
    f = (ymax / torch.sqrt(ysq))[:, None]
    G = torch.zeros(Bm + 1, pad64(Bn), dtype=F64)
    G[:Bm, :Bn] = D * f
    tol_G = torch.ones_like(G)
    # sqrt, sqrt, quotient, product: four roundings and one to spare
    tol_G[:Bm, :Bn] = f * tol_D + 5 * U32 * G[:Bm, :Bn].abs() + ulp(G[:Bm, :Bn], dtype)
    dl = (D * l).sum(0)
    tol_dl = sum_tol(D * l, tol_D * l.abs() + U32 * (D * l).abs(), block_acc(Bm), dim=0)
    rscale = inv * dl / zsq
    alpha = float(torch.exp(c["temp"].double()))
    cscale = inv * alpha / (ymax * torch.sqrt(zsq))
    jj = torch.arange(Bn)
    rl, cl, ljj = c["row_lse"].double()[col0 + jj], c["col_lse"].double(), l[col0 + jj, jj]
    cp0 = (rl - ljj) + (cl - ljj)
    tol_cp0 = U32 * ((rl - ljj).abs() + (cl - ljj).abs() + cp0.abs())
    s0, s1 = inv * cp0.sum(), inv * dl.sum()
    # the kernel adds the fp32 column partials in float64: their own tolerances summed, plus one fp32 ulp of the result
    return dict(G=G, tol_G=tol_G, rscale=rscale, tol_rscale=inv * tol_dl / zsq + 3 * U32 * rscale.abs() + FTZ,
                # exp(temp), two square roots, two products and a quotient: a logit's operations and one more
                cscale=cscale, tol_cscale=2 * C_LOGIT * cscale,
                scalars=torch.stack([s0, s1]),
                tol_scalars=torch.stack([inv * tol_cp0.sum() + ulp32(s0), (inv * tol_dl + 2 * U32 * (inv * dl).abs()).sum() + ulp32(s1)]))


def check_clip_grad(c, dtype, G_buf, rscale, cscale, scalars):
    """G_buf: (Bm + 2, pad64(Bn)) of dtype, its last row sentinel"""
    Bm, Bn = c["Bm"], c["Bn"]
    r = clip_grad_ref(c, dtype)
    G = host(G_buf).float()
    pad = torch.ones(Bm + 1, G.shape[1], dtype=torch.bool)
    pad[:Bm, :Bn] = False
    return {"G": ratio(G[:Bm + 1], r["G"], r["tol_G"]), "G zero row and pad columns exactly zero": exact((G[:Bm + 1][pad] == 0).all()),
            "G past row Bm untouched": exact((G[Bm + 1:] == SENT).all()), "G of tied entries equal": tied_entries_equal(c, G[:Bm, :Bn]),
            "rscale": ratio(host(rscale), r["rscale"], r["tol_rscale"]),
            "cscale": ratio(host(cscale), r["cscale"], r["tol_cscale"]), "scalars[0] loss": ratio(host(scalars)[0], r["scalars"][0], r["tol_scalars"][0]),
            "scalars[1] dtemp": ratio(host(scalars)[1], r["scalars"][1], r["tol_scalars"][1])}


def emul_D(l, rl, cl, col0, hw=0, mutant=None):
    d = _exp(l - rl[:, None], hw) + _exp(l - cl[None, :], hw)
    jj = torch.arange(l.shape[1])
    rows = jj if mutant == "clip_delta_at_i_eq_j" else col0 + jj
    d[rows, jj] = d[rows, jj] - 2.0
    return d


def emul_clip_grad(c, dtype, hw=0, mutant=None):
    Bm, Bn, col0 = c["Bm"], c["Bn"], c["col0"]
    l, rl, cl, ysq, zsq = c["logits"], c["row_lse"], c["col_lse"], c["ysq"], c["zsq"]
    inv = torch.tensor(c["inv_norm"], dtype=F32)
    d = emul_D(l, rl, cl, col0, hw, mutant)
    ymax = torch.sqrt((ysq[col0:col0 + Bn] if mutant == "clip_ymax_over_block_rows" else ysq).max())
    G = torch.full((Bm + 2, pad64(Bn)), SENT)
    G[:Bm + 1] = 0.0
    G[:Bm, :Bn] = q(d * (ymax / torch.sqrt(ysq))[:, None], dtype)
    dl = (d * l).sum(0) * inv
    jj = torch.arange(Bn)
    ljj = l[col0 + jj, jj]
    rlj = rl[jj] if mutant == "clip_row_lse_local_index" else rl[col0 + jj]
    cp0 = (rlj - ljj) + (cl - ljj)
    scal = torch.stack([(cp0.double().sum() * float(inv)).float(), dl.double().sum().float()])
    return G, dl / zsq, inv * _exp(c["temp"], hw) / (ymax * torch.sqrt(zsq)), scal


# ---- clip_grad_y and its finisher
def gy_rows(c):
    """for every column of Gy: the speech row it holds and whether it holds one"""
    seg, seg_pitch, groups = gy_layout(c["Bm"], c["Bn"], c["col0"])
    cc = torch.arange(groups * seg_pitch)
    o = cc % seg_pitch
    i = (cc // seg_pitch) * seg + o
    return i.clamp(max=c["Bm"] - 1), (o < seg) & (i < c["Bm"])


def clip_grad_y_ref(c, dtype):
    Bm, Bn = c["Bm"], c["Bn"]
    l = c["logits"].double()
    D, mag = clip_D(c)
    tol_D = C_D * mag + FTZ
    fz = (math.sqrt(float(c["zsq_all"].double().max())) / torch.sqrt(c["zsq"].double()))[:, None]
    i, ok = gy_rows(c)
    Gy = torch.zeros(Bn + 1, i.numel(), dtype=F64)
    Gy[:Bn] = torch.where(ok[None, :], (D * fz.t())[i].t(), torch.zeros((), dtype=F64))
    tol = torch.ones_like(Gy)
    tol[:Bn] = torch.where(ok[None, :], (tol_D * fz.t())[i].t(), torch.ones((), dtype=F64)) + 5 * U32 * Gy[:Bn].abs() + ulp(Gy[:Bn], dtype)
    nparts = (Bn + 63) // 64
    part = torch.stack([(D * l)[:, t * 64:(t + 1) * 64].sum(1) for t in range(nparts)])
    # a wave sum: 6 shuffle levels
    tol_part = torch.stack([sum_tol((D * l)[:, t * 64:(t + 1) * 64], (tol_D * l.abs() + U32 * (D * l).abs())[:, t * 64:(t + 1) * 64], 7, dim=1)
                            for t in range(nparts)])
    return dict(Gy=Gy, tol_Gy=tol, ok=ok, part=part, tol_part=tol_part)


def check_clip_grad_y(c, dtype, Gy_buf, part_buf):
    """Gy_buf: (Bn + 2, groups * seg_pitch) of dtype, last row sentinel; part_buf: (nparts + 1, Bm) fp32, last row sentinel"""
    Bn = c["Bn"]
    r = clip_grad_y_ref(c, dtype)
    Gy, part = host(Gy_buf).float(), host(part_buf)
    nparts = r["part"].shape[0]
    return {"Gy": ratio(Gy[:Bn + 1], r["Gy"], r["tol_Gy"]), "Gy zero row exactly zero": exact((Gy[Bn] == 0).all()),
            "Gy columns without a row exactly zero": exact((Gy[:Bn][:, ~r["ok"]] == 0).all()),
            "Gy past row Bn untouched": exact((Gy[Bn + 1:] == SENT).all()),
            "Gy of tied entries equal": tied_entries_equal(c, Gy[:Bn], True, (gy_rows(c)[0], r["ok"])), "part": ratio(part[:nparts], r["part"], r["tol_part"]),
            "part past its rows untouched": exact((part[nparts:] == SENT).all())}


def emul_clip_grad_y(c, dtype, hw=0, mutant=None):
    Bm, Bn, col0 = c["Bm"], c["Bn"], c["col0"]
    l = c["logits"]
    d = emul_D(l, c["row_lse"], c["col_lse"], col0, hw)
    zmax = torch.sqrt((c["zsq"] if mutant == "clip_zmax_over_local_zsq" else c["zsq_all"]).max())
    i, ok = gy_rows(c)
    if mutant == "clip_gy_map_without_gap":
        i = torch.arange(i.numel())
        ok = i < Bm
        i = i.clamp(max=Bm - 1)
    Gy = torch.full((Bn + 2, i.numel()), SENT)
    vals = (d * (zmax / torch.sqrt(c["zsq"]))[None, :])[i].t()
    Gy[:Bn] = q(torch.where(ok[None, :], vals, torch.zeros(())), dtype)
    if mutant != "clip_gy_zero_row_unwritten":
        Gy[Bn] = 0.0
    nparts = (Bn + 63) // 64
    part = torch.full((nparts + 1, Bm), SENT)
    for t in range(nparts):
        part[t] = (d * l)[:, t * 64:(t + 1) * 64].sum(1)
    if mutant == "clip_part_of_extra_block_written" and Bn % 64 == 0:
        part[nparts] = 0.0
    return Gy, part


def blocks_of(c):
    """the column blocks of the global batch in rank order: (col0, Bn) each, the last ragged"""
    return [(b, min(c["Bn"], c["Bm"] - b)) for b in range(0, c["Bm"], c["Bn"])]


def finish_case(c):
    """fp32 partials of every block stacked in rank order (the rounded float64 values), and the rows the finisher is asked for"""
    parts = []
    for b0, bn in blocks_of(c):
        l = c["Lg32"][:, b0:b0 + bn]
        D, _ = clip_D(c, l, c["row_lse"], c["col_lse_all"][b0:b0 + bn], b0)
        parts += [(D * l.double())[:, t * 64:(t + 1) * 64].sum(1) for t in range((bn + 63) // 64)]
    row0 = c["col0"] if c["col0"] > 0 else c["Bm"] // 2
    return torch.stack(parts).float(), row0, (c["Bn"] if c["col0"] > 0 else c["Bm"] - row0)


def check_clip_grad_y_finish(c, part32, row0, nrows, rscale_y, cscale_y):
    inv = c["inv_norm"]
    p = part32.double()[:, row0:row0 + nrows]
    ysq = c["ysq"].double()[row0:row0 + nrows]
    ref_r = inv * p.sum(0) / ysq
    tol_r = inv * (p.shape[0] * U32 * p.abs().sum(0)) / ysq + 3 * U32 * ref_r.abs() + ulp32(ref_r) + FTZ
    ref_c = inv * float(torch.exp(c["temp"].double())) / (math.sqrt(float(c["zsq_all"].double().max())) * torch.sqrt(ysq))
    return {"rscale_y": ratio(host(rscale_y), ref_r, tol_r), "cscale_y": ratio(host(cscale_y), ref_c, 2 * C_LOGIT * ref_c)}


def emul_clip_grad_y_finish(c, part32, row0, nrows, hw=0, mutant=None):
    r0 = 0 if mutant == "clip_finish_ignores_row0" else row0
    inv = torch.tensor(c["inv_norm"], dtype=F32)
    s = torch.zeros(nrows)
    for p in range(part32.shape[0]):
        s = s + part32[p, r0:r0 + nrows]
    ysq = c["ysq"][r0:r0 + nrows]
    return s * inv / ysq, inv * _exp(c["temp"], hw) / (torch.sqrt(c["zsq_all"].max()) * torch.sqrt(ysq))


# ---- clip_ranks
def ranks_ref(c):
    """cnt_i = #{j : l_ij > d_i or (l_ij == d_i and col0 + j < i)}, a plain loop over the fp32 values"""
    l, d = c["logits"].tolist(), c["diag"].tolist()
    return torch.tensor([sum(1 for j, v in enumerate(l[i]) if v > d[i] or (v == d[i] and c["col0"] + j < i)) for i in range(c["Bm"])],
                        dtype=torch.int32)


def emul_ranks(c, mutant=None):
    l, d = c["logits"], c["diag"][:, None]
    ii, jj = torch.arange(c["Bm"])[:, None], torch.arange(c["Bn"])[None, :]
    if mutant == "clip_tie_rule_gt_only":
        hit = l > d
    elif mutant == "clip_tie_rule_local_index":
        hit = (l > d) | ((l == d) & (jj < ii))
    else:
        hit = (l > d) | ((l == d) & (c["col0"] + jj < ii))
    return hit.float().sum(1).add(0.5).to(torch.int32)


# ---- clip_merge_rows
def merge_cases():
    """name -> [world][3][Bg] fp32 tables of (row max, row sum, positive's logit)"""
    g = _gen(77)
    world, Bg = 4, 300
    mx = torch.randn(world, Bg, generator=g) * 3 + 4
    sm = torch.rand(world, Bg, generator=g) * 60 + 1
    dg = torch.randn(world, Bg, generator=g)
    base = torch.stack([mx, sm, dg], 1)
    empty = base.clone()                     # one rank saw no mass at all for these rows: sum 0 at a very negative max
    empty[2, 0], empty[2, 1] = -3.0e38, 0.0
    same = base[:1].repeat(world, 1, 1)      # every rank equal: lse = max + log(world sum)
    return {"random": base, "a rank with row_sum 0 at row_max -3e38": empty, "all ranks equal": same}


def merge_ref(allp):
    a = allp.double()
    M = a[:, 0].amax(0)
    lse = M + torch.log((a[:, 1] * torch.exp(a[:, 0] - M)).sum(0))
    world = a.shape[0]
    tol = C_LSE * ulp32(torch.maximum(torch.maximum(lse.abs(), M.abs()), torch.ones_like(M))) + (world + 4) * U32
    d = a[:, 2].sum(0)
    return lse, tol, d, world * U32 * a[:, 2].abs().sum(0) + ulp32(d)


def check_merge(allp, lse, diag):
    rl, tl, rd, td = merge_ref(allp)
    return {"lse": ratio(host(lse), rl, tl), "diag": ratio(host(diag), rd, td)}


def emul_merge(allp, hw=0):
    M = allp[:, 0].amax(0)
    S, D = torch.zeros_like(M), torch.zeros_like(M)
    for r in range(allp.shape[0]):
        S = S + allp[r, 1] * _exp(allp[r, 0] - M, hw)
        D = D + allp[r, 2]
    return M + _log(S), D


# ---------------------------------------------------------------------------------------------------------------
# measuring the table
# ---------------------------------------------------------------------------------------------------------------
def measure_constants(sa_cases, clip_cases):
    """largest error of the emulations against float64 in units of each constant's magnitude, over the given cases and HW"""
    m = dict(C_SM=0.0, C_LOGIT=0.0, C_LSE=0.0, C_D=0.0)
    for case in sa_cases:
        a32 = sa_forward_ref(case, False)["a"].float()
        a = a32.double()
        W = torch.softmax(a, 1)
        mag = (a - a.amax(1, keepdim=True)).abs().clamp(min=1.0) * W
        keep = W >= FTZ
        for hw in HW:
            Wb, _ = emul_softmax_pack(a32, dict(case, mask=None), F32, hw)
            m["C_SM"] = max(m["C_SM"], float(((Wb[:case["D1"]].double() - W).abs()[keep] / mag[keep]).max()))
    for c in clip_cases:
        l32 = c["logits"].double()
        rl, cl = torch.logsumexp(l32, 1), torch.logsumexp(l32, 0)
        D, mag = clip_D(c)
        one, onec = torch.ones_like(rl), torch.ones_like(cl)
        mag_r = ulp32(torch.maximum(torch.maximum(rl.abs(), l32.amax(1).abs()), one))
        mag_c = ulp32(torch.maximum(torch.maximum(cl.abs(), l32.amax(0).abs()), onec))
        nz = c["l64"] != 0
        for hw in HW:
            l = emul_logits_stats(c, hw)[0]
            m["C_LOGIT"] = max(m["C_LOGIT"], float(((l.double() - c["l64"]).abs()[nz] / c["l64"].abs()[nz]).max()))
            m["C_LSE"] = max(m["C_LSE"], float(((emul_lse(c["logits"], 1, hw)[2].double() - rl).abs() / mag_r).max()),
                             float(((emul_lse(c["logits"], 0, hw)[2].double() - cl).abs() / mag_c).max()))
            d = emul_D(c["logits"], c["row_lse"], c["col_lse"], c["col0"], hw)
            m["C_D"] = max(m["C_D"], float(((d.double() - D).abs() / mag).max()))
    return m
