"""Inputs, float64 references, tolerances and plain-torch fp32 emulations for the kernel-level tests of csrc/sigmoid_loss.hip (the
pairwise sigmoid loss tail: sda_sigmoid_pairs, sda_sigmoid_finish, sda_sigmoid_grad_y), and the float64 autograd reference of the
whole loss.  tests/test_sigmoid_loss_cpu.py proves on the CPU that the cases reach their edges and catch the planted bugs;
tests/test_sigmoid_loss_gpu.py holds the HIP kernels to the same check_*() functions.  Nothing here needs a GPU.

A case is one of tests/sa_loss_cases.clip_case's blocks (its raw dot products S, squared norms and Gy layouts) with a temperature
and a bias of its own and, where labelled, tests/clip_label_cases.labels_of's speech labels.  The conventions are those files':
every kernel is handed exact fp32 inputs, its float64 reference is computed from those fp32 values, and no tolerance comes from a
kernel's output.  a = S e^temp / (sqrt ysq sqrt zsq) is the expression of clip_rows_kernel: its constant C_LOGIT is reused.  Two
quantities are new, measured like sa_loss_cases.measure_constants over every shape x regime x label pattern x mode below with
every exp and log1p result moved by -1, 0, +1 ulp, and held to 4 .. 5 x measured by
test_sigmoid_loss_cpu.py::test_tolerance_table_matches_the_emulation:

      constant   measured on the CPU   chosen     magnitude it multiplies
      C_SIGD     1.50                  6.5        ulp32(max(|l|, 1)) s (1 - s) + ulp32(D)       D = -z s, s = sigma(-z l), l = a + bias
      C_SP       2.50                  11         ulp32(max(|l|, 1)) s + ulp32(softplus)        softplus(-z l) = max(x, 0) + log1p(e^-|x|)

A kernel that forms l from its own fp32 a (sda_sigmoid_pairs) is given a's tolerance through the derivative besides:
s (1 - s) C_LOGIT |a| for D, s C_LOGIT |a| for the loss term.  Sums: n u sum|t_i| + the terms' tolerances + one ulp of the sum
(sum_tol); n = 19 for a column's 64-row partial (16 rows of one wave, 3 adds of the wave sums), 7 for a wave sum, the number of
partials for the finishing sums.  Stored values: one ulp of the storage type.
"""
import math

import torch

from tests.clip_label_cases import I32, LABEL_PATTERNS, LABEL_SHAPES, MODES, labels_of, store  # noqa: F401
from tests.sa_loss_cases import (C_LOGIT, CLIP_REGIMES, DTYPES, F32, F64, FTZ, GY_LAYOUT, HW, SENT, U32, _exp, clip_case,  # noqa: F401
                                 exact, gy_layout, host, pad64, q, ratio, sum_tol, ulp, ulp32)
from tests.elementwise_cases import _nudge

C_SIGD = 6.5
C_SP = 11.0

# (Bm, Bn, col0): one pair; one wave; one full 64 x 64 tile (the zero row of G alone in a tile row of its own); both sides of 256
# rows and of four tile rows; a ragged fifth; column blocks with col0 != 0 and their segmented Gy layouts
SHAPES = ((1, 1, 0), (3, 3, 0), (64, 64, 0), (255, 255, 0), (257, 257, 0), (300, 300, 0), (15, 5, 10), (140, 70, 70), (513, 70, 140))
# sa_loss_cases' regimes (their cosines and norms; `hot`: e^9, |l| in the thousands), the loss's own initial values, a positive bias
REGIMES = CLIP_REGIMES + ("init", "bias3")
_BASE = {"init": "trained", "bias3": "trained"}
_TEMP = {"init": math.log(10.0)}
_BIAS = {"flat": 0.0, "bias3": 3.0}


def sig_case(Bm, Bn, col0, regime, base=None):
    """clip_case's block (S with its padded pitch, ysq, zsq, zsq_all, inv_norm for the `mean` reduction) with this loss's temp
    and bias; a64 = the float64 scaled cosines from the fp32 inputs, a = their fp32 rounding (what sda_sigmoid_grad_y is handed)"""
    b = base if base is not None else clip_case(Bm, Bn, col0, _BASE.get(regime, regime))
    temp = torch.tensor([_TEMP[regime]], dtype=F32) if regime in _TEMP else b["temp"]
    bias = torch.tensor([_BIAS.get(regime, -10.0)], dtype=F32)
    S = b["S"][:, :Bn].double()
    a64 = S * torch.exp(temp.double()) / (torch.sqrt(b["ysq"].double())[:, None] * torch.sqrt(b["zsq"].double())[None, :])
    ii = torch.arange(Bm)
    pos = ii[:, None] == (col0 + torch.arange(Bn))[None, :]
    return dict(name=f"sigmoid Bm={Bm} Bn={Bn} col0={col0} {regime}", Bm=Bm, Bn=Bn, col0=col0, regime=regime, S=b["S"], ysq=b["ysq"],
                zsq=b["zsq"], zsq_all=b["zsq_all"], temp=temp, bias=bias, inv_norm=float(torch.tensor(1.0 / Bm, dtype=F32)), a64=a64,
                a=a64.float(), inb=b["inb"], pos=pos, labels=None, pattern=None, same=pos)


def labels_for(Bm, Bn, col0, pattern):
    """labels_of, with a pair planted inside the block where the pattern has put none there (`extremes` on a narrow block)"""
    lab = labels_of(Bm, Bn, col0, pattern).clone()
    same = (lab[:, None] == lab[None, col0:col0 + Bn])
    same[col0 + torch.arange(Bn), torch.arange(Bn)] = False
    if pattern != "distinct" and not bool(same.any()) and Bn >= 2:
        lab[col0 + Bn - 1] = lab[col0]
    return lab


def with_labels(c, pattern):
    lab = labels_for(c["Bm"], c["Bn"], c["col0"], pattern)
    return dict(c, name=f"{c['name']} labels={pattern}", labels=lab, pattern=pattern,
                same=lab[:, None] == lab[None, c["col0"]:c["col0"] + c["Bn"]])


def variants(c):
    """(case, mode) of every way a block is run: unlabelled, and each label pattern in both modes"""
    yield c, "positive"
    if (c["Bm"], c["Bn"], c["col0"]) in LABEL_SHAPES:
        for pattern in LABEL_PATTERNS:
            lc = with_labels(c, pattern)
            for mode in MODES:
                yield lc, mode


def signs(c, mode):
    """z of the block: +1, -1, 0 = dropped (int8)"""
    z = torch.where(c["pos"], 1, -1)
    if c["labels"] is not None:
        z = torch.where(c["same"] & ~c["pos"], 1 if mode == "positive" else 0, z)
    return z


# ---------------------------------------------------------------------------------------------------------------
# float64
# ---------------------------------------------------------------------------------------------------------------
def terms64(a, bias, z):
    """float64 (l, softplus(-z l), D, s, magnitude of C_SP, magnitude of C_SIGD) of a float64 a; dropped pairs: 0"""
    l = a + float(bias)
    x = -z.double() * l
    keep = z != 0
    zero = torch.zeros((), dtype=F64)
    s = torch.where(keep, torch.sigmoid(x), zero)
    # 1 - sigma(x) = sigma(-x), without the subtraction
    s1 = torch.where(keep, torch.sigmoid(-x), zero)
    sp = torch.where(keep, torch.clamp(x, min=0) + torch.log1p(torch.exp(-x.abs())), zero)
    D = -z.double() * s
    ul = ulp32(torch.maximum(l.abs(), torch.ones_like(l)))
    mag_sp = torch.where(keep, ul * s + ulp32(sp), zero)
    mag_D = torch.where(keep, ul * s * s1 + ulp32(D), zero)
    return dict(l=l, sp=sp, D=D, s=s, s1=s1, mag_sp=mag_sp, mag_D=mag_D, keep=keep)


def pairs_ref(c, mode, dtype):
    Bm, Bn, col0 = c["Bm"], c["Bn"], c["col0"]
    a = c["a64"]
    tol_a = C_LOGIT * a.abs() + FTZ
    t = terms64(a, c["bias"], signs(c, mode))
    tol_D = C_SIGD * t["mag_D"] + t["s"] * t["s1"] * tol_a + FTZ * t["keep"]
    tol_sp = C_SP * t["mag_sp"] + t["s"] * tol_a + FTZ * t["keep"]
    ysq = c["ysq"].double()
    f = (math.sqrt(float(ysq.max())) / torch.sqrt(ysq))[:, None]
    G = torch.zeros(Bm + 1, pad64(Bn), dtype=F64)
    G[:Bm, :Bn] = t["D"] * f
    tol_G = torch.ones_like(G)
    tol_G[:Bm, :Bn] = f * tol_D + 5 * U32 * G[:Bm, :Bn].abs() + ulp(G[:Bm, :Bn], dtype)
    ii = torch.arange(Bm)
    jj = (ii - col0).clamp(0, Bn - 1)
    Da = t["D"] * a
    tol_Da = tol_D * a.abs() + t["D"].abs() * tol_a + U32 * Da.abs()
    nparts = (Bm + 63) // 64
    part, tol_part = [], []
    for p in range(nparts):
        r = slice(p * 64, (p + 1) * 64)
        part.append(torch.stack([t["sp"][r].sum(0), Da[r].sum(0), t["D"][r].sum(0)], -1))
        tol_part.append(torch.stack([sum_tol(t["sp"][r], tol_sp[r] + U32 * t["sp"][r], 19), sum_tol(Da[r], tol_Da[r], 19),
                                     sum_tol(t["D"][r], tol_D[r], 19)], -1))
    return dict(a=a, tol_a=tol_a, D=t["D"], diag=torch.where(c["inb"], a[ii, jj], torch.zeros(Bm, dtype=F64)), tol_diag=tol_a[ii, jj],
                G=G, tol_G=tol_G, part=torch.stack(part), tol_part=torch.stack(tol_part), dropped=~t["keep"])


def check_pairs(c, mode, dtype, a_buf, diag_buf, G_buf, part_buf):
    """a_buf (Bm + 1, Bn) fp32, diag_buf (Bm + 1,) fp32, G_buf (Bm + 2, pad64(Bn)) of dtype, part_buf (nparts + 1, Bn, 3) fp32: the
    last row (element) of each is the sentinel the kernel must leave"""
    Bm, Bn = c["Bm"], c["Bn"]
    r = pairs_ref(c, mode, dtype)
    a, diag, G, part = host(a_buf), host(diag_buf), host(G_buf).float(), host(part_buf)
    inb = c["inb"]
    pad = torch.ones(Bm + 1, G.shape[1], dtype=torch.bool)
    pad[:Bm, :Bn] = False
    nparts = r["part"].shape[0]
    return {"a": ratio(a[:Bm], r["a"], r["tol_a"]), "diag": ratio(diag[:Bm][inb], r["diag"][inb], r["tol_diag"][inb]),
            "diag equals a's entry": exact(torch.equal(diag[:Bm][inb], a[:Bm][torch.arange(Bm)[inb], torch.arange(Bm)[inb] - c["col0"]])),
            "diag exactly zero outside the block": exact((diag[:Bm][~inb] == 0).all()),
            "G": ratio(G[:Bm + 1], r["G"], r["tol_G"]), "G zero row and pad columns exactly zero": exact((G[:Bm + 1][pad] == 0).all()),
            "G of a dropped pair exactly zero": exact((G[:Bm, :Bn][r["dropped"]] == 0).all()),
            "part": ratio(part[:nparts], r["part"], r["tol_part"]),
            "past the outputs untouched": exact(bool((a[Bm:] == SENT).all()) and bool((diag[Bm:] == SENT).all())
                                                and bool((G[Bm + 1:] == SENT).all()) and bool((part[nparts:] == SENT).all()))}


def finish_ref(c, part32):
    """from the fp32 partials the finisher is handed"""
    inv = c["inv_norm"]
    p = part32.double()
    n = p.shape[0]
    col, tol_col = p.sum(0), n * U32 * p.abs().sum(0)                       # (Bn, 3)
    zsq, ysq = c["zsq"].double(), c["ysq"].double()
    rscale = inv * col[:, 1] / zsq
    cscale = inv * float(torch.exp(c["temp"].double())) / (math.sqrt(float(ysq.max())) * torch.sqrt(zsq))
    scal = inv * col.sum(0)
    return dict(rscale=rscale, tol_rscale=inv * tol_col[:, 1] / zsq + 3 * U32 * rscale.abs() + ulp32(rscale) + FTZ, cscale=cscale,
                tol_cscale=2 * C_LOGIT * cscale, scalars=scal, tol_scalars=inv * tol_col.sum(0) + ulp32(scal) + FTZ)


def check_finish(c, part32, rscale_buf, cscale_buf, scalars_buf):
    """rscale_buf, cscale_buf (Bn + 1,), scalars_buf (4,): the last element of each the sentinel"""
    Bn = c["Bn"]
    r = finish_ref(c, part32)
    rs, cs, sc = host(rscale_buf), host(cscale_buf), host(scalars_buf)
    return {"rscale": ratio(rs[:Bn], r["rscale"], r["tol_rscale"]), "cscale": ratio(cs[:Bn], r["cscale"], r["tol_cscale"]),
            "scalars[0] loss": ratio(sc[0], r["scalars"][0], r["tol_scalars"][0]),
            "scalars[1] dtemp": ratio(sc[1], r["scalars"][1], r["tol_scalars"][1]),
            "scalars[2] dbias": ratio(sc[2], r["scalars"][2], r["tol_scalars"][2]),
            "past the outputs untouched": exact(float(rs[Bn]) == SENT and float(cs[Bn]) == SENT and float(sc[3]) == SENT)}


def gy_rows(c):
    """for every column of Gy: the speech row it holds and whether it holds one"""
    seg, seg_pitch, groups = gy_layout(c["Bm"], c["Bn"], c["col0"])
    cc = torch.arange(groups * seg_pitch)
    o = cc % seg_pitch
    i = (cc // seg_pitch) * seg + o
    return i.clamp(max=c["Bm"] - 1), (o < seg) & (i < c["Bm"])


def grad_y_ref(c, mode, dtype):
    """from the fp32 a the kernel is handed"""
    Bn = c["Bn"]
    a = c["a"].double()
    t = terms64(a, c["bias"], signs(c, mode))
    tol_D = C_SIGD * t["mag_D"] + FTZ * t["keep"]
    fz = (math.sqrt(float(c["zsq_all"].double().max())) / torch.sqrt(c["zsq"].double()))[None, :]
    i, ok = gy_rows(c)
    zero = torch.zeros((), dtype=F64)
    Gy = torch.zeros(Bn + 1, i.numel(), dtype=F64)
    Gy[:Bn] = torch.where(ok[None, :], (t["D"] * fz)[i].t(), zero)
    tol = torch.ones_like(Gy)
    tol[:Bn] = torch.where(ok[None, :], (tol_D * fz)[i].t(), torch.ones((), dtype=F64)) + 5 * U32 * Gy[:Bn].abs() + ulp(Gy[:Bn], dtype)
    Da = t["D"] * a
    nparts = (Bn + 63) // 64
    part = torch.stack([Da[:, p * 64:(p + 1) * 64].sum(1) for p in range(nparts)])
    tol_part = torch.stack([sum_tol(Da[:, p * 64:(p + 1) * 64], (tol_D * a.abs() + U32 * Da.abs())[:, p * 64:(p + 1) * 64], 7, dim=1)
                            for p in range(nparts)])
    return dict(Gy=Gy, tol_Gy=tol, ok=ok, i=i, part=part, tol_part=tol_part, dropped=~t["keep"])


def check_grad_y(c, mode, dtype, Gy_buf, part_buf):
    """Gy_buf: (Bn + 2, groups * seg_pitch) of dtype, last row sentinel; part_buf: (nparts + 1, Bm) fp32, last row sentinel"""
    Bn = c["Bn"]
    r = grad_y_ref(c, mode, dtype)
    Gy, part = host(Gy_buf).float(), host(part_buf)
    nparts = r["part"].shape[0]
    rep = r["dropped"][r["i"]].t() & r["ok"][None, :]                        # [j][column of Gy]
    return {"Gy": ratio(Gy[:Bn + 1], r["Gy"], r["tol_Gy"]), "Gy zero row exactly zero": exact((Gy[Bn] == 0).all()),
            "Gy columns without a row exactly zero": exact((Gy[:Bn][:, ~r["ok"]] == 0).all()),
            "Gy past row Bn untouched": exact((Gy[Bn + 1:] == SENT).all()),
            "Gy of a dropped pair exactly zero": exact((Gy[:Bn][rep] == 0).all()),
            "part": ratio(part[:nparts], r["part"], r["tol_part"]), "part past its rows untouched": exact((part[nparts:] == SENT).all())}


# ---------------------------------------------------------------------------------------------------------------
# fp32 emulation of the kernels, in their summation order
# ---------------------------------------------------------------------------------------------------------------
def _log1p(x, hw=0):
    return _nudge(torch.log1p(x.double()).float(), hw)


def emul_terms(a, bias, z, hw=0, mutant=None):
    """fp32 (softplus, D) of softplus_sigmoid() on x = -z (a + bias); dropped pairs selected to zero"""
    l = a if mutant == "bias_left_out" else a + bias
    zf = z.float()
    x = torch.where(z > 0, -l, l)
    zero = torch.zeros(())
    if mutant == "one_minus_sigma":
        s = 1.0 / (1.0 + _exp(-l, hw))                       # sigma(l); a positive's sigma(-l) as 1 - sigma(l)
        sg = torch.where(z > 0, 1.0 - s, s)
    else:
        t = _exp(-x.abs(), hw)
        r = 1.0 / (1.0 + t)
        sg = torch.where(x >= 0, r, t * r)
    if mutant == "naive_log1pexp":
        sp = torch.log(1.0 + _exp(x, hw))
    else:
        sp = torch.clamp(x, min=0.0) + _log1p(_exp(-x.abs(), hw), hw)
    sp = torch.where(x != x, x, sp)                          # (clamp drops a NaN the device's select keeps in the sum)
    d = -zf * sg
    if mutant == "masked_times_zero":
        return sp * (z != 0).float(), d                      # d = -0 * sg
    return torch.where(z != 0, sp, zero), torch.where(z != 0, d, zero)


NONFINITE_MUTANTS = ("masked_times_zero", "saturating_store", "colsum_skips_nonfinite")      # (tests/test_nonfinite_cpu.py)


def _sum_terms(t, mutant=None):
    """the terms of a partial sum.  mutant colsum_skips_nonfinite: `isfinite(t) ? t : 0`"""
    return torch.where(torch.isfinite(t), t, torch.zeros(())) if mutant == "colsum_skips_nonfinite" else t


def _tile_colsum(v):
    """(rows <= 64, Bn) -> (Bn,): wave w adds rows w, w + 4, ... in order; the four wave sums are added in wave order"""
    n, Bn = v.shape
    full = torch.zeros(64, Bn)
    full[:n] = v
    waves = full.reshape(16, 4, Bn)
    acc = torch.zeros(4, Bn)
    for k in range(16):
        acc = acc + waves[k]
    return ((acc[0] + acc[1]) + acc[2]) + acc[3]


def emul_pairs(c, mode, dtype, hw=0, mutant=None):
    """sigmoid_pairs_kernel: the four buffers check_pairs() takes"""
    Bm, Bn, col0 = c["Bm"], c["Bn"], c["col0"]
    ri = _exp(c["temp"], hw) / torch.sqrt(c["ysq"])
    a = c["S"][:, :Bn] * ri[:, None] / torch.sqrt(c["zsq"])[None, :]
    z = signs(c, mode)
    if mutant == "same_label_as_negative":
        z = torch.where(c["pos"], 1, -1)
    sp, d = emul_terms(a, c["bias"], z, hw, mutant)
    ysq = c["ysq"][col0:col0 + Bn] if mutant == "ymax_local_rows" else c["ysq"]
    if mutant == "fmaxf_ymax":
        ymax = torch.sqrt(torch.where(ysq != ysq, torch.zeros(()), ysq).max())
    else:
        ymax = torch.sqrt(ysq.max()) if not bool((ysq != ysq).any()) else torch.tensor(math.nan)
    G = torch.full((Bm + 2, pad64(Bn)), SENT)
    G[:Bm + 1] = 0.0
    g = d * (ymax / torch.sqrt(c["ysq"]))[:, None]
    G[:Bm, :Bn] = store(g if mutant == "masked_times_zero" else torch.where(z != 0, g, torch.zeros(())), dtype, mutant)
    if mutant == "zero_row_unwritten":
        G[Bm] = SENT
    if mutant == "pad_column_unwritten" and pad64(Bn) > Bn:
        G[:Bm, Bn:] = SENT
    a_buf = torch.full((Bm + 1, Bn), SENT)
    a_buf[:Bm] = a
    ii = torch.arange(Bm)
    diag = torch.full((Bm + 1,), SENT)
    if mutant == "diag_without_col0":
        diag[:Bm] = torch.where(ii < Bn, a[ii, ii.clamp(max=Bn - 1)], torch.zeros(Bm))
    else:
        diag[:Bm] = torch.where(c["inb"], a[ii, (ii - col0).clamp(0, Bn - 1)], torch.zeros(Bm))
    nparts = (Bm + 63) // 64
    part = torch.full((nparts + 1, Bn, 3), SENT)
    da = d * ((a + c["bias"]) if mutant == "sum_Dl_not_Da" else a)
    if mutant != "masked_times_zero":
        da = torch.where(z != 0, da, torch.zeros(()))        # (a dropped pair's a never enters a sum)
    sp, da, d = _sum_terms(sp, mutant), _sum_terms(da, mutant), _sum_terms(d, mutant)
    for p in range(nparts):
        r = slice(p * 64, (p + 1) * 64)
        part[p] = torch.stack([_tile_colsum(sp[r]), _tile_colsum(da[r]), _tile_colsum(d[r])], -1)
    return a_buf, diag, G, part


def emul_finish(c, part32, hw=0, mutant=None):
    """sigmoid_finish_kernel: (rscale, cscale, scalars) with one sentinel behind each"""
    Bn = c["Bn"]
    inv = torch.tensor(c["inv_norm"] / 2 if mutant == "inv_norm_2B" else c["inv_norm"], dtype=F32)
    col = torch.zeros(Bn, 3)
    for p in range(part32.shape[0]):
        col = col + part32[p]
    ymax = torch.sqrt(c["ysq"].max())
    rs, cs, sc = torch.full((Bn + 1,), SENT), torch.full((Bn + 1,), SENT), torch.full((4,), SENT)
    rs[:Bn] = col[:, 1] * inv / c["zsq"]
    cs[:Bn] = inv * _exp(c["temp"], hw) / (ymax * torch.sqrt(c["zsq"]))
    tot = col.double().sum(0)
    sc[:3] = (tot * float(inv)).float()
    if mutant == "dbias_without_inv_norm":
        sc[2] = tot[2].float()
    return rs, cs, sc


def emul_grad_y(c, mode, dtype, hw=0, mutant=None):
    """sigmoid_grad_y_kernel on the fp32 a: (Gy, part) with their sentinel rows"""
    Bm, Bn = c["Bm"], c["Bn"]
    a = c["a"]
    z = signs(c, mode)
    if mutant == "same_label_as_negative":
        z = torch.where(c["pos"], 1, -1)
    _, d = emul_terms(a, c["bias"], z, hw, mutant)
    zmax = torch.sqrt(c["zsq_all"].max())
    i, ok = gy_rows(c)
    Gy = torch.full((Bn + 2, i.numel()), SENT)
    g = d * (zmax / torch.sqrt(c["zsq"]))[None, :]
    # (a dropped pair's coefficient is selected, never 0 * zmax / |Z_j|: a non-finite norm stays out of it)
    vals = (g if mutant == "masked_times_zero" else torch.where(z != 0, g, torch.zeros(())))[i].t()
    Gy[:Bn] = store(torch.where(ok[None, :], vals, torch.zeros(())), dtype, mutant)
    Gy[Bn] = 0.0
    if mutant == "zero_row_unwritten":
        Gy[Bn] = SENT
    if mutant == "pad_column_unwritten" and not bool(ok.all()):
        Gy[:Bn][:, ~ok] = SENT
    nparts = (Bn + 63) // 64
    part = torch.full((nparts + 1, Bm), SENT)
    da = d * ((a + c["bias"]) if mutant == "sum_Dl_not_Da" else a)
    if mutant != "masked_times_zero":
        da = torch.where(z != 0, da, torch.zeros(()))        # (a dropped pair's a never enters a sum)
    da = _sum_terms(da, mutant)
    for p in range(nparts):
        part[p] = da[:, p * 64:(p + 1) * 64].sum(1)
    return Gy, part


# ---------------------------------------------------------------------------------------------------------------
# non-finite inputs
# ---------------------------------------------------------------------------------------------------------------
def poison_at(c):
    """(i, j) of a negative pair of the block (Bm >= 2)"""
    j = c["Bn"] // 2
    i = c["col0"] + j + 1
    return (i if i < c["Bm"] else c["col0"] + j - 1), j


def poisoned(c, where, value):
    """the case with one element of S (a negative pair's), of ysq or the bias replaced by NaN or inf, a64 and a derived again"""
    d = dict(c)
    i, j = poison_at(c)
    if where == "S":
        d["S"] = c["S"].clone()
        d["S"][i, j] = value
    elif where == "ysq":
        d["ysq"] = c["ysq"].clone()
        d["ysq"][i] = value
    elif where == "bias":
        d["bias"] = torch.tensor([value], dtype=F32)
    else:
        raise KeyError(where)
    Bn = c["Bn"]
    d["a64"] = d["S"][:, :Bn].double() * torch.exp(d["temp"].double()) / (torch.sqrt(d["ysq"].double())[:, None] *
                                                                        torch.sqrt(d["zsq"].double())[None, :])
    d["a"] = d["a64"].float()
    d["name"] = f"{c['name']} {where}={value}"
    return d


def check_nonfinite(c, p, where, mode, dtype, G_buf, scalars_buf, G_clean):
    """p = poisoned(c, where, value), run through pairs and finish: whatever the float64 formulas make non-finite on the poisoned
    inputs is non-finite in G and in the three scalars, nothing else is, and (one element of S poisoned) every other entry of G
    keeps the bits of the clean run"""
    Bm, Bn = c["Bm"], c["Bn"]
    r = pairs_ref(p, mode, dtype)
    G, Gc, sc = host(G_buf).float()[:Bm, :Bn], host(G_clean).float()[:Bm, :Bn], host(scalars_buf)[:3]
    want = r["part"].sum((0, 1))
    out = {"G non-finite exactly where the formulas say": exact(torch.equal(torch.isfinite(G), torch.isfinite(r["G"][:Bm, :Bn]))),
           "loss, dtemp, dbias non-finite exactly where the formulas say": exact(torch.equal(torch.isfinite(sc), torch.isfinite(want)))}
    if where == "S":
        other = torch.ones(Bm, Bn, dtype=torch.bool)
        other[poison_at(c)] = False
        out["every other entry of G keeps the clean run's bits"] = exact(torch.equal(G[other], Gc[other]))
    return out


def dropped_pair_case(c):
    """a mask-mode labelled case with a NaN planted in S at a dropped pair -> (case, (i, j)); None where no pair is dropped"""
    idx = (c["same"] & ~c["pos"]).nonzero()
    if c["labels"] is None or idx.numel() == 0:
        return None
    i, j = (int(v) for v in idx[0])
    d = dict(c, S=c["S"].clone())
    d["S"][i, j] = math.nan
    return d, (i, j)


def check_dropped_nan(ij, G_buf, part_buf, G_clean, part_clean):
    """a dropped pair is left out, not multiplied by zero: a NaN there reaches neither G nor any sum"""
    G, Gc = host(G_buf).float(), host(G_clean).float()
    return {"G of the dropped NaN pair exactly zero": exact(float(G[ij]) == 0.0),
            "G elsewhere keeps the clean run's bits": exact(torch.equal(G, Gc)),
            "the sums keep the clean run's bits": exact(torch.equal(host(part_buf), host(part_clean)))}


# ---------------------------------------------------------------------------------------------------------------
# the whole loss in float64
# ---------------------------------------------------------------------------------------------------------------
def loss_ref(l, labels, mode, reduction="mean"):
    """The pairwise sigmoid loss of a float64 logits matrix l (speech rows x brain columns of the whole batch), in its autograd
    form: softplus(-z l) summed over the pairs that take part, over B for the mean"""
    B = l.shape[0]
    eye = torch.eye(B, dtype=torch.bool)
    z = torch.where(eye, 1.0, -1.0).double()
    keep = torch.ones(B, B, dtype=torch.bool)
    if labels is not None:
        same = labels[:, None] == labels[None, :]
        if mode == "positive":
            z = torch.where(same, 1.0, -1.0).double()
        else:
            keep = ~same | eye
    terms = -torch.nn.functional.logsigmoid(z * l)              # softplus(-z l), in the form whose backward stays finite at |l| > 709
    total = torch.where(keep, terms, torch.zeros((), dtype=F64)).sum()
    return total / B if reduction == "mean" else total


def loss_ref_embeddings(x, y, temp, bias, labels, mode, reduction="mean"):
    """float64 autograd on embeddings x (speech), y (brain), (B, F, T): (loss, dx, dy, dtemp, dbias, logits, sum|D a|, sum|D|)"""
    x = x.detach().double().cpu().requires_grad_(True)
    y = y.detach().double().cpu().requires_grad_(True)
    t = torch.tensor([float(temp)], dtype=F64, requires_grad=True)
    b = torch.tensor([float(bias)], dtype=F64, requires_grad=True)
    B = x.shape[0]
    X, Y = x.reshape(B, -1), y.reshape(B, -1)
    a = (X / X.norm(dim=1, keepdim=True)) @ (Y / Y.norm(dim=1, keepdim=True)).T * torch.exp(t)
    lg = a + b
    lg.retain_grad()
    lab = None if labels is None else torch.as_tensor(labels).cpu().to(torch.int64)
    loss = loss_ref(lg, lab, mode, reduction)
    loss.backward()
    D = lg.grad
    return dict(loss=loss.detach(), dx=x.grad, dy=y.grad, dtemp=t.grad, dbias=b.grad, logits=lg.detach(),
                abs_Da=float((D * a.detach()).abs().sum()), abs_D=float(D.abs().sum()))


# ---------------------------------------------------------------------------------------------------------------
# measuring the table
# ---------------------------------------------------------------------------------------------------------------
def measure_constants(cases):
    """largest error of emul_terms against float64 in units of each constant's magnitude, over the (case, mode) given and HW"""
    m = dict(C_SIGD=0.0, C_SP=0.0)
    for c, mode in cases:
        z = signs(c, mode)
        t = terms64(c["a"].double(), c["bias"], z)
        k = t["keep"]
        if not bool(k.any()):
            continue
        for hw in HW:
            sp, d = emul_terms(c["a"], c["bias"], z, hw)
            m["C_SIGD"] = max(m["C_SIGD"], float(((d.double() - t["D"]).abs()[k] / t["mag_D"][k]).max()))
            m["C_SP"] = max(m["C_SP"], float(((sp.double() - t["sp"]).abs()[k] / t["mag_sp"][k]).max()))
    return m
