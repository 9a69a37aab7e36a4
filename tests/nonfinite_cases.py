"""Poison values, named poison positions, the two checks and plain-torch restatements (with seeded mutants) for the tests
of inf / NaN propagation through the backward kernels (tests/test_nonfinite_cpu.py proves on the CPU that the checks catch
the four ways a kernel swallows or leaks a non-finite value; tests/test_nonfinite_gpu.py and tests/test_nonfinite_losses_gpu.py
hold the HIP kernels to the same checks; tests/test_overflow_guard_gpu.py runs the fp16 overflow guard that depends on them).
Nothing here needs a GPU.

Why: fp16 training rests on one property.  When an activation gradient overflows, the inf or NaN must reach at least one
parameter gradient, or LossScaler.unscale_(check=True) never sees it and Adam is fed a wrong, finite gradient.

A case = the operands of an existing small case + one poison value at one named position of one operand.  The reference is
the restatement the kernel's own test uses (torch on the CPU: IEEE semantics) evaluated on the poisoned operands, and ONLY its
isfinite mask is used: inf is never compared with NaN, nor signs (0 * inf, inf - inf and reordered sums differ legitimately).

  propagation   every element the reference makes non-finite is non-finite in the kernel's output — the by-products the training
                step consumes included (column sums, statistics partials, row sums of squares, rscale / cscale, colpart);
  containment   every element the reference leaves finite is finite in the kernel's output, AND where the reference does not
                depend on the poisoned element at all (its value on the poisoned operands equals its value on the clean ones)
                the output carries the bits of the same call on the unpoisoned operands.  (A finite element that does depend
                on the poison — the rest of a soft-max row that holds a -inf, anything a finite 1e5 enters in fp32 — owes
                finiteness only: its value is the business of the kernel's own accuracy test.)

Where the maths couples everything (training-mode BatchNorm within a channel, the soft-max normalisers) the reference's mask
says so, and containment has nothing left to hold there.

EXCEPTIONS lists the kernels in which a leak is a deliberate trade, with the reason and the exact extent of the waiver;
propagation still holds for them in full."""
import math

import torch

INF, NAN = math.inf, math.nan
POISONS = {"+inf": INF, "-inf": -INF, "nan": NAN}
# a finite fp32 value above the storage type's largest finite one (65504 / 3.3895e38): a store must make it inf, never the
# largest finite value.  3.4e38 lies above the midpoint 3.3961e38 between bf16's largest value and 2^128.
OVERFLOW = {torch.float16: 1e5, torch.bfloat16: 3.4e38}


PAD = ", pad channels"


def _pad_channels(name, refs):
    """The tests hand the pad channels of a data-gradient conv's outputs over as outputs of their own, named "<output>, pad
    channels"; every other output gets no waiver.  Pad channels of a (B, C, T) output: only in the frames (b, t) whose REAL
    channels hold a non-finite element in the reference.  Pad channels of per-channel sums: all (they add up the frames' pad
    channels, and nothing reads them: a bias or BatchNorm gradient has C entries)."""
    bad = ~torch.isfinite(refs[name])
    if not name.endswith(PAD):
        return torch.zeros_like(bad)
    if bad.dim() != 3:
        return torch.ones_like(bad)
    real = ~torch.isfinite(refs[name[:-len(PAD)]])
    return real.any(dim=1, keepdim=True).expand_as(bad)


def _every_tap(name, refs):
    """(..., Cout, Cin, KS) mask -> every tap of a weight (co, ci) that holds a non-finite tap"""
    bad = ~torch.isfinite(refs[name])
    return bad.any(dim=-1, keepdim=True).expand_as(bad) if bad.dim() >= 3 else torch.zeros_like(bad)


PAD_COLS = ", pad columns"


def _pad_columns(name, refs):
    """The tests hand the columns N ... pad64(N) - 1 of a similarity product over as an output of their own, named "<output>, pad
    columns": waived in the rows i in which the LAST real column of the same output is non-finite, and nowhere else."""
    bad = ~torch.isfinite(refs[name])
    if not name.endswith(PAD_COLS):
        return torch.zeros_like(bad)
    real = ~torch.isfinite(refs[name[:-len(PAD_COLS)]])
    return real[:, -1:].expand_as(bad)


# kernel -> (reason, widen): the deliberate trades.  The first two kernels mask by a zero operand instead of a select (0 * inf = NaN), which
# the maths does not do; `widen` maps an output's name and the references of all outputs to the elements that may come out
# non-finite although the reference leaves them finite.  It is as narrow as the kernel's construction allows: propagation is unchanged, containment (finiteness and
# the clean run's bits) holds for every element outside the widened mask, and inside it for every element the kernel does
# leave finite.
EXCEPTIONS = {
    "conv_gemm (data gradient)": (
        "the PAD channels of dx (Cin..Cin_p) are products of the packed weight's zero columns: a frame whose real channels are "
        "non-finite (every one is: each weight column meets the poisoned dy) has NaN in its pad channels too.  The next conv "
        "multiplies them with zero weight columns again, so they only reach frames that are non-finite already, and the weight "
        "gradient's pad columns are dropped by the unpack.  No other frame, no other sample and NO REAL CHANNEL is waived: not for "
        "a poisoned dy, and not for a poisoned saved operand of an epilogue, which the maths lets reach one element only.",
        _pad_channels),
    "wgrad_gemm": (
        "a tap that reads x past the end of its sample is masked by dy's all-zero row, not by a select: x[b, ci, T - 1] = inf makes "
        "g[:, ci, tap 0] NaN although only taps 1 and 2 read that frame.  The leak stays inside weights (co, ci) of the same segment "
        "whose other taps are non-finite by the maths: the same parameter tensor fails the finiteness check either way, and a "
        "skipped step reads none of it.  A select in the K loop would sit on the MFMA operand path of the step's largest GEMMs.",
        _every_tap),
    "sim_gemm": (
        "the columns N ... pad64(N) - 1 of S are stored although nobody reads them, and a tile row past N is fed the LAST candidate's "
        "row (sim_gemm) or window (sim_gemm_windows) by the clamp on the LDS-DMA offsets: S[i][N ...] repeats S[i][N - 1], and is "
        "non-finite exactly where that is.  Waived: pad columns, in the rows whose last real column is non-finite by the maths.  No "
        "real column, no other row, and no pad column of a row whose last real column is finite.  Zeroing them would be a select on "
        "the store of the similarity GEMM of every step for the sake of elements without a reader.",
        _pad_columns),
}


def poisons(dtype=None):
    """name -> value; with a 16-bit `dtype` also the finite fp32 value that overflows it (for operands held in fp32)"""
    out = dict(POISONS)
    if dtype in OVERFLOW:
        out[f"{OVERFLOW[dtype]:g}"] = OVERFLOW[dtype]
    return out


# ---------------------------------------------------------------------------------------------------------------
# positions
# ---------------------------------------------------------------------------------------------------------------
def row_positions(B, T, t_edges=(), flat_edges=(), row_pad=16):
    """name -> (b, t).  t_edges: tile boundaries inside a sample (rows t - 1 and t of the middle sample); flat_edges: boundaries
    in memory rows of the row layout (sample b starts at b (T + row_pad) + row_pad), taken where both neighbours are valid rows."""
    out = {"first row of the first sample": (0, 0), "last row of the last sample": (B - 1, T - 1)}
    for e in t_edges:
        if 0 < e < T:
            out[f"row {e - 1}, below the boundary at {e}"] = (B // 2, e - 1)
            out[f"row {e}, above the boundary at {e}"] = (B // 2, e)
    Tp = T + row_pad
    for e in flat_edges:
        for m, side in ((e - 1, "below"), (e, "above")):
            b, t = divmod(m, Tp)
            if b < B and t >= row_pad:
                out[f"memory row {m}, {side} the boundary at {e}"] = (b, t - row_pad)
    return out


def channel_positions(C):
    """name -> c: channel 0 and the last real channel (next to the pad channels).  (A GLU's two halves are separate saved
    operands — value / out and gate — and the tests poison each once.)"""
    return {"channel 0": 0, f"channel {C - 1}, the last real one": C - 1}


def positions(B, T, C, t_edges=(), flat_edges=()):
    """name -> (b, t, c): every named row and every named channel at least once (rows and channels paired up in turn, not
    multiplied out: a kernel's row path and channel path are independent)"""
    rows, chans = row_positions(B, T, t_edges, flat_edges), channel_positions(C)
    rn, cn = list(rows), list(chans)
    out = {}
    for i in range(max(len(rn), len(cn))):
        r, c = rn[i % len(rn)], cn[i % len(cn)]
        out[f"{r}, {c}"] = rows[r] + (chans[c],)
    return out


def split_pad(label, t, C, dim=1, pad=PAD):
    """an output with padded channels along `dim` -> {label: the real channels, label + pad: the pad channels} (nothing when
    there are none)"""
    n = t.shape[dim]
    out = {label: t.narrow(dim, 0, C).contiguous()}
    if n > C:
        out[label + pad] = t.narrow(dim, C, n - C).contiguous()
    return out


def poisoned(t, index, value):
    """a copy of t with `value` at `index`"""
    out = t.clone()
    out[index] = value
    return out


# ---------------------------------------------------------------------------------------------------------------
# the two checks
# ---------------------------------------------------------------------------------------------------------------
def stored(ref, dtype):
    """the reference as the kernel stores it: through fp32 (the accumulator) into `dtype` (None: fp32), round to nearest even —
    a finite value beyond the type's range becomes inf"""
    out = ref.float()
    return out if dtype in (None, torch.float32) else out.to(dtype)


def _bits(t):
    t = t.contiguous()
    return t.view({1: torch.int8, 2: torch.int16, 4: torch.int32, 8: torch.int64}[t.element_size()])


def _first(mask):
    return tuple(int(i) for i in mask.nonzero()[0])


def check(ref, got, clean, ref_clean, allowed=None, independent=None):
    """ref: the restatement on the poisoned operands (any float dtype, as stored()), got: the output under test on the same
    operands, clean: the same call on the unpoisoned operands, ref_clean: the restatement on the unpoisoned operands.
    allowed (EXCEPTIONS): mask of the elements that may be non-finite although the reference is finite there.
    independent: mask of the elements the poisoned element does not enter at all (run_cases, structural=True); without it an
    element counts as independent where the reference's value did not move.
    Returns {check name: message} of the failed checks."""
    ref, got, clean, ref_clean = ref.detach().cpu(), got.detach().cpu(), clean.detach().cpu(), ref_clean.detach().cpu()
    assert ref.shape == got.shape == clean.shape == ref_clean.shape, (ref.shape, got.shape, clean.shape, ref_clean.shape)
    bad_ref, bad_got = ~torch.isfinite(ref), ~torch.isfinite(got)
    out = {}
    swallowed = bad_ref & ~bad_got
    if bool(swallowed.any()):
        i = _first(swallowed)
        out["propagation"] = (f"{int(swallowed.sum())} of {int(bad_ref.sum())} non-finite elements came out finite, first at {i}: "
                              f"reference {float(ref[i])}, got {float(got[i])}")
    leaked = ~bad_ref & bad_got
    if allowed is not None:
        assert allowed.shape == ref.shape
        leaked = leaked & ~allowed
    same = ref == ref_clean
    if independent is not None:
        same = same & independent.cpu()
    changed = ~bad_ref & ~bad_got & same & (_bits(got) != _bits(clean))
    if bool(leaked.any()):
        i = _first(leaked)
        out["containment"] = (f"{int(leaked.sum())} of {int((~bad_ref).sum())} finite elements came out non-finite, first at {i}: "
                              f"reference {float(ref[i])}, got {float(got[i])}")
    elif bool(changed.any()):
        i = _first(changed)
        out["containment"] = (f"{int(changed.sum())} finite elements changed their bits, first at {i}: "
                              f"got {float(got[i])!r}, on the unpoisoned operands {float(clean[i])!r}")
    return out


def check_all(kernel, refs, gots, cleans, refs_clean, what="", independent=None):
    """dicts output name -> tensor; asserts both checks on every output (a kernel listed in EXCEPTIONS: with its widened mask)"""
    assert set(refs) == set(gots) == set(cleans) == set(refs_clean), (kernel, sorted(refs), sorted(gots), sorted(cleans))
    failed = {}
    for name in refs:
        allowed = EXCEPTIONS[kernel][1](name, refs) if kernel in EXCEPTIONS else None
        res = check(refs[name], gots[name], cleans[name], refs_clean[name], allowed, None if independent is None else independent[name])
        for k, msg in res.items():
            failed[f"{name}: {k}"] = msg
    assert not failed, f"{kernel} {what}: " + "; ".join(f"{k}: {v}" for k, v in failed.items())


# ---------------------------------------------------------------------------------------------------------------
# restatements of the four constructs, each with the mutant that swallows or leaks
# ---------------------------------------------------------------------------------------------------------------
MUTANTS = ("softmax_skips_nan", "saturating_store", "mask_by_multiply", "colsum_skips_nonfinite")


def softmax_rows(a, mutant=None):
    """soft-max of every row with the maximum subtracted.  mutant: the maximum and the normaliser skip NaN (what fmaxf does with
    a NaN operand) and the result is selected to 0 where the input was NaN"""
    if mutant == "softmax_skips_nan":
        nan = torch.isnan(a)
        mx = torch.where(nan, torch.full_like(a, -INF), a).amax(1, keepdim=True)
        e = torch.where(nan, torch.zeros_like(a), torch.exp(a - mx))
        return torch.where(nan, torch.zeros_like(a), e / e.sum(1, keepdim=True))
    e = torch.exp(a - a.amax(1, keepdim=True))
    return e / e.sum(1, keepdim=True)


def store16(v, dtype, mutant=None):
    """an fp32 value into 16-bit storage, round to nearest even.  mutant: a saturating convert (NaN stays NaN)"""
    v = v.float()
    if mutant == "saturating_store":
        big = torch.finfo(dtype).max
        v = torch.where(torch.isnan(v), v, v.clamp(-big, big))
    return v.to(dtype)


def conv3_rows(x, w, B, T, dil, mutant=None):
    """kernel-size-3 "same" convolution of the valid rows x (B T, C) with taps w (3, C, C): a tap that falls outside its sample
    reads zero.  The restatement selects; the mutant reads whatever row lies there and multiplies it with a 0 mask."""
    rows = torch.arange(B * T)
    out = torch.zeros(B * T, w.shape[1], dtype=x.dtype)
    for k in range(3):
        src = rows + (k - 1) * dil
        inside = (src >= 0) & (src < B * T) & (src.clamp(0, B * T - 1) // T == rows // T)
        xs = x[src.clamp(0, B * T - 1)]
        if mutant == "mask_by_multiply":
            xs = xs * inside.to(x.dtype)[:, None]
        else:
            xs = torch.where(inside[:, None], xs, torch.zeros_like(xs))
        out = out + xs @ w[k].t()
    return out


def colsum(x, mutant=None):
    """column sums over the rows.  mutant: non-finite terms are skipped (`isfinite(v) ? v : 0`)"""
    if mutant == "colsum_skips_nonfinite":
        x = torch.where(torch.isfinite(x), x, torch.zeros_like(x))
    return x.sum(0)


# the CPU cases of the four restatements: (B, T, C) small enough to read, a boundary between samples in every one
CPU_SHAPE = (3, 5, 8)


def cpu_operands(seed=0):
    B, T, C = CPU_SHAPE
    g = torch.Generator().manual_seed(seed)
    return dict(x=torch.randn(B * T, C, generator=g), w=torch.randn(3, C, C, generator=g))


def restatement(name, o, mutant=None):
    """name of a mutant -> {output: tensor} of the restatement it belongs to (or of the mutant itself) on operands o"""
    B, T, _ = CPU_SHAPE
    if name == "softmax_skips_nan":
        return {"W": softmax_rows(o["x"], mutant)}
    if name == "saturating_store":
        return {"y fp16": store16(o["x"], torch.float16, mutant), "y bf16": store16(o["x"], torch.bfloat16, mutant)}
    if name == "mask_by_multiply":
        return {"y": conv3_rows(o["x"], o["w"], B, T, 1, mutant)}
    if name == "colsum_skips_nonfinite":
        return {"colsum": colsum(o["x"], mutant)}
    raise KeyError(name)


def cpu_cases():
    """(what, poisoned operands) for every poison value (the fp32 values that overflow a 16-bit store included) at every
    named position; the boundary between two samples stands in for a tile boundary"""
    B, T, C = CPU_SHAPE
    o = cpu_operands()
    values = dict(POISONS, **{f"{v:g}": v for v in OVERFLOW.values()})
    for pname, (b, t, c) in positions(B, T, C, flat_edges=()).items():
        for vname, v in values.items():
            yield f"{vname} at {pname}", dict(o, x=poisoned(o["x"], (b * T + t, c), v))
    for b, t, side in ((0, T - 1, "last row of sample 0"), (1, 0, "first row of sample 1")):
        for vname, v in values.items():
            yield f"{vname} at the {side}, channel 0", dict(o, x=poisoned(o["x"], (b * T + t, 0), v))


# ---------------------------------------------------------------------------------------------------------------
# the runner of tests/test_nonfinite_gpu.py and tests/test_nonfinite_losses_gpu.py
# ---------------------------------------------------------------------------------------------------------------
def run_cases(kernel, run, ref, operands, sites, values, what="", seen=None, unreached=(), finite_clean=True, structural=False):
    """run(o) -> {output: tensor}, ref(o) -> {output: tensor as stored}; sites: (site, operand, index) to poison, one at a time, with
    every value of `values`.  seen(o): the operands as the kernel reads them (a 1e5 handed to an fp16 operand IS an inf).
    `unreached` names the sites whose element the maths leaves out (a dropped pair): the reference must stay finite for every
    value there, and then the whole output owes the clean run's bits.  Every other site must reach an output with at least one
    value.  finite_clean=False: the unpoisoned reference may hold the -inf of an empty soft-max.
    structural=True: which elements the poisoned element enters is read off the reference with a NaN at the site (a NaN reaches
    everything the element enters), not off the reference's values — a bias of -inf or a norm of 1e5 moves sums and 16-bit
    coefficients by less than their rounding, and the stored reference then equals the clean one where the device, which adds in
    another order, lands an ulp away.  Such elements owe finiteness; only the others owe the clean run's bits."""
    seen = seen or (lambda o: o)
    clean, ref_clean = run(operands), ref(seen(operands))
    if finite_clean:
        for k, r in ref_clean.items():
            assert bool(torch.isfinite(r).all()), (kernel, k, "the unpoisoned reference is not finite")
    check_all(kernel, ref_clean, clean, clean, ref_clean, f"{what} unpoisoned")
    n = 0
    for site, key, index in sites:
        reached = False
        independent = None
        if structural:
            r_nan = ref(seen(dict(operands, **{key: poisoned(operands[key], index, NAN)})))
            independent = {k: torch.isfinite(t) & (t == ref_clean[k]) for k, t in r_nan.items()}
        for vname, v in values.items():
            o = dict(operands)
            o[key] = poisoned(operands[key], index, v)
            r = ref(seen(o))
            reached = reached or any(bool((torch.isfinite(t) != torch.isfinite(ref_clean[k])).any()) for k, t in r.items())
            check_all(kernel, r, run(o), clean, ref_clean, f"{what}, {vname} in {key} at {site}", independent)
            n += 1
        if site in unreached:
            assert not reached, (kernel, site, key, "the reference lets a dropped element reach an output")
        else:
            assert reached, (kernel, site, key, "no poison value at this site reaches an output")      # (a gate of +-inf alone does not)
    return n


# ---------------------------------------------------------------------------------------------------------------
# the loss kernels behind labels, SigmoidLoss and extra negatives (csrc/clip_labels.hip, sigmoid_loss.hip, clip_negatives.hip,
# sim_gemm.hip): cases shared by tests/test_nonfinite_cpu.py (no case passes vacuously; the mutants are caught) and
# tests/test_nonfinite_losses_gpu.py (the kernels).  A case = dict(kernel, what, operands, sites, ref, values, unreached, coupled,
# finite_clean): `ref` is the restatement of the kernel's own case module — its fp32 emulation, whose torch operators have IEEE
# semantics and whose masks are selects — as ref(operands, mutant=None) -> {output: tensor as stored}; `coupled` names the sites
# at which the maths leaves no finite element that is independent of the poison.
# ---------------------------------------------------------------------------------------------------------------
LOSS_BLOCKS = ((15, 5, 10), (257, 257, 0), (140, 70, 70))          # (Bm, Bn, col0)
LOSS_PATTERNS = ("pair", "straddle3", "partners_outside", "one_class")
LOSS_MODES = ("positive", "mask")
LOSS_DTYPES = (torch.float32, torch.bfloat16, torch.float16)
NEG_SHAPES = ((2, 31), (64, 33), (3, 256), (70, 257))              # (Bn, N)
DZ_SHAPES = ((2, 31, 5), (65, 33, 4), (257, 256, 4), (65, 257, 9))  # (Bn, N, T)
DZ_PATTERNS = ("overlap", "edges")
SIM_SHAPES = ((5, 33), (257, 257))                                 # (M, N); K = SIM_T * SIM_FP
SIM_T, SIM_FP, SIM_ROWS = 4, 64, 40
_CACHE = {}


def _cached(key, make):
    if key not in _CACHE:
        _CACHE[key] = make()
    return _CACHE[key]


def dtype_name(dtype):
    return str(dtype).replace("torch.", "")


def matrix_positions(Bm, Bn, col0, same, pos):
    """name -> (i, j) of a block's (speech row i, local brain column j) matrix: a positive, a repeat of the column's speech, an
    ordinary negative, row 0, the last row, rows 255 | 256 and columns 63 | 64 where they exist, a row in front of the block's
    own columns.  (What a named row or column holds — positive, repeat or negative — is the pattern's business: one_class makes
    every one of them a repeat.)"""
    out = {"the positive of column 0": (col0, 0), "the positive of the last column": (col0 + Bn - 1, Bn - 1)}
    rep, neg = (same & ~pos).nonzero(), (~same).nonzero()
    if rep.numel():
        out["the first repeat of a column's speech"] = tuple(int(v) for v in rep[0])
        out["the last repeat of a column's speech"] = tuple(int(v) for v in rep[-1])
    if neg.numel():
        out["an ordinary negative"] = tuple(int(v) for v in neg[neg.shape[0] // 2])
    out["row 0"] = (0, Bn // 2)
    out["the last row"] = (Bm - 1, (Bn // 2 + 1) % Bn)
    if Bm > 256:
        out["row 255, in front of the second pass of the 256-thread stride"] = (255, 1)
        out["row 256, the second pass of the 256-thread stride"] = (256, Bn - 2)
    if Bn > 64:
        out["column 63, the last of the first 64-wide tile"] = (Bm // 2, 63)
        out["column 64, the first of the second 64-wide tile"] = (Bm // 2 + 1, 64)
    if col0 > 0:
        out["a row in front of the block's own columns"] = (col0 - 1, Bn - 1)
    seen, uniq = set(), {}
    for k, ij in out.items():
        if ij not in seen:
            seen.add(ij)
            uniq[k] = ij
    return uniq


def _sites(key, positions):
    return [(f"{key}: {k}", key, ij) for k, ij in positions.items()]


def _dropped_sites(key, positions, drop):
    return {f"{key}: {k}" for k, ij in positions.items() if bool(drop[ij])}


def label_cases(Bm, Bn, col0, pattern):
    """the cases of csrc/clip_labels.hip on one block and label pattern (regime `trained`): the masked statistics (mask mode's
    only: positive mode runs the unlabelled kernel), and in both modes and every storage type of G / Gy the two coefficient
    kernels.  Repeat sites in mask mode: the loss does not depend on that entry, so a non-finite logit there reaches no statistic,
    no G / Gy entry, no rscale / part / colpart / scalar — only the stored logits entry itself."""
    from tests import clip_label_cases as LC
    c = _cached(("label", Bm, Bn, col0, pattern), lambda: LC.label_case(Bm, Bn, col0, "trained", pattern))
    P = matrix_positions(Bm, Bn, col0, c["same"], c["pos"])
    tag = f"({Bm}, {Bn}, {col0}) {pattern}"
    names = ("logits", "row_max", "row_sum", "col_lse", "diag", "row_lse")
    yield dict(kernel="clip_logits_stats_masked", what=f"{tag} mask", mode="mask", dtype=torch.float32, operands=c, unreached=set(),
               sites=_sites("S", P) + [("the temperature", "temp", (0,))], values=poisons(None), finite_clean=False,
               coupled={"the temperature"}, ref=lambda o, mutant=None: dict(zip(names, LC.emul_masked_stats(o, mutant=mutant))))
    nparts = (Bn + 63) // 64
    j1, i_in = min(1, Bn - 1), col0 + Bn - 1
    for mode in LOSS_MODES:
        rl, cl = ("row_lse_m", "col_lse_m") if mode == "mask" else ("row_lse", "col_lse")
        drop = LC.dropped(c, mode)
        for dtype in LOSS_DTYPES:
            def ref_g(o, mutant=None, mode=mode, dtype=dtype):
                r = LC.emul_grad_labels_parts(o, mode, dtype, mutant=mutant)
                return dict(r, G=r["G"][:Bm + 1])

            def ref_gy(o, mutant=None, mode=mode, dtype=dtype):
                Gy, part = LC.emul_grad_y_labels(o, mode, dtype, mutant=mutant)
                return {"Gy": Gy[:Bn + 1], "part": part[:nparts]}

            common = dict(what=f"{tag} {mode} {dtype_name(dtype)}", mode=mode, dtype=dtype, operands=c, values=poisons(dtype), finite_clean=True,
                          coupled=set())
            yield dict(common, kernel="clip_grad_labels", ref=ref_g, unreached=_dropped_sites("logits", P, drop),
                       sites=_sites("logits", P) + [("row_lse of the last column's positive", rl, (i_in,)), ("col_lse, the last column", cl, (Bn - 1,)),
                                                    ("the speech norms, row 1", "ysq", (1,)), ("the brain norms, the last column", "zsq", (Bn - 1,)),
                                                    ("the temperature", "temp", (0,))])
            yield dict(common, kernel="clip_grad_y_labels", ref=ref_gy, unreached=_dropped_sites("logits", P, drop),
                       sites=_sites("logits", P) + [("row_lse of column 1's positive", rl, (col0 + j1,)), ("col_lse, the last column", cl, (Bn - 1,)),
                                                    ("the brain norms, column 1", "zsq", (j1,)), ("every rank's brain norms, sample 0", "zsq_all", (0,))])


def sigmoid_cases(Bm, Bn, col0, pattern):
    """the cases of csrc/sigmoid_loss.hip that tests/test_sigmoid_loss_gpu.py leaves open: sigmoid_grad_y with labels in both
    modes, sigmoid_pairs + sigmoid_finish in mask mode.  A dropped pair is held to sigmoid_loss_cases.check_dropped_nan's contract
    for Gy and part as well: nothing but the stored a entry itself."""
    from tests import sigmoid_loss_cases as SG
    c = _cached(("sigmoid", Bm, Bn, col0, pattern), lambda: SG.with_labels(SG.sig_case(Bm, Bn, col0, "trained"), pattern))
    P = matrix_positions(Bm, Bn, col0, c["same"], c["pos"])
    tag = f"({Bm}, {Bn}, {col0}) {pattern}"
    nparts_y, nparts = (Bn + 63) // 64, (Bm + 63) // 64
    j1 = min(1, Bn - 1)
    for dtype in LOSS_DTYPES:
        for mode in LOSS_MODES:
            drop = SG.signs(c, mode) == 0

            def ref_gy(o, mutant=None, mode=mode, dtype=dtype):
                Gy, part = SG.emul_grad_y(o, mode, dtype, mutant=mutant)
                return {"Gy": Gy[:Bn + 1], "part": part[:nparts_y]}

            yield dict(kernel="sigmoid_grad_y", what=f"{tag} {mode} {dtype_name(dtype)}", mode=mode, dtype=dtype, operands=c, values=poisons(dtype),
                       finite_clean=True, coupled=set(), ref=ref_gy, unreached=_dropped_sites("a", P, drop),
                       sites=_sites("a", P) + [("the bias", "bias", (0,)), ("the brain norms, column 1", "zsq", (j1,)),
                                               ("every rank's brain norms, sample 0", "zsq_all", (0,))])

        def ref_pf(o, mutant=None, dtype=dtype):
            a, diag, G, part = SG.emul_pairs(o, "mask", dtype, mutant=mutant)
            rs, cs, sc = SG.emul_finish(o, part[:nparts])
            return {"a": a[:Bm], "diag": diag[:Bm], "G": G[:Bm + 1], "part": part[:nparts], "rscale": rs[:Bn], "cscale": cs[:Bn], "scalars": sc[:3]}

        yield dict(kernel="sigmoid_pairs + sigmoid_finish", what=f"{tag} mask {dtype_name(dtype)}", mode="mask", dtype=dtype, operands=c,
                   values=poisons(dtype), finite_clean=True, coupled=set(), ref=ref_pf, unreached=set(),
                   sites=_sites("S", P) + [("the bias", "bias", (0,)), ("the brain norms, column 1", "zsq", (j1,)), ("the temperature", "temp", (0,)),
                                           ("the speech norms, row 1 (the range factor ymax: the one way a bounded D overflows G)", "ysq", (1,))])


def neg_positions(Bn, N):
    """name -> (j, n) of the negatives' (brain column j, negative n) matrix"""
    out = {"first column, first negative": (0, 0), "last column, last negative": (Bn - 1, N - 1), "negative 31, the last of the first K-step": (Bn // 2, min(31, N - 1))}
    if N > 32:
        out["negative 32, the first of the second K-step"] = (Bn // 2, 32)
    if N > 255:
        out["negative 255, in front of the second pass of the 256-thread stride"] = (min(1, Bn - 1), 255)
    if N > 256:
        out["negative 256, the second pass of the 256-thread stride"] = (Bn - 1, 256)
    return {k: ij for i, (k, ij) in enumerate(out.items()) if ij not in list(out.values())[:i]}


def neg_cases(Bn, N):
    """sda_clip_neg_stats and sda_clip_neg_grad (regime `trained`).  The incoming rscale[j] and scalars[1] the grad kernel adds to
    are operands: a non-finite value there stays.  G^n is compared whole: its rows N ... neg_rows(N) - 1 and its pad columns are
    zeros of the reference that depend on nothing, so they owe the clean run's bits — exact zeros — whatever the poison."""
    from tests import clip_negative_cases as NC
    c = _cached(("neg", Bn, N), lambda: NC.stats_case(Bn, N, "trained"))
    P = neg_positions(Bn, N)
    tag = f"({Bn}, {N})"
    nr = NC.neg_rows(N)
    yield dict(kernel="clip_neg_stats", what=tag, dtype=torch.float32, operands=c, values=poisons(None), finite_clean=True, unreached=set(),
               coupled={"the temperature"}, ref=lambda o, mutant=None: dict(zip(("mlog", "col_lse"), NC.emul_neg_stats(o, mutant=mutant))),
               sites=_sites("S", P) + [("the negatives' norms, the last", "wsq", (N - 1,)), ("the brain norms, column 0", "zsq", (0,)),
                                       ("the temperature", "temp", (0,)), ("the incoming col_lse, the last column", "col_lse", (Bn - 1,))])
    for dtype in (torch.bfloat16, torch.float16):
        def ref_g(o, mutant=None, dtype=dtype):
            G, cs, rs, sc, cp = NC.emul_neg_grad(o, dtype, mutant=mutant, colpart=True)
            return {"Gn": G[:nr], "cscale_n": cs, "rscale": rs, "scalars": sc, "colpart": cp}

        yield dict(kernel="clip_neg_grad", what=f"{tag} {dtype_name(dtype)}", dtype=dtype, operands=c, values=poisons(dtype), finite_clean=True,
                   unreached=set(), coupled=set(), ref=ref_g,
                   sites=_sites("mlog", P) + [("the merged col_lse, the last column", "col_lse_merged", (Bn - 1,)),
                                              ("the negatives' norms, the last", "wsq", (N - 1,)), ("the brain norms, column 0", "zsq", (0,)),
                                              ("the temperature", "temp", (0,)), ("the incoming rscale, column 0", "rscale_in", (0,)),
                                              ("the incoming d loss / d temp", "scalars_in", (1,))])


def table_rows(starts, T, L):
    """name -> table row: in exactly one window, in several, in the last candidate's alone (the window the K-steps past N
    re-read), in none (between windows, in front of the smallest or behind the largest start), and the last candidate's first row
    whatever else holds it — those of them the starts offer"""
    starts = [int(s) for s in starts]
    count = [sum(s <= r < s + T for s in starts) for r in range(L)]
    last = range(starts[-1], starts[-1] + T)
    out = {}
    first = lambda rows: next((r for r in rows), None)
    for k, r in (("a row of exactly one window", first(r for r in range(L) if count[r] == 1 and r not in last)),
                 ("a row of several overlapping windows", first(r for r in reversed(range(L)) if count[r] >= 2)),
                 ("a row of the last candidate's window alone", first(r for r in last if count[r] == 1)),
                 ("the first row of the last candidate's window", starts[-1]),
                 ("a row of no window, inside the table", first(r for r in reversed(range(L)) if count[r] == 0)),
                 ("a row of no window, in front of the largest start", first(r for r in range(max(starts)) if count[r] == 0))):
        if r is not None and r not in out.values():
            out[k] = r
    return out


def dz_cases(Bn, N, T, pattern):
    """sda_clip_dz_windows, bf16 and fp16.  From the restatement dz_windows_ref: a table element (r, c) reaches
    dZ[j][(r - starts[n]) Fp + c] for every j < Bn and every n whose window holds r, an element of no window nothing; G^n[n][j] and
    cscale_n[j] reach brain row j, out[j][k] itself.  G^n, the table and out live in the storage type (the three IEEE poisons);
    cscale_n and out_scale are fp32 and stored nowhere themselves (the three as well: a finite factor of 1e5 would put elements
    next to fp16's largest value, where the kernel's own rounding decides)."""
    from tests import clip_negative_cases as NC
    for dtype in (torch.bfloat16, torch.float16):
        def make():
            # two more table rows behind the case's own: whatever the starts, rows of no window inside the allocation
            c = NC.dz_case(Bn, N, T, pattern, dtype)
            more = NC.q(torch.randn(2, c["Fp"], generator=torch.Generator().manual_seed(N)), dtype)
            return dict(c, table=torch.cat([c["table"], more]))

        c = _cached(("dz", Bn, N, T, pattern, dtype), make)
        Fp, L = c["Fp"], c["table"].shape[0]
        rows = table_rows(c["starts"], T, L)
        chans = (0, Fp - 1)
        sites = [(f"the table: {k}, channel {chans[i % 2]}", "table", (r, chans[i % 2])) for i, (k, r) in enumerate(rows.items())]
        unreached = {s[0] for s in sites if "no window" in s[0]}
        data = c["data_rows"].nonzero().flatten()
        sites += [("G^n, first negative, first column", "Gn", (0, 0)), ("G^n, last negative, last column", "Gn", (N - 1, Bn - 1)),
                  ("cscale_n, the last column", "cscale", (Bn - 1,)), ("out_scale", "out_scale", (0,)),
                  ("out, the last data row, channel 0", "out", (int(data[-1]), 0))]

        def ref(o, mutant=None, dtype=dtype):
            return {"dZ": NC.emul_dz_windows(o, dtype, mutant)[:-1]}

        yield dict(kernel="clip_dz_windows", what=f"({Bn}, {N}, {T}) {pattern} {dtype_name(dtype)}", dtype=dtype, operands=c, values=dict(POISONS),
                   finite_clean=True, unreached=unreached, coupled=set(), ref=ref, sites=sites)


def sim_cases(M, N):
    """sda_sim_gemm_windows and, on the same windows cut out, sda_sim_gemm (K = SIM_T x SIM_FP): X[i][k] reaches row i, a table
    element the columns of the candidates whose window holds it.  Each product is handed over as its N real columns and, as an
    output of its own, its pad columns (the exception "sim_gemm" covers exactly those)."""
    from tests import clip_negative_cases as NC
    for dtype in (torch.bfloat16, torch.float16):
        c = _cached(("sim", M, N, dtype), lambda: NC.sim_case(M, N, SIM_T, SIM_FP, dtype))
        L, K = c["table"].shape[0], c["K"]
        s = [int(v) for v in c["starts"]]
        sites = [("X: row 0, k 0", "X", (0, 0)), ("X: the last row, the last k", "X", (M - 1, K - 1))]
        if M > 256:
            sites += [("X: row 255, in front of the second tile", "X", (255, 1)), ("X: row 256, the second tile", "X", (256, K - 2))]
        sites += [("the table: a row of one window (the first candidate's)", "table", (s[0] + 1, 0)),
                  ("the table: a row of two windows", "table", (s[1], SIM_FP - 1)),
                  ("the table: the last row of the last candidate's window", "table", (s[-1] + SIM_T - 1, 1)),
                  ("the table: a row of no window, in front of the smallest start", "table", (s[0] - 1, SIM_FP - 1)),
                  ("the table: a row of no window, behind the last", "table", (L - 1, 0))]

        def ref(o, mutant=None):
            S = NC.sim_windows_ref(o).float()
            return {"S": S, "S" + PAD_COLS: torch.zeros(M, NC.pad64(N) - N)}

        yield dict(kernel="sim_gemm", what=f"({M}, {N}) {dtype_name(dtype)}", dtype=dtype, operands=c, values=dict(POISONS), finite_clean=True,
                   unreached={k for k, _, _ in sites if "no window" in k}, coupled=set(), ref=ref, sites=sites)
