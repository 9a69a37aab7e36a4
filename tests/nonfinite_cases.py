"""Poison values, named poison positions, the two checks and plain-torch restatements (with seeded mutants) for the tests
of inf / NaN propagation through the backward kernels (tests/test_nonfinite_cpu.py proves on the CPU that the checks catch
the four ways a kernel swallows or leaks a non-finite value; tests/test_nonfinite_gpu.py holds the HIP kernels to the same
checks; tests/test_overflow_guard_gpu.py runs the fp16 overflow guard that depends on them).  Nothing here needs a GPU.

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


# kernel -> (reason, widen): the deliberate trades.  Both kernels mask by a zero operand instead of a select (0 * inf = NaN), which
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


def split_pad(label, t, C, dim=1):
    """an output with padded channels along `dim` -> {label: the real channels, label + PAD: the pad channels} (nothing when
    there are none)"""
    n = t.shape[dim]
    out = {label: t.narrow(dim, 0, C).contiguous()}
    if n > C:
        out[label + PAD] = t.narrow(dim, C, n - C).contiguous()
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


def check(ref, got, clean, ref_clean, allowed=None):
    """ref: the restatement on the poisoned operands (any float dtype, as stored()), got: the output under test on the same
    operands, clean: the same call on the unpoisoned operands, ref_clean: the restatement on the unpoisoned operands.
    allowed (EXCEPTIONS): mask of the elements that may be non-finite although the reference is finite there.
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
    changed = ~bad_ref & ~bad_got & (ref == ref_clean) & (_bits(got) != _bits(clean))
    if bool(leaked.any()):
        i = _first(leaked)
        out["containment"] = (f"{int(leaked.sum())} of {int((~bad_ref).sum())} finite elements came out non-finite, first at {i}: "
                              f"reference {float(ref[i])}, got {float(got[i])}")
    elif bool(changed.any()):
        i = _first(changed)
        out["containment"] = (f"{int(changed.sum())} finite elements changed their bits, first at {i}: "
                              f"got {float(got[i])!r}, on the unpoisoned operands {float(clean[i])!r}")
    return out


def check_all(kernel, refs, gots, cleans, refs_clean, what=""):
    """dicts output name -> tensor; asserts both checks on every output (a kernel listed in EXCEPTIONS: with its widened mask)"""
    assert set(refs) == set(gots) == set(cleans) == set(refs_clean), (kernel, sorted(refs), sorted(gots), sorted(cleans))
    failed = {}
    for name in refs:
        allowed = EXCEPTIONS[kernel][1](name, refs) if kernel in EXCEPTIONS else None
        res = check(refs[name], gots[name], cleans[name], refs_clean[name], allowed)
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
