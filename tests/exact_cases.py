"""Small-integer operands, integer references and CPU emulations for the exact-arithmetic tests of the matrix-core kernels,
shared by tests/test_exact_cpu.py (which proves on the CPU that the cases exercise the rounding and that every mutant of
the reference is caught) and tests/test_exact_gpu.py (which runs them on the kernels with torch.equal).

With operands that are integers in [-R, R] every product and every fp32 partial sum is an integer below 2^24: the
accumulator is the same in every summation order, tiling and split-K plan, and the one correct stored value is the
round-to-nearest-even rounding of the exact result.  Two regimes:
    "exact"     R <= 3, lowered per shape until every stored output is representable in bf16, fp16 and fp32: the three
                storage types must give identical values;
    "rounding"  R >= 15, raised per shape and type until at least 10 % of the outputs are not representable in the stored
                type and at least 1 % are exact ties: the expected output is torch's round-to-nearest-even of the exact one.
Everything here is plain torch on the CPU, computed in float64 (exact on integers below 2^53)."""
import functools
from collections import namedtuple

import torch
import torch.nn.functional as TF

DTYPES = [torch.float32, torch.bfloat16, torch.float16]
DTYPES16 = [torch.bfloat16, torch.float16]
REGIMES = ["exact", "rounding"]
R_EXACT = (3, 2, 1)
R_ROUND = (15, 19, 23, 27, 31, 35, 39, 47, 55, 63, 79, 95, 127)
MIN_INEXACT, MIN_TIES = 0.10, 0.01
_DROP = {torch.bfloat16: 16, torch.float16: 13}       # fp32 mantissa bits a 16-bit store drops (normal numbers)


# ---------------------------------------------------------------------------------------------------------------
# operands, stores
# ---------------------------------------------------------------------------------------------------------------
def ints(shape, R, seed):
    """seeded integers in [-R, R] as float64"""
    g = torch.Generator().manual_seed(seed)
    return torch.randint(-R, R + 1, tuple(shape), generator=g).double()


def operand(t, dtype):
    """float64 values -> the storage type, asserted lossless"""
    o = t.to(dtype)
    assert torch.equal(o.double(), t.double()), f"operand not representable in {dtype}"
    return o


def _trunc_next(y, dtype):
    """(toward-zero neighbour, away-from-zero neighbour) of float32-representable y in a 16-bit type, as float64"""
    f = y.float()
    assert torch.equal(f.double(), y), "exact value beyond float32"
    bits = f.view(torch.int32)
    lo = bits & ~((1 << _DROP[dtype]) - 1)
    hi = lo + (1 << _DROP[dtype])                       # one unit in the kept mantissa; carries into the exponent
    return lo.view(torch.float32).double(), hi.view(torch.float32).double()


def store(y, dtype, mode="rne"):
    """what a store of the fp32 accumulator y (float64 here, float32-representable) leaves in `dtype`, as float64.
    mode "rne" is the contract (torch's cast); "trunc" and "half_away" are mutants."""
    if dtype == torch.float32:
        return y.float().double()
    if mode == "rne":
        return y.float().to(dtype).double()
    lo, hi = _trunc_next(y, dtype)
    if mode == "trunc":
        return lo
    assert mode == "half_away"
    return torch.where((y - lo).abs() >= (hi - y).abs(), hi, lo).where(lo != y, y)


def representable(y, dtype):
    return y.float().to(dtype).double() == y


def is_tie(y, dtype):
    if dtype == torch.float32:
        return torch.zeros_like(y, dtype=torch.bool)
    lo, hi = _trunc_next(y, dtype)
    return (lo != y) & ((y - lo).abs() == (hi - y).abs())


def shares(y, dtype):
    """(share of outputs not representable in dtype, share that are exact ties)"""
    n = max(1, y.numel())
    return float((~representable(y, dtype)).sum()) / n, float(is_tie(y, dtype).sum()) / n


def check_regime(y, regime, dtype, what=""):
    """The conditions a case must meet, asserted: see the module docstring."""
    m = float(y.abs().max()) if y.numel() else 0.0
    assert m < 2 ** 24, f"{what}: |reference| reaches {m}"
    if regime == "exact":
        for d in DTYPES:
            assert bool(representable(y, d).all()), f"{what}: an exact-regime output is not representable in {d}"
        return
    if dtype == torch.float32:
        return
    if dtype == torch.float16:
        assert m <= 2 ** 15, f"{what}: |reference| {m} beyond 2^15 in fp16"
    inexact, ties = shares(y, dtype)
    assert inexact >= MIN_INEXACT and ties >= MIN_TIES, f"{what}: {inexact:.3f} not representable, {ties:.3f} ties in {dtype}"


def _search(build, regime, dtype, what):
    """first R of the regime's ladder whose reference meets check_regime"""
    last = None
    for R in (R_EXACT if regime == "exact" else R_ROUND):
        case = build(R)
        try:
            check_regime(case.ref, regime, dtype, what)
            return case
        except AssertionError as e:
            last = e
    raise AssertionError(f"{what}: no R of the {regime} ladder meets the conditions ({last})")


# ---------------------------------------------------------------------------------------------------------------
# failure helper
# ---------------------------------------------------------------------------------------------------------------
def mismatch(got, want, axes="bct"):
    """None when equal; else 'n of N differ, first at (b, c, t) = ...: got x expected y' (a tile edge shows in the index)"""
    got, want = got.detach().cpu().double(), want.detach().cpu().double()
    if got.shape != want.shape:
        return f"shape {tuple(got.shape)} != {tuple(want.shape)}"
    bad = ~((got == want) | (torch.isnan(got) & torch.isnan(want)))
    n = int(bad.sum())
    if n == 0:
        return None
    idx = tuple(int(i) for i in bad.nonzero()[0])
    names = ", ".join(axes[:len(idx)]) if len(axes) >= len(idx) else "index"
    return f"{n} of {bad.numel()} differ, first at ({names}) = {idx}: got {float(got[idx])!r} expected {float(want[idx])!r}"


def assert_same(got, want, what, axes="bct"):
    msg = mismatch(got, want, axes)
    assert msg is None, f"{what}: {msg}"


# ---------------------------------------------------------------------------------------------------------------
# references (float64 on integers: exact)
# ---------------------------------------------------------------------------------------------------------------
def conv_taps(x, w, dil):
    """per-tap partial sums [KS] of (B, Cout, T) of a "same" zero-padded, dilated conv1d; x (B, Cin, T), w (Cout, Cin, KS)"""
    KS, T = w.shape[-1], x.shape[-1]
    pad = dil * (KS // 2)
    xp = TF.pad(x, (pad, pad))
    return [torch.einsum("oc,bct->bot", w[:, :, k], xp[:, :, k * dil: k * dil + T]) for k in range(KS)]


def conv_ref(x, w, dil, bias=None, res=None):
    """y = bias + conv(x, w) + res in exact arithmetic (sda_conv_args: both enter the fp32 accumulator, one rounding)"""
    KS = w.shape[-1]
    y = TF.conv1d(x, w, bias, padding=dil * (KS // 2), dilation=max(dil, 1))
    return y if res is None else y + res


def dgrad_ref(dy, w, dil):
    """dx of conv_ref with respect to x: (B, Cin, T)"""
    KS = w.shape[-1]
    return TF.conv1d(dy, w.transpose(0, 1).flip(2), None, padding=dil * (KS // 2), dilation=max(dil, 1))


def wgrad_ref(dy, x, KS, dil, sample_seg=None, nseg=1):
    """g[seg][co][ci][tap] = sum over the segment's samples and t of dy[b, co, t] * x[b, ci, t + (tap - KS/2) dil]"""
    B, _, T = x.shape
    pad = dil * (KS // 2)
    xp = TF.pad(x, (pad, pad))
    per = torch.stack([torch.einsum("bot,bct->boc", dy, xp[:, :, k * dil: k * dil + T]) for k in range(KS)], dim=-1)
    g = torch.zeros((nseg,) + tuple(per.shape[1:]), dtype=torch.float64)
    for b in range(B):
        g[0 if sample_seg is None else int(sample_seg[b])] += per[b]
    return g


def matmul_nt_ref(A, Bm):
    return A @ Bm.t()


# ---------------------------------------------------------------------------------------------------------------
# the conv forward cases and their emulation with mutants
# ---------------------------------------------------------------------------------------------------------------
ConvShape = namedtuple("ConvShape", "cin cout dil T B")
# T below / above one 128-row tile (40, 129, 130), T = 1, dil = 16 = the row padding, T < dil; B * (T + 16) rows put the flat
# kernel's 128-row tiles across two (or all) samples and leave the last tile partial — with no CU limit a shape this small is
# planned one unit per workgroup, so the flat kernel's 256-row tile does not run here: tests/persistent_cases.py has the
# (shape, CU limit) pairs that run it; Cout_p on the 64- (48, 64), 160- (320, 640, 160) and 128-channel (128) tiles; Cin 40 and
# 96 are no multiples of 64.  cin == cout: the residual is the conv's own input.
CONV3_SHAPES = [ConvShape(40, 48, 1, 40, 3), ConvShape(320, 320, 16, 130, 2), ConvShape(64, 640, 4, 129, 3),
                ConvShape(96, 128, 2, 1, 5), ConvShape(64, 64, 16, 9, 4), ConvShape(64, 160, 16, 5, 7)]
EPILOGUES = ["bare", "bias", "bias_res"]
CONV_MUTANTS = ["trunc_store", "half_away_store", "round_each_tap", "round_each_k64", "bias_after_store", "res_after_store",
                "drop_last_k32_one_tile", "tap0_reads_neighbour", "dup_row128"]
ConvCase = namedtuple("ConvCase", "shape R x w bias res ref")      # ref = the bias_res form when the shape has a residual


def _has_res(s):
    return s.cin == s.cout


def _conv_build(s, KS, seed, R):
    x, w = ints((s.B, s.cin, s.T), R, seed), ints((s.cout, s.cin, KS), R, seed + 1)
    bias = ints((s.cout,), R, seed + 2)
    res = x if _has_res(s) else None
    return ConvCase(s, R, x, w, bias, res, conv_ref(x, w, s.dil, bias, res))


@functools.lru_cache(maxsize=None)
def conv3_case(i, regime, dtype):
    """operands of CONV3_SHAPES[i]; exact-regime operands are the same for every dtype"""
    s = CONV3_SHAPES[i]
    key = None if regime == "exact" else dtype
    if key == torch.float32:
        return conv3_case(i, regime, torch.bfloat16)
    return _search(lambda R: _conv_build(s, 3, 1000 + 10 * i, R), regime, key, f"conv3 {tuple(s)}")


def conv_expected(case, epilogue):
    """exact value of one epilogue form"""
    s = case.shape
    return conv_ref(case.x, case.w, s.dil, None if epilogue == "bare" else case.bias, case.res if epilogue == "bias_res" else None)


def conv_emulation(case, dtype, mutant=None):
    """The forward conv as the kernels are meant to compute it — integer partial sums in any order, bias and residual into the
    accumulator, one round-to-nearest-even store — or one subtly wrong variant of it (CONV_MUTANTS).  Returns float64 (B, Cout, T)."""
    assert mutant is None or mutant in CONV_MUTANTS
    s, x, w = case.shape, case.x, case.w
    KS = w.shape[-1]
    r16 = lambda v: store(v, dtype)
    if mutant == "round_each_tap":
        acc = torch.zeros(s.B, s.cout, s.T, dtype=torch.float64)
        for p in conv_taps(x, w, s.dil):
            acc = r16(acc + p)
    elif mutant == "round_each_k64":
        acc = torch.zeros(s.B, s.cout, s.T, dtype=torch.float64)
        for k in range(KS):
            for c0 in range(0, s.cin, 64):
                wk = torch.zeros_like(w)
                wk[:, c0:c0 + 64, k] = w[:, c0:c0 + 64, k]
                acc = r16(acc + conv_ref(x, wk, s.dil))
    elif mutant == "tap0_reads_neighbour":
        # the rows in front of sample b >= 1 hold the tail of sample b - 1 instead of zeros
        acc = conv_ref(x, w, s.dil)
        if KS == 3:
            for b in range(1, s.B):
                for t in range(min(s.dil, s.T)):
                    src = s.T + t - s.dil
                    if src >= 0:
                        acc[b, :, t] += w[:, :, 0] @ x[b - 1, :, src]
    else:
        acc = conv_ref(x, w, s.dil)
    if mutant == "drop_last_k32_one_tile":
        # the last 32 elements of the padded contraction (last tap, channels [Cin_p - 32, Cin_p)) of the last sample's first tile
        cin_p = (s.cin + 63) // 64 * 64
        wk = torch.zeros_like(w)
        wk[:, cin_p - 32:, KS - 1] = w[:, cin_p - 32:, KS - 1]
        acc[s.B - 1, :, :128] -= conv_ref(x[s.B - 1:], wk, s.dil)[0, :, :128]
    bias = case.bias[None, :, None]
    res = case.res if case.res is not None else torch.zeros_like(acc)
    if mutant == "bias_after_store":
        y = r16(r16(acc + res) + bias)
    elif mutant == "res_after_store":
        y = r16(r16(acc + bias) + res)
    else:
        y = store(acc + bias + res, dtype, {"trunc_store": "trunc", "half_away_store": "half_away"}.get(mutant, "rne"))
    if mutant == "dup_row128" and s.T > 128:
        y[:, :, 128] = y[:, :, 127]
    return y


# F.glu in the flat kernel's epilogue: (cin, half, dil, T, B); the conv has 2 * half output channels [value | gate]
GLU_SHAPE = ConvShape(64, 600, 2, 129, 3)
GLU_HALF = 300


@functools.lru_cache(maxsize=None)
def glu_case(regime, dtype):
    key = None if regime == "exact" else dtype
    if key == torch.float32:
        return glu_case(regime, torch.bfloat16)
    return _search(lambda R: _conv_build(GLU_SHAPE, 3, 1900, R), regime, key, "conv3 glu")


# ---------------------------------------------------------------------------------------------------------------
# kernel size 1
# ---------------------------------------------------------------------------------------------------------------
# (cin, cout, dil, T, B): tile kernel with per-sample weights; conv1_flat on 128- and 160-channel tiles; conv1_wide on 256 and 320
CONV1_SHAPES = {"tile_widx": ConvShape(72, 72, 0, 40, 5), "flat128": ConvShape(100, 128, 0, 77, 2), "flat160": ConvShape(100, 320, 0, 40, 5),
                "wide256": ConvShape(96, 256, 0, 129, 3), "wide320": ConvShape(64, 320, 0, 130, 3)}
CONV1_NW = 4
CONV1_WIDX = [2, 0, 3, 3, 1]
Conv1Case = namedtuple("Conv1Case", "shape R x w bias widx ref")


def _conv1_build(name, seed, R):
    s = CONV1_SHAPES[name]
    x, bias = ints((s.B, s.cin, s.T), R, seed), ints((s.cout,), R, seed + 2)
    if name == "tile_widx":
        w = ints((CONV1_NW, s.cout, s.cin, 1), R, seed + 1)
        widx = torch.tensor(CONV1_WIDX, dtype=torch.int32)
        ref = torch.bmm(w[widx.long(), :, :, 0], x) + bias[None, :, None]
    else:
        w, widx = ints((s.cout, s.cin, 1), R, seed + 1), None
        ref = conv_ref(x, w, 0, bias)
    return Conv1Case(s, R, x, w, bias, widx, ref)


@functools.lru_cache(maxsize=None)
def conv1_case(name, regime, dtype):
    """ref = conv + bias (the pre-activation)"""
    key = None if regime == "exact" else dtype
    if key == torch.float32:
        return conv1_case(name, regime, torch.bfloat16)
    return _search(lambda R: _conv1_build(name, 2000 + 10 * sorted(CONV1_SHAPES).index(name), R), regime, key, f"conv1 {name}")


def row_sumsq_ref(y, group=128):
    """(B, T, Cout / group) sums of squares of each row's channel groups"""
    B, C, T = y.shape
    return (y * y).permute(0, 2, 1).reshape(B, T, C // group, group).sum(-1)


# ---------------------------------------------------------------------------------------------------------------
# data gradient
# ---------------------------------------------------------------------------------------------------------------
DgradShape = namedtuple("DgradShape", "cin cout KS dil T B glu")
DGRAD_SHAPES = [DgradShape(40, 48, 3, 2, 70, 3, False), DgradShape(64, 48, 3, 16, 40, 3, True), DgradShape(320, 640, 3, 2, 130, 2, True),
                DgradShape(96, 128, 3, 16, 129, 2, False), DgradShape(72, 100, 1, 0, 77, 3, False)]
DgradCase = namedtuple("DgradCase", "shape R dy w ref")


@functools.lru_cache(maxsize=None)
def dgrad_case(i, regime, dtype):
    s = DGRAD_SHAPES[i]
    key = None if regime == "exact" else dtype
    if key == torch.float32:
        return dgrad_case(i, regime, torch.bfloat16)

    def build(R):
        dy, w = ints((s.B, s.cout, s.T), R, 3000 + 10 * i), ints((s.cout, s.cin, s.KS), R, 3001 + 10 * i)
        return DgradCase(s, R, dy, w, dgrad_ref(dy, w, s.dil))
    return _search(build, regime, key, f"dgrad {tuple(s)}")


# ---------------------------------------------------------------------------------------------------------------
# weight gradient (fp32 slabs: exact in every type, one operand set) and its typed-output mode
# ---------------------------------------------------------------------------------------------------------------
WgradShape = namedtuple("WgradShape", "cin cout KS dil T B subjects")
# T = 77, 100, 130: no multiples of the 32- / 64-row K chunk; T = 104 + 24 = 128: a sample that pads to whole chunks
WGRAD_SHAPES = [WgradShape(40, 48, 3, 2, 77, 5, [1, 3, 1, 0, 3]), WgradShape(64, 160, 3, 16, 130, 4, [2, 0, 2, 0]),
                WgradShape(72, 128, 1, 0, 100, 6, [1, 3, 1, 0, 3, 3]), WgradShape(70, 160, 3, 1, 104, 7, [2, 0, 2, 2, 0, 2, 0])]
WGRAD_R = 15
WGRAD_NSUBJ = 4
WgradCase = namedtuple("WgradCase", "shape dy x")


@functools.lru_cache(maxsize=None)
def wgrad_case(i):
    s = WGRAD_SHAPES[i]
    case = WgradCase(s, ints((s.B, s.cout, s.T), WGRAD_R, 4000 + 10 * i), ints((s.B, s.cin, s.T), WGRAD_R, 4001 + 10 * i))
    assert WGRAD_R * WGRAD_R * s.B * s.T < 2 ** 24
    return case


TypedShape = namedtuple("TypedShape", "M N K")            # out (N, K) = scales . G^T (M, N) Y (M, K)
TYPED_SHAPES = [TypedShape(33, 70, 192), TypedShape(300, 100, 320)]
TypedCase = namedtuple("TypedCase", "shape R G Y sub acc_scale rscale out_scale ref")


def _typed_build(s, seed, R, acc_pool, with_acc=True):
    g = torch.Generator().manual_seed(seed + 7)
    G, Y, sub = ints((s.M, s.N), R, seed), ints((s.M, s.K), R, seed + 1), ints((s.N, s.K), R, seed + 2)
    pool = torch.tensor(acc_pool, dtype=torch.float64)
    acc_scale = pool[torch.randint(0, len(pool), (s.N,), generator=g)] if with_acc else torch.ones(s.N, dtype=torch.float64)
    rscale = torch.randint(-3, 4, (s.N,), generator=g).double()
    out_scale = 2.0
    # sda_wgrad_args / sda_clip_dz: out = out_scale * (acc_scale[j] * acc - rscale[j] * sub[j][k]), one rounding
    ref = out_scale * (acc_scale[:, None] * (G.t() @ Y) - rscale[:, None] * sub)
    return TypedCase(s, R, G, Y, sub, acc_scale, rscale, out_scale, ref)


@functools.lru_cache(maxsize=None)
def typed_case(i, regime, dtype):
    s = TYPED_SHAPES[i]
    key = None if regime == "exact" else dtype
    if key == torch.float32:
        return typed_case(i, regime, torch.bfloat16)
    return _search(lambda R: _typed_build(s, 5000 + 10 * i, R, (0.5, 1.0)), regime, key, f"typed wgrad {tuple(s)}")


# ---------------------------------------------------------------------------------------------------------------
# split-K / similarity GEMM (fp32 result: exact), the loss's dZ, the input gradient, the parameter GEMM
# ---------------------------------------------------------------------------------------------------------------
SimShape = namedtuple("SimShape", "M N K pitch")
SIM_SHAPES = [SimShape(300, 200, 512, 576), SimShape(70, 24, 256, 256 + 64), SimShape(257, 513, 128, 192)]
SIM_R = 15
SIM_KSPLITS = [1, 4]


@functools.lru_cache(maxsize=None)
def sim_case(i):
    s = SIM_SHAPES[i]
    A, Bm = ints((s.M, s.K), SIM_R, 6000 + 10 * i), ints((s.N, s.K), SIM_R, 6001 + 10 * i)
    assert SIM_R * SIM_R * s.K < 2 ** 24
    return A, Bm, matmul_nt_ref(A, Bm)


ClipShape = namedtuple("ClipShape", "Bm Bn F T")
# Bm <= 256 with row_elems % 64 == 0 (coefficients in registers), and Bm >= 256 on 256 x 256 tiles (row_elems % 256 == 0)
CLIP_SHAPES = [ClipShape(33, 64, 192, 9), ClipShape(100, 70, 64, 17), ClipShape(288, 70, 128, 48), ClipShape(512, 256, 64, 44)]
ClipCase = namedtuple("ClipCase", "shape R G Y Z cscale rscale out_scale ref")     # Y (Bm, F, T), Z / ref (Bn, F, T)


@functools.lru_cache(maxsize=None)
def clip_case(i, regime, dtype):
    s = CLIP_SHAPES[i]
    assert dtype in DTYPES16

    def build(R):
        t = _typed_build(TypedShape(s.Bm, s.Bn, s.F * s.T), 7000 + 10 * i, R, (0.5, 1.0))
        sh = lambda v, n: v.reshape(n, s.T, s.F).permute(0, 2, 1).contiguous()        # rows are (t, f) in the row layout
        return ClipCase(s, R, t.G, sh(t.Y, s.Bm), sh(t.sub, s.Bn), t.acc_scale, t.rscale, t.out_scale, sh(t.ref, s.Bn))
    return _search(build, regime, None if regime == "exact" else dtype, f"clip_dz {tuple(s)}")


IgShape = namedtuple("IgShape", "nW Kp C Cp B T")
IG_SHAPES = [IgShape(3, 32, 20, 64, 4, 77), IgShape(2, 96, 70, 128, 3, 130)]
IG_WIDX = [[2, 0, 1, 2], [1, 0, 1]]
IgCase = namedtuple("IgCase", "shape R G W ref")          # G (B, Kp, T), W (nW, Kp, Cp), ref (B, C, T)


@functools.lru_cache(maxsize=None)
def ig_case(i, regime, out_dtype):
    s = IG_SHAPES[i]

    def build(R):
        G, W = ints((s.B, s.Kp, s.T), R, 8000 + 10 * i), ints((s.nW, s.Kp, s.Cp), R, 8001 + 10 * i)
        idx = torch.tensor(IG_WIDX[i])
        ref = torch.einsum("bdc,bdt->bct", W[idx][:, :, :s.C], G)
        return IgCase(s, R, G, W, ref)
    key = None if regime == "exact" else out_dtype
    if key == torch.float32:
        return ig_case(i, regime, torch.bfloat16)
    return _search(build, regime, key, f"input_grad {tuple(s)}")


PGEMM_FORMS = ["a_transposed", "batched_both_sliced", "typed_out_into_view"]
PGEMM_R = 15


def pgemm_operands(form):
    """(A, B) float64 integer tensors in the allocation shapes of the existing strided-view test; the views are cut by the test"""
    shapes = {"a_transposed": ((270, 270), (270, 208)), "batched_both_sliced": ((7, 300, 270), (7, 320, 256)),
              "typed_out_into_view": ((4, 270, 270), (270, 209))}[form]
    seed = 9000 + 10 * PGEMM_FORMS.index(form)
    return ints(shapes[0], PGEMM_R, seed), ints(shapes[1], PGEMM_R, seed + 1)
