"""Inputs, float64 references, tolerances and plain-torch emulations for the kernel-level tests of csrc/elementwise.hip
(the streaming, column-sum and norm passes) and csrc/param_ops.hip (vector maps, slab reduce / unpack, Adam)
(tests/test_elementwise_cpu.py proves on the CPU that the cases catch planted bugs, tests/test_elementwise_gpu.py holds the
HIP kernels to the same comparisons).  Nothing here needs a GPU; every comparison helper works on tensors of any device.

Tolerances (no figure below comes from a kernel's output).  u = 2^-24 is fp32's unit roundoff.
  stored value      one ulp of the storage type at the float64 reference = half an ulp (round to nearest) doubled for a
                    reference that sits on a rounding boundary: ulp().
  sums              an fp32 accumulator that adds n terms is within n u sum|t_i| of the exact sum (running error bound);
                    the terms' own tolerances add up: sum_tol().
  formulas          C * (a magnitude written next to each), where C = 4 x the largest error of the fp32 emulation of the
                    kernel's formula below against float64 on the exhaustive inputs of section 2, with the exp2 and rcp results
                    moved by -1, 0, +1 ulp (the hardware instructions are 1-ulp approximations); 4 covers the device's libm
                    (erff) and instruction selection.  tests/test_elementwise_cpu.py::test_tolerance_table_matches_the_emulation
                    measures the middle column again and holds the constants to it.

      constant   measured on the CPU          chosen (= 4 x measured, rounded up)   magnitude it multiplies
      C_GELU16   1.68e-7 (A-S 7.5e-8 + fp32)  6.8e-7                                max(1, |z|)
      C_GGRAD16  4.08e-7                      1.65e-6                               1 (|GELU'| <= 1.13)
      C_GELU32   9.68e-8                      3.9e-7                                max(1, |z|)
      C_GGRAD32  1.44e-7                      5.8e-7                                1
      C_SIG      4.82 u                       19.5 u                                max(1, |g|) sigmoid(g), + 2^-126 (flush to zero)
      C_BN       4.17 u                       17 u                                  |a g| + |p| + |q x|   (section 4)
      C_ADAM     1.04 u                       4.2 u                                 see adam_tolerances()
"""
import math

import torch

from speech_decoding_amd import lib as L

DTYPES = (torch.float32, torch.bfloat16, torch.float16)
PAD = L.ROW_PAD
SENT = -7.0                       # sentinel of output buffers: representable in every storage type
U32 = 2.0 ** -24

C_GELU16, C_GGRAD16 = 6.8e-7, 1.65e-6
C_GELU32, C_GGRAD32 = 3.9e-7, 5.8e-7
C_SIG = 19.5 * U32
C_BN = 17.0 * U32
C_ADAM = 4.2 * U32
FTZ = 2.0 ** -126                 # a result below fp32's smallest normal may come back as zero


def q(x, dtype):
    """quantise to the storage dtype (what the kernels will actually read), back in float32"""
    return x.to(dtype).float()


def chunk(dtype):
    """elements of a 16-byte chunk = channels one thread owns"""
    return 4 if dtype == torch.float32 else 8


# ---------------------------------------------------------------------------------------------------------------
# tolerances
# ---------------------------------------------------------------------------------------------------------------
_PBITS = {torch.float32: 24, torch.bfloat16: 8, torch.float16: 11}
_EMIN = {torch.float32: -126, torch.bfloat16: -126, torch.float16: -14}


def ulp(ref, dtype):
    """spacing of `dtype` at |ref| (the subnormal spacing below its smallest normal), float64"""
    ref = ref.double()
    _, e = torch.frexp(ref.abs())
    e = torch.where(ref == 0, torch.full_like(e, _EMIN[dtype]), e - 1).clamp(min=_EMIN[dtype])
    return torch.ldexp(torch.ones_like(ref), e - (_PBITS[dtype] - 1))


def ratio(got, ref, tol):
    """max |got - ref| / tol; NaN / Inf in `got` count as infinitely far"""
    got = got.double()
    if not bool(torch.isfinite(got).all()):
        return float("inf")
    if got.numel() == 0:
        return 0.0
    return float(((got - ref.double()).abs() / tol).max())


def sum_tol(terms, term_tol, n_acc, dim=0):
    """tolerance of an fp32 sum of `terms` whose accumulators see at most n_acc additions; term_tol: the terms' own tolerances"""
    s = terms.double().sum(dim)
    return term_tol.double().expand_as(terms).sum(dim) + n_acc * U32 * terms.double().abs().sum(dim) + ulp(s, torch.float32)


# float64 forms
def phi64(x):
    return 0.5 * torch.special.erfc(-x.double() / math.sqrt(2.0))


def gelu64(x):
    return x.double() * phi64(x)


def ggrad64(x):
    x = x.double()
    return phi64(x) + x * torch.exp(-0.5 * x * x) / math.sqrt(2.0 * math.pi)


def sig64(x):
    return torch.sigmoid(x.double())


def gelu_budget(z, dtype):
    return (C_GELU32 if dtype == torch.float32 else C_GELU16) * z.double().abs().clamp(min=1.0)


def ggrad_budget(dtype):
    return C_GGRAD32 if dtype == torch.float32 else C_GGRAD16


def sig_tol(g):
    g = g.double()
    return C_SIG * g.abs().clamp(min=1.0) * sig64(g) + FTZ


# ---------------------------------------------------------------------------------------------------------------
# fp32 emulation of the device formulas (sd_common.h).  hw = (ulps added to every exp2 result, to every rcp result).
# ---------------------------------------------------------------------------------------------------------------
def _f(x):
    return x.to(torch.float32)


def _fma(a, b, c):
    return (a.double() * b.double() + c.double()).float()         # the product of two fp32 is exact in fp64


def _nudge(x, k):
    """k ulps up or down; 0 and inf (exp2 of a large argument, rcp of inf or of 0) are exact on the device and stay"""
    y = x
    for _ in range(abs(k)):
        y = torch.nextafter(y, torch.full_like(y, math.inf if k > 0 else -math.inf))
    return torch.where((x == 0) | torch.isinf(x), x, y)


def _exp2(x, hw):
    return _nudge(torch.exp2(x.double()).float(), hw[0])


def _rcp(x, hw):
    return _nudge((1.0 / x.double()).float(), hw[1])


def _c(v):
    return torch.tensor(v, dtype=torch.float32)


def normal_tail(x, hw, mutant=None):
    y = x * _c(0.849321800288)
    e = _exp2(-(y * y), hw)
    t = _rcp(_fma(x.abs(), _c(0.2316419), _c(1.0)), hw)
    qq = _fma(t, _c(0.5) * _c(1.061405429), _c(0.5) * _c(-1.453152027))
    qq = _fma(qq, t, _c(0.5) * _c(1.421413741))
    qq = _fma(qq, t, _c(0.5) * _c(-0.284496736))
    qq = _fma(qq, t, _c(0.5) * _c(0.254829592))
    tail = (qq * t) * e
    if mutant == "tail_without_e":                                 # mutant 6
        tail = torch.where(x.abs() > 4, qq * t, tail)
    return tail, e


def _tanh_gelu(x):
    return (0.5 * x.double() * (1.0 + torch.tanh(math.sqrt(2.0 / math.pi) * (x.double() + 0.044715 * x.double() ** 3)))).float()


def gelu_emul(x, dtype, hw=(0, 0), mutant=None):
    x = _f(x)
    if mutant == "tanh_gelu":                                      # mutant 5
        return _tanh_gelu(x)
    if dtype == torch.float32:
        return _c(0.5) * x * (_c(1.0) + torch.erf(x * _c(0.70710678118654752)))
    tail, _ = normal_tail(x, hw, mutant)
    return _fma(-x.abs(), tail, x.clamp(min=0.0))


def ggrad_emul(x, dtype, hw=(0, 0), mutant=None):
    x = _f(x)
    if dtype == torch.float32:
        cdf = _c(0.5) * (_c(1.0) + torch.erf(x * _c(0.70710678118654752)))
        pdf = _c(0.3989422804014327) * _exp2((_c(-0.5) * x * x) * _c(1.4426950408889634), hw)
        out = cdf + x * pdf
    else:
        tail, e = normal_tail(x, hw, mutant)
        h = _c(0.5) - tail
        out = _fma(x * _c(0.3989422804014327), e, torch.copysign(h, x) + _c(0.5))
    if mutant == "ggrad_sign":                                     # mutant 7: Phi(|x|) + x phi(x) on the negative side
        out = torch.where(x < 0, (1.0 - phi64(x)).float() + (out - phi64(x).float()), out)
    return out


def sigmoid_emul(x, hw=(0, 0)):
    x = _f(x)
    return _rcp(_c(1.0) + _exp2((-x) * _c(1.4426950408889634), hw), hw)


HW_VARIANTS = ((0, 0), (1, 1), (1, -1), (-1, 1), (-1, -1))


# ---------------------------------------------------------------------------------------------------------------
# row layout and the kernels' row partition
# ---------------------------------------------------------------------------------------------------------------
def mem_rows(B, T):
    """memory row of valid row r = b T + t"""
    r = torch.arange(B * T)
    return (r // T) * L.rows_tp(T) + PAD + r % T


def to_rl(valid, B, T, fill=0.0):
    """(B T, W) values -> (rows_alloc, W) row-layout image, every other row `fill`"""
    out = torch.full((L.rows_alloc(B, T), valid.shape[1]), fill, dtype=valid.dtype)
    out[mem_rows(B, T)] = valid
    return out


def row_group(nch):
    return 1 if nch >= 256 else 256 // nch


def stream_blocks(B, T, nch):
    nb = (B * T + row_group(nch) * 8 - 1) // (row_group(nch) * 8)
    return max(1, min(2048, nb))


def red_blocks(B, T):
    return max(1, min(1024, (B * T + 31) // 32))


def cursor_count(r0, r1, rg, RG):
    """RowCursor::n"""
    first = r0 + rg
    return (r1 - first + RG - 1) // RG if first < r1 else 0


def thread_rows(first, n, RG, T, mutant=None):
    """memory rows a thread takes: RowCursor / RowWalk from valid row `first`, n rows, stride RG"""
    b, t = divmod(first, T)
    row, out = b * L.rows_tp(T) + PAD + t, []
    for _ in range(n):
        out.append(row)
        row += RG
        t += RG
        if mutant == "pad_once_per_step":                          # mutant 1: `if` for `while`
            if t >= T:
                t -= T
                row += PAD
        else:
            while t >= T:
                t -= T
                row += PAD
    return out


def block_range(rows, nb, blk, mutant=None):
    per = (rows + nb - 1) // nb
    r0 = min(rows, blk * per)
    r1 = min(rows, r0 + per)
    if mutant == "drop_last_row" and r1 > r0:                      # mutant 2
        r1 -= 1
    return r0, r1


def stream_mask(B, T, W, dtype, U, mutant=None):
    """bool (rows_alloc, W) image of the elements a streaming kernel of W-wide rows writes; asserts that no element is
    written twice and none outside the buffer"""
    CH = chunk(dtype)
    nch, rows = W // CH, B * T
    RG, nb = row_group(nch), stream_blocks(B, T, nch)
    hit = torch.zeros((L.rows_alloc(B, T), nch), dtype=torch.int32)
    for blk in range(nb):
        r0, r1 = block_range(rows, nb, blk, mutant)
        for tid in range(256):
            for c in range(tid, RG * nch, 256):
                if mutant == "drop_second_pass" and c >= 256:      # mutant 4
                    continue
                ch, rg = c % nch, c // nch
                n = cursor_count(r0, r1, rg, RG)
                if mutant == "drop_batch_remainder":               # mutant 3
                    n -= n % U
                for row in thread_rows(r0 + rg, n, RG, T, mutant):
                    assert row < hit.shape[0]
                    hit[row, ch] += 1
    assert int(hit.max()) <= 1
    return hit.bool().repeat_interleave(CH, dim=1)


def reduce_rows(B, T, W, dtype, mutant=None):
    """[block][row group] -> memory rows, for col_reduce_kernel / bwd_colsum_kernel on W-wide rows"""
    nch, rows, nb = W // chunk(dtype), B * T, red_blocks(B, T)
    RG = 256 // nch
    out = []
    for blk in range(nb):
        r0, r1 = block_range(rows, nb, blk, mutant)
        out.append([thread_rows(r0 + rg, cursor_count(r0, r1, rg, RG), RG, T, mutant) for rg in range(RG)])
    return out


def reduce_n_acc(B, T, W, dtype):
    """additions an fp32 accumulator of the two-stage column sum sees at most: a thread's rows, then the row groups"""
    RG = 256 // (W // chunk(dtype))
    per = (B * T + red_blocks(B, T) - 1) // red_blocks(B, T)
    return (per + RG - 1) // RG + RG


def final_reduce(partial, mutant=None):
    """block_partial_sums: (n, Cp) fp32 partial rows -> fp32"""
    if mutant == "fp32_final":                                     # mutant 10
        s = torch.zeros(partial.shape[1:], dtype=torch.float32)
        for k in range(partial.shape[0]):
            s = s + partial[k]
        return s
    if mutant == "first_128_rows":                                 # mutant 11
        partial = partial[:128]
    return partial.double().sum(0).float()


def emul_colsum(rl_terms, B, T, dtype, mutant=None):
    """two-stage ordered column sum of the fp32 row-layout image `rl_terms` (what each thread adds per row), as the kernels do
    it: per thread in row order, row groups in order, blocks in fp64"""
    W = rl_terms.shape[1]
    parts = []
    for groups in reduce_rows(B, T, W, dtype, mutant):
        s = torch.zeros(W, dtype=torch.float32)
        for rows_ in groups:
            a = torch.zeros(W, dtype=torch.float32)
            for r in rows_:
                a = a + rl_terms[r]
            s = s + a
        parts.append(s)
    return final_reduce(torch.stack(parts), mutant)


STREAM_SHAPES = ((1, 1, 64), (7, 5, 64), (5, 33, 128), (3, 77, 320), (2, 9, 1024))
WIDE_SHAPE = {torch.float32: (2, 5, 1088), torch.bfloat16: (2, 5, 2112), torch.float16: (2, 5, 2112)}
REDUCE_SHAPES = STREAM_SHAPES + ((7, 5, 128),) + tuple((3, 11, w) for w in range(64, 1025, 64))


def stream_cap_shape(dtype):
    """more than 2048 x 8 x RG rows at width 64 (the narrowest): 67 MB per 64-wide buffer in every dtype"""
    RG = row_group(64 // chunk(dtype))
    T = 2048 * 8 * RG // 3 + 1
    return (3, T, 64)


REDUCE_CAP_SHAPE = (3, 10923, 64)          # 32 769 rows > 1024 blocks x 32


def thread_row_counts(B, T, W, dtype):
    """every RowCursor::n of a streaming launch"""
    nch = W // chunk(dtype)
    RG, nb = row_group(nch), stream_blocks(B, T, nch)
    return {cursor_count(*block_range(B * T, nb, blk), rg, RG) for blk in range(nb) for rg in range(RG)}


# ---------------------------------------------------------------------------------------------------------------
# section 1 / 2: elementwise cases.  A case is a dict of fp32 (already quantised) valid-row operands; refs are float64.
# ---------------------------------------------------------------------------------------------------------------
def _gen(seed):
    return torch.Generator().manual_seed(seed)


def real_operands(rows, C, dtype, seed=0):
    g = _gen(seed)
    d = dict(x=q(torch.randn(rows, C, generator=g) * 2.0, dtype), d=q(torch.randn(rows, C, generator=g), dtype),
             val=q(torch.randn(rows, C, generator=g) * 1.5, dtype), gate=q(torch.randn(rows, C, generator=g) * 3.0, dtype),
             scale=torch.randn(C, generator=g), shift=torch.randn(C, generator=g) * 0.5)
    return d


def integer_operands(rows, C, seed=1):
    """operands on which every product and sum of the fused backward passes is a small integer: GELU' is exactly 1 / 0 at
    +-32 (the density's exp2 underflows to 0 exactly) and sigmoid exactly 1 / 0 at +-100 (1 + tiny = 1 and 1 + inf = inf; rcp(inf) = 0,
    and rcp(1) = 1: a 1-ulp reciprocal is exact at a power of two)"""
    g = _gen(seed)
    ri = lambda lo, hi: torch.randint(lo, hi + 1, (rows, C), generator=g).float()
    sign = lambda: torch.randint(0, 2, (rows, C), generator=g).float() * 2 - 1
    return dict(x=32.0 * sign(), d=ri(-3, 3), val=ri(-4, 4), gate=100.0 * sign())


def ref_bn_gelu_forward(x, scale, shift, dtype):
    z = x.double() * scale.double() + shift.double()
    ref = gelu64(z)
    return ref, 1.13 * U32 * z.abs() + gelu_budget(z, dtype) + ulp(ref, dtype)


def ref_gelu_backward(u, dz, dtype):
    ref = dz.double() * ggrad64(u)
    return ref, dz.double().abs() * ggrad_budget(dtype) + U32 * ref.abs() + ulp(ref, dtype)


def ref_glu_forward(val, gate, dtype):
    ref = val.double() * sig64(gate)
    return ref, val.double().abs() * sig_tol(gate) + U32 * ref.abs() + ulp(ref, dtype)


def ref_glu_backward(val, gate, dy, dtype, unstored=False):
    """[d value | d gate]; unstored: the fp32 values before the store (what the fused column sums add)"""
    sg, da_ = sig64(gate), dy.double() * val.double()
    da, dg = dy.double() * sg, da_ * sg * (1 - sg)
    ta = dy.double().abs() * sig_tol(gate) + U32 * da.abs()
    tg = da_.abs() * (sig_tol(gate) + 4 * U32 * sg * (1 - sg))
    ref, tol = torch.cat([da, dg], 1), torch.cat([ta, tg], 1)
    return ref, tol if unstored else tol + ulp(ref, dtype)


def ref_glu_backward_og(out, gate, dy, dtype, unstored=False):
    sg, do_ = sig64(gate), dy.double() * out.double()
    da, dg = dy.double() * sg, do_ * (1 - sg)
    ta = dy.double().abs() * sig_tol(gate) + U32 * da.abs()
    tg = do_.abs() * (sig_tol(gate) + 3 * U32 * (1 - sg))
    ref, tol = torch.cat([da, dg], 1), torch.cat([ta, tg], 1)
    return ref, tol if unstored else tol + ulp(ref, dtype)


# emulations of the same passes on valid rows (fp32 in, fp32 before the store out)
def emul_bn_gelu_forward(x, scale, shift, dtype, hw=(0, 0), mutant=None):
    return gelu_emul(_fma(_f(x), scale, shift), dtype, hw, mutant)


def emul_gelu_backward(u, dz, dtype, hw=(0, 0), mutant=None):
    return _f(dz) * ggrad_emul(u, dtype, hw, mutant)


def emul_glu_forward(val, gate, hw=(0, 0)):
    return _f(val) * sigmoid_emul(gate, hw)


def emul_glu_backward(val, gate, dy, hw=(0, 0), mutant=None):
    sg = sigmoid_emul(gate, hw)
    one_m = _c(1.0) - sg
    dg = _f(dy) * _f(val) * sg * one_m
    if mutant == "sig_grad_squared":                               # mutant 8
        dg = dg * one_m
    return torch.cat([_f(dy) * sg, dg], 1)


def emul_glu_backward_og(out, gate, dy, hw=(0, 0), mutant=None, val=None):
    sg = sigmoid_emul(gate, hw)
    src = _f(val) if mutant == "og_uses_value" else _f(out)        # mutant 9
    return torch.cat([_f(dy) * sg, _f(dy) * src * (_c(1.0) - sg)], 1)


def finite_values(dtype):
    """every finite bit pattern of a 16-bit type, as float32 (65 280 of bf16, 63 488 of fp16)"""
    bits = torch.arange(-32768, 32768, dtype=torch.int32).to(torch.int16)
    v = bits.view(dtype).float()
    return v[torch.isfinite(v)]


def loguniform_values(n=65536, seed=5):
    g = _gen(seed)
    mag = torch.exp(torch.empty(n, dtype=torch.float64).uniform_(math.log(1e-30), math.log(1e30), generator=g))
    sign = torch.randint(0, 2, (n,), generator=g).double() * 2 - 1
    return (mag * sign).float()


def sweep_sets(dtype):
    """name -> (1024, 64) fp32 image of the inputs of the exhaustive sweep for a storage dtype (unused slots 0)"""
    def image(v):
        out = torch.zeros(65536)
        out[:v.numel()] = v
        return out.reshape(1024, 64)
    if dtype == torch.float32:
        return {"bf16": image(finite_values(torch.bfloat16)), "fp16": image(finite_values(torch.float16)),
                "loguniform": image(loguniform_values())}
    return {str(dtype): image(finite_values(dtype))}


TINY = {torch.float32: 2.0 ** -126, torch.bfloat16: 2.0 ** -126, torch.float16: 2.0 ** -14}


# ---------------------------------------------------------------------------------------------------------------
# section 3: bn_finalize on given partials
# ---------------------------------------------------------------------------------------------------------------
NTILES = (1, 2, 127, 128, 129, 300, 1024)
ROWS_PER_TILE = 8


def exact_partials(ntiles, Cp, seed=7):
    """(ntiles, 2, Cp) fp32: multiples of 2^-20 below 2^10 — 1024 of them need 40 bits: exact in fp64, not in fp32"""
    g = _gen(seed + ntiles + Cp)
    return (torch.randint(-2 ** 29, 2 ** 29, (ntiles, 2, Cp), generator=g).double() * 2.0 ** -20).float()


def bn_partials(ntiles, C, Cp, seed=11):
    """Per-tile (sum x, sum x^2) of ROWS_PER_TILE rows each.  Channel 0: ordinary.  1: mean = 1000 std.  2: constant 3 (sum 3 n,
    sum of squares 9 n: q / N - mean^2 is exactly 0 in any evaluation order).  3: as 2 with 2^-10 added to the first tile's sum:
    q / N - mean^2 = -(6 d + d^2) < 0, d = 2^-10 / N.  >= 4: ordinary.  Channels >= C hold junk the kernel must not pass on."""
    g = _gen(seed + ntiles)
    n = ROWS_PER_TILE
    x = torch.randn(ntiles, n, Cp, generator=g, dtype=torch.float64) * 1.5 + 0.3
    x[:, :, 1] = 1000.0 + torch.randn(ntiles, n, generator=g, dtype=torch.float64)
    part = torch.stack([x.sum(1), (x * x).sum(1)], 1).float()
    part[:, 0, 2], part[:, 1, 2] = 3.0 * n, 9.0 * n
    part[:, 0, 3], part[:, 1, 3] = 3.0 * n, 9.0 * n
    part[0, 0, 3] += 2.0 ** -10
    part[:, :, C:] = 5.0
    return part


def bn_params(C, seed=13):
    g = _gen(seed)
    return dict(gamma=torch.randn(C, generator=g), beta=torch.randn(C, generator=g), running_mean=torch.randn(C, generator=g),
                running_var=torch.rand(C, generator=g) + 0.5)


def ref_bn_finalize(part, count, p, C, Cp, training, eps=1e-5, momentum=0.1, mutant=None):
    """float64 on the fp32 partials, in the kernel's order of operations.  Returns dict of float64 (Cp,) / (C,) tensors."""
    gamma, beta = p["gamma"].double(), p["beta"].double()
    rm, rv = p["running_mean"].double(), p["running_var"].double()
    eps, momentum = float(torch.tensor(eps, dtype=torch.float32)), float(torch.tensor(momentum, dtype=torch.float32))
    if training:
        s = part.double().sum(0)
        mean = s[0, :C] / count
        var = s[1, :C] / count - mean * mean
        if mutant != "no_clamp":                                   # mutant 12
            var = var.clamp(min=0.0)
        unb = var * count / (count - 1.0) if count > 1 else var
        rm, rv = (1.0 - momentum) * rm + momentum * mean, (1.0 - momentum) * rv + momentum * unb
        if mutant == "unbiased_norm":                              # mutant 13
            var = unb
    else:
        mean, var = rm, rv
    rstd = 1.0 / torch.sqrt(var + eps)
    sc = gamma * rstd
    pad = lambda v: torch.cat([v, torch.zeros(Cp - C, dtype=torch.float64)])
    return dict(mean=pad(mean), rstd=pad(rstd), scale=pad(sc), shift=pad(beta - mean * sc), running_mean=rm, running_var=rv,
                coef=torch.stack([pad(gamma), pad(beta), pad(mean), pad(rstd)]))


def within_one_ulp(got, ref):
    """fp32 `got` within one fp32 ulp of float64 `ref` (the kernel works in double and rounds once; NaN fails)"""
    got = got.double().cpu()
    return bool(((got - ref).abs() <= ulp(ref, torch.float32)).all())


# ---------------------------------------------------------------------------------------------------------------
# section 4: BatchNorm + GELU backward
# ---------------------------------------------------------------------------------------------------------------
BN_RATIOS = (0.0, 1.0, 30.0, 300.0)


def bn_backward_case(B, T, C, dtype, designed, seed=17):
    """x (rows, C) with per-channel mean / std, dy, gamma, beta.  designed: channel c has mean / std = BN_RATIOS[c % 4], gamma of
    both signs and gamma[5] = 0; else mean / std = 0.3 everywhere."""
    g = _gen(seed + B * T + C)
    rows = B * T
    std = torch.rand(C, generator=g) + 0.5
    mr = torch.tensor([BN_RATIOS[c % 4] for c in range(C)]) if designed else torch.full((C,), 0.3)
    x = q(torch.randn(rows, C, generator=g) * std + mr * std, dtype)
    dy = q(torch.randn(rows, C, generator=g), dtype)
    gamma, beta = torch.randn(C, generator=g), torch.randn(C, generator=g) * 0.5
    if designed:
        gamma[5] = 0.0
    return dict(x=x, dy=dy, gamma=gamma, beta=beta)


def ref_bn_backward(case, dtype, dg_form, weight=None, n_acc=None, eps=1e-5):
    """float64 backward of gelu(batch_norm(x)) (dg_form: of batch_norm(x) alone, with the stored dg as the incoming gradient):
    the closed form, checked here against float64 autograd whenever autograd can run (more than one row, no weights).
    weight: how often each row of the case occurs in the batch (a batch tiled from a short pattern).  n_acc: additions an fp32
    accumulator of the sums sees (default: all rows on one).  Returns the per-row
    operands of each form, dx, dgamma, dbeta and their tolerances."""
    eps = float(torch.tensor(eps, dtype=torch.float32))
    x, dy, gamma, beta = case["x"].double(), case["dy"].double(), case["gamma"].double(), case["beta"].double()
    w = torch.ones(x.shape[0], 1, dtype=torch.float64) if weight is None else weight.double().reshape(-1, 1)
    N = float(w.sum())
    mean = (w * x).sum(0) / N
    var = (w * (x - mean) ** 2).sum(0) / N
    rstd = 1.0 / torch.sqrt(var + eps)
    xhat = (x - mean) * rstd
    z = gamma * xhat + beta
    dg = q(dy * ggrad64(z), dtype).double() if dg_form else dy * ggrad64(z)      # dg_form: what a conv epilogue stored
    dbeta, dgamma = (w * dg).sum(0), (w * dg * xhat).sum(0)
    a = gamma * rstd
    dx = a * (dg - dbeta / N - xhat * dgamma / N)
    if weight is None and x.shape[0] > 1:
        xa, ga, ba = x.clone().requires_grad_(True), gamma.clone().requires_grad_(True), beta.clone().requires_grad_(True)
        y = torch.nn.functional.batch_norm(xa, None, None, ga, ba, training=True, eps=eps)
        if dg_form:
            y.backward(dg)
        else:
            torch.nn.functional.gelu(y).backward(dy)
        scale = lambda t: float(t.abs().max()) + 1e-300
        assert float((xa.grad - dx).abs().max()) <= 1e-9 * max(scale(a * dg), scale(dx)), "closed form against autograd"
        assert float((ga.grad - dgamma).abs().max()) <= 1e-10 * scale((dg * xhat).abs().sum(0))
        assert float((ba.grad - dbeta).abs().max()) <= 1e-10 * scale(dg.abs().sum(0))
        dx, dgamma, dbeta = xa.grad, ga.grad, ba.grad
    qq = a * rstd * dgamma / N
    p = a * dbeta / N - qq * mean
    # The kernels are handed mean and rstd as fp32, so xhat carries dxh = u (|mean| rstd + |xhat|) whatever they do.  Column
    # sums: the terms' own tolerance (GELU' budget and dxh through GELU'' <= 0.8), then the accumulation.
    dxh = U32 * (mean.abs() * rstd + xhat.abs())
    t_dg = torch.zeros_like(dg) if dg_form else dy.abs() * (ggrad_budget(dtype) + 4 * U32 + 0.8 * gamma.abs() * dxh) + U32 * dg.abs()
    n_acc = N + 1 if n_acc is None else n_acc
    tol_db = sum_tol(w * dg, w * t_dg, n_acc)
    tol_dgam = sum_tol(w * dg * xhat, w * (t_dg * xhat.abs() + dg.abs() * dxh + 4 * U32 * (dg * xhat).abs()), n_acc)
    b = beta - a * mean
    tol = C_BN * ((a * dg).abs() + p.abs() + (qq * x).abs()) + 2 * U32 * (qq * mean).abs() + a.abs() * (tol_db + xhat.abs() * tol_dgam) / N
    if not dg_form:                                                # GELU' at a x + b, evaluated in fp32 (|GELU''| <= 0.8)
        tol = tol + (a * dy).abs() * (ggrad_budget(dtype) + 0.8 * C_BN * ((a * x).abs() + b.abs()))
    tol = tol + ulp(dx, dtype)
    return dict(dx=dx, tol=tol, dgamma=dgamma, dbeta=dbeta, tol_dgamma=tol_dgam, tol_dbeta=tol_db, dg=dg, xhat=xhat,
                mean=mean, rstd=rstd, a=a, p=p, q=qq, N=N)


def emul_bn_backward_apply(case, mean, rstd, dgamma, dbeta, dtype, dg_form, dg=None, hw=(0, 0), mutant=None):
    """bn_bwd_coef_kernel + bn_gelu_bwd_apply_kernel on valid rows, fp32: mean, rstd, dgamma, dbeta as fp32 (C,) tensors"""
    inv = torch.tensor(1.0 / case["x"].shape[0], dtype=torch.float32)
    ga, be, mu, rs = _f(case["gamma"]), _f(case["beta"]), _f(mean), _f(rstd)
    c4, c5 = _f(dbeta) * inv, _f(dgamma) * inv
    if mutant == "swap_dgamma_dbeta":                              # mutant 15
        c4, c5 = c5, c4
    ca = ga * rs
    cb = be - ca * mu
    cq = ca * rs * c5
    cp = ca * c4 if mutant == "p_without_q_mean" else ca * c4 - cq * mu     # mutant 14
    x = _f(case["x"])
    g = _f(dg) if dg_form else _f(case["dy"]) * ggrad_emul(_fma(ca, x, cb), dtype, hw)
    return _fma(ca, g, -_fma(cq, x, cp))


# ---------------------------------------------------------------------------------------------------------------
# section 5: weight-gradient reduce / unpack and vector maps
# ---------------------------------------------------------------------------------------------------------------
WGRAD_NSLABS = (1, 7, 8, 9, 17)
WGRAD_KS = (1, 3)
WGRAD_SHAPES = ((48, 40, 0, 0), (320, 270, 0, 0), (70, 64, 0, 0), (600, 64, 300, 320))     # (Cout, Cin, glu_half, glu_half_p)


def glu_map(co, half, half_p):
    return co if (half == 0 or co < half) else half_p + co - half


def wgrad_case(nslabs, KS, Cout, Cin, half, half_p, seed=19):
    """integer-valued slabs (nslabs, KS, Cout_p, Cin_p): any summation order is exact; pad rows / columns hold 99"""
    g = _gen(seed + nslabs + KS + Cout)
    Cin_p = L.pad_channels(Cin)
    Cout_p = L.pad_channels(half_p + Cout - half) if half else L.pad_channels(Cout)
    return torch.randint(-8, 9, (nslabs, KS, Cout_p, Cin_p), generator=g).float()


def ref_reduce_unpack(slabs, Cout, Cin, KS, half=0, half_p=0, mutant=None):
    """dst[co][ci][tap] = sum_s slabs[s][tap][map(co)][ci], a plain loop over (co, tap)"""
    out = torch.zeros(Cout, Cin, KS, dtype=torch.float64)
    for co in range(Cout):
        row = glu_map(co, half, half if mutant == "half_for_half_p" else half_p)       # mutant 17
        for tap in range(KS):
            out[co, :, tap] = slabs[:, tap, row, :Cin].double().sum(0)
    return out.float()


def emul_reduce_unpack_vec(slabs, Cout, Cin, KS, half=0, half_p=0, mutant=None):
    """reduce_unpack_wgrad_vec_kernel: four input channels per thread, written at stride KS"""
    total = slabs.sum(0)
    out = torch.full((Cout * Cin * KS + 4 * KS,), SENT)
    for co in range(Cout):
        row = glu_map(co, half, half_p)
        for tap in range(KS):
            for c4 in range(Cin // 4):
                base = (co * Cin + 4 * c4) * KS + tap
                idx = [base, base + (1 if mutant == "o1_for_oKS" else KS), base + 2 * KS, base + 3 * KS]    # mutant 16
                for j in range(4):
                    out[idx[j]] = total[tap, row, 4 * c4 + j]
    return out[:Cout * Cin * KS].reshape(Cout, Cin, KS)


# ---------------------------------------------------------------------------------------------------------------
# section 6: per-sample norms
# ---------------------------------------------------------------------------------------------------------------
SUMSQ_ROW_ELEMS = (4, 252, 256, 65540)
SUMSQ_B = (1, 65)


def sumsq_n_acc(row_elems):
    """additions one fp32 accumulator of rows_sumsq sees: 4 products per 16-byte load of its chunk, 6 wave-shuffle levels, 3 waves"""
    n4 = row_elems // 4
    per = (n4 + 63) // 64
    return 4 * ((per + 255) // 256) + 6 + 3


# ---------------------------------------------------------------------------------------------------------------
# section 7: Adam
# ---------------------------------------------------------------------------------------------------------------
ADAM_BIG = 262144 + 1029
ADAM_STEPS = (1, 2, 7)


def adam_grads(names, steps, seed=23):
    """name -> list over steps of fp32 gradients (None: no gradient that step); magnitudes 1e-12 .. 1e12 per tensor"""
    g = _gen(seed)
    shapes = dict(big=(ADAM_BIG,), three=(3,), cplx=(5, 7, 2), offset=(1001,), late=(130,), never=(9,), zero=(33,))
    mags = dict(big=1.0, three=1e-12, cplx=1e12, offset=1e-3, late=1e6, never=1.0, zero=0.0)
    out = {}
    for name in names:
        seq = []
        for k in range(1, steps + 1):
            if name == "never" or (name == "late" and k < 3):
                seq.append(None)
            else:
                seq.append(torch.randn(shapes[name], generator=g) * mags[name])
        out[name] = seq
    return out, shapes


def adam_tolerances(grads, p0, m0, v0, step0, lr=1e-3, b1=0.9, b2=0.999, eps=1e-8):
    """Running-error bounds of the fp32 update against float64 Adam after each step, as (tol_p, tol_m, tol_v) per step.
    exp_avg: k roundings on a sum whose magnitude recurrence is M_k = b1 M_(k-1) + (1 - b1) |g_k|.  exp_avg_sq: the same on
    positive terms, plus the betas' own format: the C ABI takes them as fp32, and 1 - fl32(b) differs from 1 - b by up to
    2^-25 b / (1 - b) relative (1.3e-5 for 0.999: the injected term (1 - b2) g^2 carries it; the bias correction is computed
    from the same fl32(b), so the parameters do not).  Parameter: every step's update u_k = lr mhat / (sqrt(vhat) + eps) carries
    the relative error of m (against its magnitude) and half that of v, six roundings of its own, and one rounding of p."""
    beta_rel = lambda b: 2.0 ** -25 * b / (1.0 - b)
    p, M, v = p0.double().abs(), m0.double().abs(), v0.double()
    tm, tv = torch.zeros_like(p), torch.zeros_like(p)
    tp = torch.zeros_like(p)
    out, k = [], step0
    for g in grads:
        if g is None:
            out.append(None)
            continue
        k += 1
        g = g.double().reshape(p.shape)
        tm = b1 * tm + (C_ADAM + beta_rel(b1)) * (b1 * M + (1 - b1) * g.abs())
        M = b1 * M + (1 - b1) * g.abs()
        tv = b2 * tv + (C_ADAM + beta_rel(b2)) * (b2 * v + (1 - b2) * g * g)
        v = b2 * v + (1 - b2) * g * g
        bc1, bc2 = 1 - b1 ** k, 1 - b2 ** k
        denom = torch.sqrt(v / bc2) + eps
        step_size = lr / bc1
        u = step_size * M / denom
        tu = step_size * tm / denom + u * (0.5 * tv / v.clamp(min=1e-300) + 6 * C_ADAM)
        p = p + u
        tp = tp + tu + C_ADAM * p
        out.append((tp.clone() + 1e-300, tm.clone() + 1e-300, tv.clone() + 1e-300))
    return out


def emul_adam(p, g, m, v, step, lr=1e-3, b1=0.9, b2=0.999, eps=1e-8, mutant=None):
    """adam_multi_kernel on one flat fp32 tensor; returns (p, m, v)"""
    b1f, b2f = _c(b1), _c(b2)
    kk = step - 1 if mutant == "bias_step_minus_1" else step                           # mutant 20
    bc1 = _c(1.0 - float(b1f) ** kk)
    bc2s = _c(math.sqrt(1.0 - float(b2f) ** kk))
    step_size = _c(lr) / bc1
    m2 = b1f * m + (_c(1.0) - b1f) * g
    v2 = b2f * v + (_c(1.0) - b2f) * g * g
    if mutant == "eps_in_sqrt":                                                        # mutant 21
        den = torch.sqrt(v2 + _c(eps)) / bc2s
    else:
        den = torch.sqrt(v2) / bc2s + _c(eps)
    p2 = p - step_size * (m2 / den)
    n = p.numel()
    keep = torch.zeros(n, dtype=torch.bool)
    if mutant == "skip_second_trip":                                                   # mutant 18
        keep[256 * 1024:] = True
    if mutant == "skip_tail":                                                          # mutant 19
        keep[n - n % 4:] = True
    return torch.where(keep, p, p2), torch.where(keep, m, m2), torch.where(keep, v, v2)
