"""Inputs, float64 references and CPU emulations for the kernel-level tests of the wav2vec 2.0 embedder's HIP kernels
(csrc/w2v2.hip), shared by tests/test_w2v2_kernels_cpu.py (which proves on the CPU that the designed inputs tell a subtly
wrong kernel from a right one) and tests/test_w2v2_kernels_gpu.py (which runs them on the kernels).

Everything here is plain torch on the CPU.  Operands are quantised to the compute dtype first (`q`), so a float64
reference sees exactly what a kernel reads."""
import math

import torch
import torch.nn.functional as TF

DTYPES = [torch.float32, torch.bfloat16, torch.float16]
ATT_T = [1, 15, 16, 17, 63, 64, 65, 127, 128, 129, 200]
ATT_HEADS = [1, 3]
HD = 64                       # head dimension of sda_w2v_attention
KB = 64                       # keys per block of its online softmax
TAIL = 1e4                    # |value| of the V^T tail columns ("anything finite"; below fp16's 65504)
ATT_MUTANTS = ["drop_tail_key", "no_rescale", "tail_v_used", "no_scale", "head_shift"]


def q(x, dtype):
    """quantise to the compute dtype (what the kernels will actually read), back in float32"""
    return x.to(dtype).float()


def ceil64(n):
    return (n + 63) // 64 * 64


def tol_ratio(got, ref, rtol, atol):
    """max |got - ref| / (atol + rtol |ref|): <= 1 passes an allclose with these tolerances; NaN / Inf count as infinitely far"""
    got, ref = got.double(), ref.double()
    if not bool(torch.isfinite(got).all()):
        return float("inf")
    return float(((got - ref).abs() / (atol + rtol * ref.abs())).max())


# ---------------------------------------------------------------------------------------------------------------
# attention
# ---------------------------------------------------------------------------------------------------------------
def _designed(c):
    """q = 8 e0, k_j = c_j e0 for one head: with scale 1/8 the logit of key j is exactly c_j in every dtype (the c_j used here
    are small integers: exact in bf16's 8 bits)."""
    T = c.shape[0]
    qh, kh = torch.zeros(T, HD), torch.zeros(T, HD)
    qh[:, 0] = 8.0
    kh[:, 0] = c
    return qh, kh


def _ramp(T, falling):
    j = torch.arange(T)
    blk = j // KB
    if falling:
        blk = (T - 1) // KB - blk
    return (24 * blk + j % 3).float()          # more than 20 from block to block, three distinct values inside one


def _dominant(T, at):
    c = (torch.arange(T) % 3).float()
    c[at] = 30.0
    return c


def attention_cases(T, heads):
    """[(name, q (heads, T, 64), k (heads, T, 64), v (heads, T, 64))] float32, not yet quantised.  Every key has its own V row."""
    g = torch.Generator().manual_seed(1000 * T + heads)
    v = torch.randn(heads, T, HD, generator=g)
    out = []

    def same(name, c):
        qh, kh = _designed(c)
        out.append((name, qh.expand(heads, T, HD).clone(), kh.expand(heads, T, HD).clone(), v))
    same("a_rising", _ramp(T, False))
    same("b_falling", _ramp(T, True))
    same("c_last_key", _dominant(T, T - 1))
    if T > 63:
        same("d_key63", _dominant(T, 63))
    if T > 64:
        same("d_key64", _dominant(T, 64))
    for std in (1.0, 4.0):                      # q . k / 8 has std sigma_q sigma_k
        qr = torch.randn(heads, T, HD, generator=g) * math.sqrt(std)
        kr = torch.randn(heads, T, HD, generator=g) * math.sqrt(std)
        out.append((f"e_random_std{std:g}", qr, kr, v))
    if heads > 1:                               # head h: its own dominant key, its own ramp direction
        qs, ks = [], []
        for h in range(heads):
            c = _ramp(T, bool(h & 1))
            c[(5 * h + 1) % T] += 30.0
            qh, kh = _designed(c)
            qs.append(qh)
            ks.append(kh)
        out.append(("f_per_head", torch.stack(qs), torch.stack(ks), v))
    return out


def vt_with_tail(v, Tp, tail):
    """V^T (heads * 64, Tp) of v (heads, T, 64); columns >= T hold +-tail, alternating in both directions."""
    heads, T, _ = v.shape
    vt = torch.zeros(heads * HD, Tp)
    vt[:, :T] = v.permute(0, 2, 1).reshape(heads * HD, T)
    if Tp > T and tail:
        r, c = torch.arange(heads * HD)[:, None], torch.arange(Tp - T)[None, :]
        vt[:, T:] = tail * (1.0 - 2.0 * ((r + c) % 2).float())
    return vt


def attention_ref(qh, kh, vh, scale):
    """float64 softmax(q k^T scale) v per head: (heads, T, 64)"""
    s = (qh.double() @ kh.double().transpose(1, 2)) * scale
    return torch.softmax(s, dim=-1) @ vh.double()


def attention_emulation(qh, kh, vt, T, scale, dtype, mutant=None):
    """attention_kernel's algorithm in torch: keys in blocks of 64, float32 running maximum m and sum l, accumulator rescaled
    by alpha = exp(m_old - m_new), probabilities rounded to the storage type BEFORE the row sum and P.V, output o / l rounded
    to the storage type.  qh, kh (heads, T, 64) and vt (heads * 64, >= ceil64(T)) already quantised.  Key rows past T - 1 are
    read clamped to T - 1 and masked, as the kernel does.  Returns (heads, T, 64) float32.
    `mutant`: one of ATT_MUTANTS — a subtly wrong kernel."""
    assert mutant is None or mutant in ATT_MUTANTS
    heads = qh.shape[0]
    qh, kh, vt = qh.float(), kh.float(), vt.float()
    if mutant == "no_scale":
        scale = 1.0
    if mutant == "head_shift":
        kh = kh[:1].expand(heads, T, HD)
    scale = torch.tensor(scale, dtype=torch.float32)
    m = torch.full((heads, T), -math.inf)
    l = torch.zeros(heads, T)
    o = torch.zeros(heads, T, HD)
    last_valid = T - 2 if mutant == "drop_tail_key" else T - 1
    for k0 in range(0, T, KB):
        idx = torch.arange(k0, k0 + KB)
        s = (qh @ kh[:, idx.clamp(max=T - 1)].transpose(1, 2)) * scale              # (heads, T, 64)
        if mutant != "tail_v_used":
            s = torch.where(idx <= last_valid, s, torch.tensor(-math.inf))
        mx = torch.maximum(m, s.max(dim=-1).values)                                 # (drop_tail_key at T = 1: NaN, a miss)
        alpha = torch.ones_like(m) if mutant == "no_rescale" else torch.exp(m - mx)
        p = q(torch.exp(s - mx[..., None]), dtype)
        l = l * alpha + p.sum(dim=-1)
        vblk = vt[:, k0:k0 + KB].reshape(heads, HD, KB)                             # (heads, 64 dims, 64 keys)
        o = o * alpha[..., None] + p @ vblk.transpose(1, 2)
        m = mx
    return q(o / l[..., None], dtype)


# ---------------------------------------------------------------------------------------------------------------
# LayerNorm
# ---------------------------------------------------------------------------------------------------------------
LN_EPS = 1e-5


def layernorm_ref(x, gamma, beta, eps=LN_EPS, gelu=False):
    """float64 LayerNorm over the last axis (biased variance) + affine (+ erf GELU)"""
    x = x.double()
    mean = x.mean(-1, keepdim=True)
    var = (x - mean).pow(2).mean(-1, keepdim=True)
    y = (x - mean) / torch.sqrt(var + eps) * gamma.double() + beta.double()
    return TF.gelu(y) if gelu else y


def layernorm_emulation(x, gamma, beta, dtype, eps=LN_EPS, variance="two_pass"):
    """float32 LayerNorm of quantised rows, rounded to the storage type.  "two_pass" is layernorm_rows_kernel's arithmetic
    (mean, then the centred squares); "one_pass" is the mutant: E[x^2] - mean^2 in float32."""
    x = x.float()
    C = x.shape[-1]
    mean = x.sum(-1, keepdim=True) / C
    if variance == "two_pass":
        var = (x - mean).pow(2).sum(-1, keepdim=True) / C
    else:
        assert variance == "one_pass"
        var = (x * x).sum(-1, keepdim=True) / C - mean * mean
    rstd = torch.rsqrt(var + torch.tensor(eps, dtype=torch.float32))
    return q((x - mean) * rstd * gamma.float() + beta.float(), dtype)


def offset_mean_rows(T, C, kind, seed=0):
    """Rows around 100 whose values are representable in fp32, fp16 AND bf16 (bf16's step at 100 is 0.5).
    "std0.1": 2 % of a row at 99.5, 2 % at 100.5, the rest at 100: mean 100, std 0.1.
    "near_constant": one value per row at 100.5, the rest at 100 (std 0.5 / sqrt(C)): the variance sits below the float32
    rounding of mean^2 = 1e4, where E[x^2] - mean^2 loses every digit.  C must be a power of two: then the mean 100 + 0.5 / C
    is a float32 number.  (Otherwise rounding the mean alone, half an ulp of 100 = 3.8e-6 against deviations of 0.5 / C,
    costs ANY float32 LayerNorm a relative error near 1e-2: a badly conditioned row, not a wrong kernel.)
    Both kinds have an exactly representable mean, so a two-pass float32 kernel loses nothing on them."""
    g = torch.Generator().manual_seed(seed + C)
    x = torch.full((T, C), 100.0)
    for t in range(T):
        perm = torch.randperm(C, generator=g)
        if kind == "std0.1":
            n = max(1, round(0.02 * C))
            x[t, perm[:n]] = 99.5
            x[t, perm[n:2 * n]] = 100.5
        else:
            assert kind == "near_constant" and C & (C - 1) == 0
            x[t, perm[0]] = 100.5
    return x


# ---------------------------------------------------------------------------------------------------------------
# conv0, grouped conv
# ---------------------------------------------------------------------------------------------------------------
def conv0_ref(wave, w, bias, gamma, beta, stride, eps=LN_EPS):
    """float64 Conv1d(1 -> C, K, stride) -> LayerNorm(C) -> erf GELU; wave (n,), w (C, K): (T, C)"""
    y = TF.conv1d(wave.double()[None, None], w.double()[:, None], None if bias is None else bias.double(), stride=stride)[0].t()
    return layernorm_ref(y, gamma, beta, eps, gelu=True)


def grouped_same_pad_ref(h, w, G):
    """float64 Conv1d(H, H, K, padding = K // 2, groups = G) with the SamePad trim of an even K; h (T, H), w (H, H / G, K): (T, H)"""
    K = w.shape[-1]
    y = TF.conv1d(h.double().t()[None], w.double(), None, padding=K // 2, groups=G)[0]
    if K % 2 == 0:
        y = y[:, :-1]
    return y.t()
