"""Restatement, designed inputs and CPU emulation for the wav2vec 2.0 variants the embedder builds beside xlsr-53's:
the group-norm feature encoder (`feat_extract_norm="group"`) and the post-LN transformer (`do_stable_layer_norm=False`) of
wav2vec2-base / -large / -960h.  Shared by tests/test_w2v2_variants_cpu.py (which pins the restatement to `transformers`,
measures the tolerance constant and proves that the designed inputs tell a subtly wrong kernel from a right one) and
tests/test_w2v2_variants_gpu.py (which runs the kernels and the embedder).  Plain torch on the CPU.

1. `hidden_states`, `conv_features`, `w2v_last_four_layers_avg`: the published forward of the four combinations of the two
   switches, in the dtype of the state dict handed in (`to64` for the float64 reference), keyed by HF state-dict names.
2. `gn_cases`: designed inputs of the two layer-0 normalisation kernels (csrc/w2v2.hip: conv0_stats_kernel,
   conv0_stats_finish_kernel, conv0_groupnorm_kernel).  Integer operands make the conv exact in fp32 in any summation order
   (|x| < 2^24), so the float64 reference sees exactly the values the kernel normalises; the channel means reach 1.6e4 against
   a spread near 5, where a careless mean or variance shows.
3. `gn_emulation`: the kernels' summation scheme in fp32 (values taken relative to the channel's frame-0 value, Welford per
   wave over every fourth frame of a workgroup's slice, Chan's merge in wave order, then in workgroup order), with planted
   mutants.

GN_ATOL (fp32) was measured by test_w2v2_variants_cpu.py::test_emulation_error_is_what_gn_atol_was_taken_from, which measures it
again at every run: the worst |emulation - float64| over all designed cases is 5.3e-6 (at 262 144 frames: 1024 partials
merged one after the other, each merge rounding the sum of squares once; 1e-6 at 999 frames); the constant is 4 x that, rounded
up, the margin of tests/elementwise_cases.py and tests/sa_loss_cases.py.  It multiplies nothing: outputs are O(1) (|y| < 8).
At 16 bits the stored value is that rounded once more: half an ulp, 2^-8 |y| (bf16) or 2^-11 |y| + 2^-25 (fp16), on top.
"""
import math
from dataclasses import dataclass
from typing import Dict, List, Tuple

import numpy as np
import torch
import torch.nn.functional as F

GN_EPS = 1e-5
GN_ATOL = 2.2e-5
GN_MEASURED = 5.3e-6
ROUNDING = {torch.float32: (0.0, 0.0), torch.bfloat16: (2.0 ** -8, 0.0), torch.float16: (2.0 ** -11, 2.0 ** -25)}
SLICE_MIN, MAX_WG = 256, 1024           # SDA_W2V_GN_SLICE_MIN, SDA_W2V_GN_MAX_WG of include/sd_amd.h
SWEEP = 4096 * 4                        # frames one sweep of conv0_groupnorm_kernel's capped grid covers
SENTINEL = 77.0


# ---------------------------------------------------------------------------------------------------------------
# 1. the four variants restated
# ---------------------------------------------------------------------------------------------------------------
@dataclass
class VariantConfig:
    conv_dim: Tuple[int, ...] = (512,) * 7
    conv_kernel: Tuple[int, ...] = (10, 3, 3, 3, 3, 2, 2)
    conv_stride: Tuple[int, ...] = (5, 2, 2, 2, 2, 2, 2)
    conv_bias: bool = False
    hidden_size: int = 768
    num_attention_heads: int = 12
    intermediate_size: int = 3072
    num_hidden_layers: int = 12
    num_conv_pos_embeddings: int = 128
    num_conv_pos_embedding_groups: int = 16
    layer_norm_eps: float = 1e-5
    feat_extract_norm: str = "group"
    do_stable_layer_norm: bool = False

    def hf_kwargs(self) -> dict:
        return dict(conv_dim=list(self.conv_dim), conv_kernel=list(self.conv_kernel), conv_stride=list(self.conv_stride),
                    conv_bias=self.conv_bias, hidden_size=self.hidden_size, num_attention_heads=self.num_attention_heads,
                    intermediate_size=self.intermediate_size, num_hidden_layers=self.num_hidden_layers,
                    num_conv_pos_embeddings=self.num_conv_pos_embeddings,
                    num_conv_pos_embedding_groups=self.num_conv_pos_embedding_groups, layer_norm_eps=self.layer_norm_eps,
                    feat_extract_norm=self.feat_extract_norm, do_stable_layer_norm=self.do_stable_layer_norm,
                    num_feat_extract_layers=len(self.conv_dim), hidden_act="gelu", feat_extract_activation="gelu",
                    apply_spec_augment=False)

    def embedder_kwargs(self) -> dict:
        """Keyword arguments of speech_decoding_amd.wav2vec2.Wav2Vec2Config"""
        return {k: getattr(self, k) for k in self.__dataclass_fields__}


COMBOS = [("group", False), ("group", True), ("layer", False), ("layer", True)]       # (feat_extract_norm, do_stable_layer_norm)
SMALL = dict(conv_dim=(64,) * 7, hidden_size=128, num_attention_heads=2, intermediate_size=256, num_hidden_layers=5,
             num_conv_pos_embeddings=16, num_conv_pos_embedding_groups=4)             # tests/test_wav2vec2_gpu.py's
MID = dict(conv_dim=(512,) * 7, hidden_size=256, num_attention_heads=4, intermediate_size=512, num_hidden_layers=4,
           num_conv_pos_embeddings=128, num_conv_pos_embedding_groups=16)
BASE = dict()                                                                        # VariantConfig's defaults: wav2vec2-base


def to64(sd):
    return {k: v.double() for k, v in sd.items() if v.is_floating_point()}


def n_frames(n: int, cfg: VariantConfig) -> int:
    for k, s in zip(cfg.conv_kernel, cfg.conv_stride):
        n = (n - k) // s + 1
    return n


def chunk_bounds(n_samples: int, n_chunks: int = 10) -> List[Tuple[int, int]]:
    q, r = divmod(n_samples, n_chunks)
    edges = np.concatenate([[0], np.cumsum([q + 1] * r + [q] * (n_chunks - r))])
    return [(int(edges[i]), int(edges[i + 1])) for i in range(n_chunks)]


def pos_conv_weight(sd) -> torch.Tensor:
    p = "encoder.pos_conv_embed.conv."
    if p + "weight_g" in sd:
        g, v = sd[p + "weight_g"], sd[p + "weight_v"]
    else:
        g, v = sd[p + "parametrizations.weight.original0"], sd[p + "parametrizations.weight.original1"]
    return g * v / v.pow(2).sum(dim=(0, 1), keepdim=True).sqrt()


def feature_encoder(sd, cfg: VariantConfig, wave: torch.Tensor) -> torch.Tensor:
    """(B, L) -> (B, C, frames): HF Wav2Vec2FeatureEncoder.  "group": GroupNorm(C groups) after conv 0 only, its statistics
    over every frame of THIS call; "layer": LayerNorm over the channels after every conv."""
    h = wave[:, None].to(sd["feature_extractor.conv_layers.0.conv.weight"].dtype)
    for i, s in enumerate(cfg.conv_stride):
        p = f"feature_extractor.conv_layers.{i}."
        h = F.conv1d(h, sd[p + "conv.weight"], sd[p + "conv.bias"] if cfg.conv_bias else None, stride=s)
        if cfg.feat_extract_norm == "layer":
            h = F.layer_norm(h.transpose(1, 2), (h.shape[1],), sd[p + "layer_norm.weight"], sd[p + "layer_norm.bias"], 1e-5).transpose(1, 2)
        elif i == 0:
            mean = h.mean(dim=2, keepdim=True)
            var = (h - mean).pow(2).mean(dim=2, keepdim=True)
            h = (h - mean) / torch.sqrt(var + GN_EPS) * sd[p + "layer_norm.weight"][None, :, None] + sd[p + "layer_norm.bias"][None, :, None]
        h = F.gelu(h)
    return h


def conv_features(sd, cfg: VariantConfig, waveform: torch.Tensor) -> torch.Tensor:
    """`model.feature_extractor(waveform)` for a (1, L) waveform: (1, C, frames), the whole file in one call."""
    with torch.no_grad():
        return feature_encoder(sd, cfg, waveform)


def _attention(sd, cfg, p, x):
    B, T, H = x.shape
    nh, hd = cfg.num_attention_heads, cfg.hidden_size // cfg.num_attention_heads
    q = F.linear(x, sd[p + "q_proj.weight"], sd[p + "q_proj.bias"]).view(B, T, nh, hd).transpose(1, 2)
    k = F.linear(x, sd[p + "k_proj.weight"], sd[p + "k_proj.bias"]).view(B, T, nh, hd).transpose(1, 2)
    v = F.linear(x, sd[p + "v_proj.weight"], sd[p + "v_proj.bias"]).view(B, T, nh, hd).transpose(1, 2)
    w = torch.softmax(torch.matmul(q, k.transpose(2, 3)) * hd ** -0.5, dim=-1)
    o = torch.matmul(w, v).transpose(1, 2).reshape(B, T, H)
    return F.linear(o, sd[p + "out_proj.weight"], sd[p + "out_proj.bias"])


def hidden_states(sd, cfg: VariantConfig, wave: torch.Tensor) -> List[torch.Tensor]:
    """`output_hidden_states` of Wav2Vec2Model(eval) for a (B, L) waveform: num_hidden_layers + 1 tensors (B, frames, H)."""
    eps = cfg.layer_norm_eps
    H = cfg.hidden_size

    def ln(x, name):
        return F.layer_norm(x, (x.shape[-1],), sd[name + ".weight"], sd[name + ".bias"], eps)

    def ffn(x, p):
        u = F.gelu(F.linear(x, sd[p + "feed_forward.intermediate_dense.weight"], sd[p + "feed_forward.intermediate_dense.bias"]))
        return F.linear(u, sd[p + "feed_forward.output_dense.weight"], sd[p + "feed_forward.output_dense.bias"])
    with torch.no_grad():
        feats = feature_encoder(sd, cfg, wave).transpose(1, 2)
        h = F.linear(ln(feats, "feature_projection.layer_norm"), sd["feature_projection.projection.weight"],
                     sd["feature_projection.projection.bias"])
        K = cfg.num_conv_pos_embeddings
        pos = F.conv1d(h.transpose(1, 2), pos_conv_weight(sd), sd["encoder.pos_conv_embed.conv.bias"], padding=K // 2,
                       groups=cfg.num_conv_pos_embedding_groups)
        if K % 2 == 0:
            pos = pos[:, :, :-1]
        h = h + F.gelu(pos).transpose(1, 2)
        out = []
        if cfg.do_stable_layer_norm:
            for i in range(cfg.num_hidden_layers):
                out.append(h)
                p = f"encoder.layers.{i}."
                h = h + _attention(sd, cfg, p + "attention.", ln(h, p + "layer_norm"))
                h = h + ffn(ln(h, p + "final_layer_norm"), p)
            out.append(ln(h, "encoder.layer_norm"))
        else:
            h = ln(h, "encoder.layer_norm")
            for i in range(cfg.num_hidden_layers):
                out.append(h)
                p = f"encoder.layers.{i}."
                h = ln(h + _attention(sd, cfg, p + "attention.", h), p + "layer_norm")
                h = ln(h + ffn(h, p), p + "final_layer_norm")
            out.append(h)
    assert out[0].shape[-1] == H
    return out


def w2v_last_four_layers_avg(sd, cfg: VariantConfig, waveform: torch.Tensor, n_chunks: int = 10) -> torch.Tensor:
    """`getW2VLastFourLayersAvg`: (1, L) -> (H, frames); every chunk is a forward call of its own (its own statistics)."""
    embs = []
    for a, b in chunk_bounds(waveform.shape[-1], n_chunks):
        embs.append(torch.stack(hidden_states(sd, cfg, waveform[:, a:b])[-4:]).mean(dim=0)[0])
    return torch.vstack(embs).t()


def random_state_dict(cfg: VariantConfig, seed: int = 0, scale: float = 1.0, parametrized: bool = False) -> Dict[str, torch.Tensor]:
    """Seeded fp32 weights under the HF key names of the variant: `layer_norm.*` of conv layer 0 only for "group", conv
    biases only with conv_bias; the positional conv's weight norm under the old or the parametrize-era names."""
    g = torch.Generator().manual_seed(seed)
    sd = {}

    def lin(name, out_f, in_f):
        sd[name + ".weight"] = torch.randn(out_f, in_f, generator=g) * (scale / np.sqrt(in_f))
        sd[name + ".bias"] = torch.randn(out_f, generator=g) * 0.1

    def ln(name, c):
        sd[name + ".weight"] = 1.0 + 0.1 * torch.randn(c, generator=g)
        sd[name + ".bias"] = 0.1 * torch.randn(c, generator=g)
    cin = 1
    for i, (c, k) in enumerate(zip(cfg.conv_dim, cfg.conv_kernel)):
        p = f"feature_extractor.conv_layers.{i}."
        sd[p + "conv.weight"] = torch.randn(c, cin, k, generator=g) * (scale / np.sqrt(cin * k))
        if cfg.conv_bias:
            sd[p + "conv.bias"] = torch.randn(c, generator=g) * 0.1
        if cfg.feat_extract_norm == "layer" or i == 0:
            ln(p + "layer_norm", c)
        cin = c
    ln("feature_projection.layer_norm", cfg.conv_dim[-1])
    lin("feature_projection.projection", cfg.hidden_size, cfg.conv_dim[-1])
    H, K, G = cfg.hidden_size, cfg.num_conv_pos_embeddings, cfg.num_conv_pos_embedding_groups
    names = ("parametrizations.weight.original0", "parametrizations.weight.original1") if parametrized else ("weight_g", "weight_v")
    sd["encoder.pos_conv_embed.conv." + names[0]] = 0.5 + torch.rand(1, 1, K, generator=g)
    sd["encoder.pos_conv_embed.conv." + names[1]] = torch.randn(H, H // G, K, generator=g) * 0.05
    sd["encoder.pos_conv_embed.conv.bias"] = torch.randn(H, generator=g) * 0.1
    ln("encoder.layer_norm", H)
    for i in range(cfg.num_hidden_layers):
        p = f"encoder.layers.{i}."
        for n in ("q_proj", "k_proj", "v_proj", "out_proj"):
            lin(p + "attention." + n, H, H)
        ln(p + "layer_norm", H)
        lin(p + "feed_forward.intermediate_dense", cfg.intermediate_size, H)
        lin(p + "feed_forward.output_dense", H, cfg.intermediate_size)
        ln(p + "final_layer_norm", H)
    return sd


def rel_l2(a, b):
    return float((a.double() - b.double()).norm() / b.double().norm())


# ---------------------------------------------------------------------------------------------------------------
# 2. designed inputs of the layer-0 normalisation kernels
# ---------------------------------------------------------------------------------------------------------------
K0, STRIDE0 = 10, 5


def samples_for(T0: int) -> int:
    return (T0 - 1) * STRIDE0 + K0


def gn_slice(T0: int) -> int:
    return max(SLICE_MIN, -(-T0 // MAX_WG))


def gn_case_list():
    """[(name, n_samples, C, with_bias, kind)]: kind "int" = the designed integers, "randn" = real-valued operands, "quiet" =
    a waveform of amplitude 1e-3 (digital near-silence: the variance falls below eps, so where eps sits matters)."""
    cases = []
    for n in (14, 19, 5004):                                        # T0 = 1 (variance 0: y = GELU(beta)), 2, 999
        for j, C in enumerate((32, 64, 96, 512, 600)):              # 96 and 600: a ragged last 64-lane group
            cases.append((f"int_n{n}_C{C}", n, C, bool(j & 1), "int"))
    for T0 in (SLICE_MIN - 1, SLICE_MIN, SLICE_MIN + 1):            # one workgroup's slice: one below, at, one above
        cases.append((f"int_slice_T{T0}", samples_for(T0), 64, T0 & 1 == 0, "int"))
    for T0 in (SWEEP - 1, SWEEP, SWEEP + 1):                        # the normalising pass's capped grid: a second sweep
        cases.append((f"int_sweep_T{T0}", samples_for(T0), 32, T0 & 1 == 1, "int"))
    cases.append((f"int_sweep_T{SWEEP + 1}_C512", samples_for(SWEEP + 1), 512, False, "int"))
    cases.append(("int_n1000003_C32", 1000003, 32, True, "int"))    # T0 = 199 999: 782 slices, the last one short
    cases.append(("int_n1000003_C64", 1000003, 64, False, "int"))
    for T0 in (SLICE_MIN * MAX_WG, SLICE_MIN * MAX_WG + 1):         # the slice grows from 256 to 257 frames: 1024 -> 1021 workgroups
        cases.append((f"int_grow_T{T0}", samples_for(T0), 32, T0 & 1 == 1, "int"))
    cases.append(("randn_n5004_C96", 5004, 96, True, "randn"))
    cases.append(("randn_n25003_C512", 25003, 512, False, "randn"))
    cases.append(("quiet_n5004_C64", 5004, 64, False, "quiet"))
    return cases


# One case whose output buffer passes 2^31 ELEMENTS ((16 + 2^21 + 5) rows of 1024 channels; 4.3 GB at 16 bits), where a 32-bit
# row offset would wrap.  Channels are independent, so the reference, the emulation and the comparison take 17 of the 1024.
LARGE = ("int_past_2p31_C1024", (2 ** 21 + 4) * 5 + 10, 1024, True, "int")
LARGE_SEL = list(range(0, 1024, 64)) + [1023]


def gn_subset(inp, sel):
    """the same inputs restricted to the channels `sel`"""
    wave, w, bias, gamma, beta = inp
    return wave, w[sel], None if bias is None else bias[sel], gamma[sel], beta[sel]


def gn_inputs(name, n, C, with_bias, kind):
    """wave (n,), w (C, K0), bias (C,) or None, gamma (C,), beta (C,): fp32"""
    g = torch.Generator().manual_seed(sum(map(ord, name)) * 7919 + n)
    if kind == "int":
        wave = 1000.0 + torch.randint(-2, 3, (n,), generator=g).float()
        w = torch.randint(-1, 3, (C, K0), generator=g).float()
        bias = torch.randint(-3, 4, (C,), generator=g).float() if with_bias else None
    else:
        wave = torch.randn(n, generator=g) * (1e-3 if kind == "quiet" else 1.0)
        w = torch.randn(C, K0, generator=g) / math.sqrt(K0)
        bias = torch.randn(C, generator=g) * 0.1 if with_bias else None
    gamma = 1.0 + 0.1 * torch.randn(C, generator=g)
    beta = 0.1 * torch.randn(C, generator=g)
    return wave, w, bias, gamma, beta


def conv0_ref(wave, w, bias):
    """float64 (T0, C) conv output"""
    return F.conv1d(wave.double()[None, None], w.double()[:, None], None if bias is None else bias.double(), stride=STRIDE0)[0].t()


def gn_ref(wave, w, bias, gamma, beta, eps=GN_EPS):
    """float64 (T0, C): GELU(gamma (x - mean_c) / sqrt(var_c + eps) + beta), statistics over all T0 frames, biased variance"""
    x = conv0_ref(wave, w, bias)
    mean = x.mean(0, keepdim=True)
    var = (x - mean).pow(2).mean(0, keepdim=True)
    return F.gelu((x - mean) / torch.sqrt(var + eps) * gamma.double() + beta.double())


def gn_bound(ref, dtype):
    """elementwise bound of |stored - float64|: GN_ATOL, plus one rounding to the storage type"""
    rel, sub = ROUNDING[dtype]
    return GN_ATOL + rel * ref.abs() + sub


def gn_ratio(got, ref, dtype=torch.float32):
    """max |got - ref| / bound: <= 1 passes; NaN / Inf count as infinitely far"""
    got, ref = got.double(), ref.double()
    if not bool(torch.isfinite(got).all()):
        return float("inf")
    return float(((got - ref).abs() / gn_bound(ref, dtype)).max())


# ---------------------------------------------------------------------------------------------------------------
# 3. the kernels' summation scheme in fp32, and its mutants
# ---------------------------------------------------------------------------------------------------------------
GN_MUTANTS = ["one_pass", "unbiased", "drop_last_slice", "slice_twice", "full_slice_count", "t0_off_by_one", "eps_outside",
              "no_between_term", "gelu_first"]


def _fma(a, b, c):
    """fp32 fused multiply-add: the product of two fp32 numbers is exact in float64"""
    return (a.double() * b.double() + c.double()).float()


def conv0_fp32(wave, w, bias):
    """conv0_frame's arithmetic: v = bias, then one fma per tap in tap order; (T0, C) fp32"""
    T0 = (wave.numel() - K0) // STRIDE0 + 1
    xs = wave.float().unfold(0, K0, STRIDE0)[:T0]                 # (T0, K0)
    v = (torch.zeros(w.shape[0]) if bias is None else bias.float())[None, :].expand(T0, -1)
    for j in range(K0):
        v = _fma(w[:, j].float()[None, :], xs[:, j][:, None], v)
    return v


def _chan(na, ma, qa, nb, mb, qb, between=True):
    """chan_merge of csrc/w2v2.hip on fp32 tensors; nb == 0 leaves (na, ma, qa) as they are"""
    n = na + nb
    d = mb - ma
    r = nb / torch.where(n > 0, n, torch.ones_like(n))
    m = _fma(d, r, ma)
    q = (qa + qb) + ((d * d) * (na * r) if between else 0.0)
    keep = nb == 0
    return torch.where(keep, na, n), torch.where(keep, ma, m), torch.where(keep, qa, q)


def gn_stats_emulation(x, mutant=None):
    """(mean (C,), M2 (C,), count) of fp32 values x (T0, C) as conv0_stats_kernel + conv0_stats_finish_kernel form them (the
    kernels hand it the conv outputs less the shift)."""
    T0, C = x.shape
    if mutant == "t0_off_by_one":
        x, T0 = x[:T0 - 1], T0 - 1
        if T0 < 1:
            nan = torch.full((C,), float("nan"))
            return nan, nan, 0
    f32 = torch.float32
    if mutant == "one_pass":
        mean = x.sum(0) / T0
        return mean, ((x * x).sum(0) / T0 - mean * mean) * T0, T0
    slice_ = gn_slice(T0)
    n_wg = -(-T0 // slice_)
    steps = -(-(slice_ + 1) // 4)
    g = torch.arange(n_wg)[None, :, None]
    wv = torch.arange(4)[None, None, :]
    i = torch.arange(steps)[:, None, None]
    start = g * slice_ - (1 if mutant == "slice_twice" else 0) * (g > 0)      # the boundary frame counted by both neighbours
    stop = torch.clamp((g + 1) * slice_, max=T0)
    t = start + wv + 4 * i                                                     # (steps, n_wg, 4)
    valid = t < stop
    xg = x[t.clamp(max=T0 - 1)]                                                # (steps, n_wg, 4, C)
    mean = torch.zeros(n_wg, 4, C)
    m2 = torch.zeros(n_wg, 4, C)
    n = torch.zeros(n_wg, 4, 1)
    for s in range(steps):
        ok = valid[s][..., None]
        n = n + ok.to(f32)
        rn = 1.0 / torch.where(n > 0, n, torch.ones_like(n))
        d = xg[s] - mean
        mnew = _fma(d, rn, mean)
        qnew = _fma(d, xg[s] - mnew, m2)
        mean, m2 = torch.where(ok, mnew, mean), torch.where(ok, qnew, m2)
    between = mutant != "no_between_term"
    na, ma, qa = torch.zeros(n_wg, 1), torch.zeros(n_wg, C), torch.zeros(n_wg, C)
    for k in range(4):
        na, ma, qa = _chan(na, ma, qa, n[:, k], mean[:, k], m2[:, k], between)
    if mutant == "full_slice_count":
        na = torch.full_like(na, float(slice_))
    last = n_wg - 1 if mutant == "drop_last_slice" else n_wg
    nt, mt, qt = torch.zeros(1), torch.zeros(C), torch.zeros(C)
    for k in range(last):
        nt, mt, qt = _chan(nt, mt, qt, na[k], ma[k], qa[k], between)
    if last == 0:
        mt, qt = torch.full((C,), float("nan")), torch.full((C,), float("nan"))
    return mt, qt, T0


def gn_emulation(wave, w, bias, gamma, beta, dtype=torch.float32, eps=GN_EPS, mutant=None):
    """The three kernels in fp32 on the CPU, the result rounded to the storage type: (T0, C) float32."""
    assert mutant is None or mutant in GN_MUTANTS
    x = conv0_fp32(wave, w, bias)
    if mutant != "one_pass":                       # z = x - shift, shift = the conv output at frame 0 (one_pass: the raw sums)
        x = x - x[:1]
    mean, m2, count = gn_stats_emulation(x, mutant)
    T0 = x.shape[0]
    eps = torch.tensor(eps, dtype=torch.float32)
    if mutant == "unbiased":
        var = m2 / torch.tensor(float(T0 - 1)) if T0 > 1 else torch.full_like(m2, float("nan"))
    else:
        var = m2 / torch.tensor(float(max(count, 1)))
    rstd = 1.0 / (torch.sqrt(var) + eps) if mutant == "eps_outside" else torch.rsqrt(var + eps)
    xh = (x - mean[None]) * rstd[None]
    if mutant == "gelu_first":
        y = _fma(F.gelu(xh), gamma.float()[None], beta.float()[None])
    else:
        y = F.gelu(_fma(xh, gamma.float()[None], beta.float()[None]))
    return y.to(dtype).float()
