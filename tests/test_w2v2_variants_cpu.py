"""CPU half of the tests of the wav2vec 2.0 variants beside xlsr-53's (group-norm feature encoder, post-LN transformer).

1. `Wav2Vec2Config.from_hf(cfg, any_variant=True)` accepts the four combinations of the two switches and still refuses what
   was refused; without the argument it keeps its earlier contract.
2. The restatement of tests/w2v2_variant_cases.py is pinned to the installed `transformers` on seeded weights (all four
   combinations, hidden states and `feature_extractor`), and reproduces the committed fixtures.
3. The tolerance of the layer-0 normalisation kernels is measured: the fp32 emulation of their summation scheme against
   float64 over every designed case; GN_ATOL is 4 .. 5 x that.  Every planted mutant misses GN_ATOL by 10 x or more on at
   least one designed case, so the GPU test's inputs tell a subtly wrong kernel from a right one.
4. Host-side refusals of the two new entry points, before anything is launched (the pointers passed are host memory)."""
import ctypes
import os
import types

import numpy as np
import pytest
import torch

from tests import w2v2_variant_cases as V

MARGIN = 10.0
GOLDEN = os.path.join(os.path.dirname(__file__), "golden")


def _hf_stub(**kw):
    base = dict(conv_dim=[512] * 7, conv_kernel=[10, 3, 3, 3, 3, 2, 2], conv_stride=[5, 2, 2, 2, 2, 2, 2], conv_bias=False,
                hidden_size=768, num_attention_heads=12, intermediate_size=3072, num_hidden_layers=12, num_conv_pos_embeddings=128,
                num_conv_pos_embedding_groups=16, layer_norm_eps=1e-5, feat_extract_norm="group", do_stable_layer_norm=False,
                hidden_act="gelu", feat_extract_activation="gelu")
    return types.SimpleNamespace(**dict(base, **kw))


@pytest.mark.parametrize("norm,stable", V.COMBOS)
def test_from_hf_accepts_the_four_combinations(norm, stable):
    from speech_decoding_amd.wav2vec2 import Wav2Vec2Config
    cfg = Wav2Vec2Config.from_hf(_hf_stub(feat_extract_norm=norm, do_stable_layer_norm=stable), any_variant=True)
    assert (cfg.feat_extract_norm, cfg.do_stable_layer_norm, cfg.conv_bias) == (norm, stable, False)
    assert (cfg.hidden_size, cfg.num_hidden_layers, cfg.conv_dim) == (768, 12, (512,) * 7)


def test_defaults_are_xlsr53s_and_what_was_refused_still_is():
    from speech_decoding_amd.wav2vec2 import Wav2Vec2Config, Wav2Vec2Embedder
    d = Wav2Vec2Config()
    assert (d.feat_extract_norm, d.do_stable_layer_norm, d.conv_bias) == ("layer", True, True)
    for kw in (dict(hidden_act="relu"), dict(feat_extract_activation="swish"), dict(feat_extract_norm="batch")):
        with pytest.raises(ValueError):
            Wav2Vec2Config.from_hf(_hf_stub(**kw), any_variant=True)
    # without any_variant the method keeps its earlier contract: xlsr-53's combination only
    assert Wav2Vec2Config.from_hf(_hf_stub(feat_extract_norm="layer", do_stable_layer_norm=True)).feat_extract_norm == "layer"
    for norm, stable in V.COMBOS[:3]:
        with pytest.raises(ValueError):
            Wav2Vec2Config.from_hf(_hf_stub(feat_extract_norm=norm, do_stable_layer_norm=stable))
    # refused by the constructor before any weight is packed or any kernel launched (no device is touched: CPU-only machine)
    for bad in (dict(hidden_size=96, num_attention_heads=2),                         # head dimension 48
                dict(conv_dim=(64, 64, 64, 64, 64, 64, 32)), dict(num_hidden_layers=3)):
        kw = dict(V.SMALL, feat_extract_norm="group", do_stable_layer_norm=False, conv_bias=False)
        kw.update(bad)
        with pytest.raises(ValueError):
            Wav2Vec2Embedder({}, Wav2Vec2Config(**kw), dtype=torch.float32)


@pytest.mark.parametrize("norm,stable", V.COMBOS)
def test_restatement_matches_transformers(norm, stable):
    tr = pytest.importorskip("transformers")
    cfg = V.VariantConfig(**dict(V.SMALL, feat_extract_norm=norm, do_stable_layer_norm=stable, conv_bias=(norm == "layer")))
    torch.manual_seed(11)
    model = tr.Wav2Vec2Model(tr.Wav2Vec2Config(**cfg.hf_kwargs())).eval()
    with torch.no_grad():
        for k, p in model.named_parameters():
            if k.endswith("bias"):
                p.normal_(0.0, 0.1)
            elif "layer_norm.weight" in k:
                p.normal_(1.0, 0.1)
    sd = {k: v for k, v in model.state_dict().items() if v.is_floating_point()}
    wave = torch.randn(1, 6000, generator=torch.Generator().manual_seed(12)) + 0.3
    with torch.no_grad():
        ref = model(input_values=wave, output_hidden_states=True).hidden_states
        feat = model.feature_extractor(wave)
    got = V.hidden_states(V.to64(sd), cfg, wave)
    assert len(got) == len(ref) == cfg.num_hidden_layers + 1
    for i, (g, r) in enumerate(zip(got, ref)):
        assert float((g - r.double()).abs().max()) < 1e-4, (i, float((g - r.double()).abs().max()))
    gf = V.conv_features(V.to64(sd), cfg, wave)
    assert gf.shape == feat.shape and float((gf - feat.double()).abs().max()) < 1e-4


def _fixture(name):
    z = np.load(os.path.join(GOLDEN, name))
    kw = {k: (tuple(int(v) for v in z["cfg_" + k]) if z["cfg_" + k].ndim else int(z["cfg_" + k]))
          for k in ("conv_dim", "conv_kernel", "conv_stride", "hidden_size", "num_attention_heads", "intermediate_size",
                    "num_hidden_layers", "num_conv_pos_embeddings", "num_conv_pos_embedding_groups")}
    kw.update(feat_extract_norm=str(z["cfg_feat_extract_norm"]), do_stable_layer_norm=bool(z["cfg_do_stable_layer_norm"]),
              conv_bias=bool(z["cfg_conv_bias"]))
    sd = {k[3:]: torch.from_numpy(z[k]) for k in z.files if k.startswith("sd/")}
    return kw, sd, z


FIXTURES = [("w2v2_group_postln.npz", False), ("w2v2_group_stable.npz", True)]


@pytest.mark.parametrize("name,stable", FIXTURES)
def test_fixtures_load_and_the_restatement_reproduces_them(name, stable):
    path = os.path.join(GOLDEN, name)
    assert os.path.getsize(path) <= os.path.getsize(os.path.join(GOLDEN, "w2v2_small.npz"))
    kw, sd, z = _fixture(name)
    assert kw["feat_extract_norm"] == "group" and kw["do_stable_layer_norm"] is stable and kw["conv_bias"] is False
    assert "feature_extractor.conv_layers.0.layer_norm.weight" in sd and "feature_extractor.conv_layers.1.layer_norm.weight" not in sd
    cfg = V.VariantConfig(**kw)
    wave = torch.from_numpy(z["waveform"])
    sd64 = V.to64(sd)
    got = V.w2v_last_four_layers_avg(sd64, cfg, wave)
    assert got.shape == z["expected"].shape
    assert float((got - torch.from_numpy(z["expected"]).double()).abs().max()) < 1e-4
    for i, h in enumerate(V.hidden_states(sd64, cfg, wave[:, :4000])):
        assert float((h[0] - torch.from_numpy(z[f"hs/{i}"]).double()).abs().max()) < 1e-4, i
    feat = V.conv_features(sd64, cfg, wave)
    assert feat.shape == z["feat"].shape == (1, 32, V.n_frames(wave.shape[1], cfg))
    assert float((feat - torch.from_numpy(z["feat"]).double()).abs().max()) < 1e-4


# ---------------------------------------------------------------------------------------------------------------
# the normalisation kernels' tolerance and the sensitivity of their designed inputs
# ---------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def designed():
    """{name: (inputs, float64 reference)}: computed once for the module"""
    out = {}
    for case in V.gn_case_list():
        inp = V.gn_inputs(*case)
        out[case[0]] = (inp, V.gn_ref(*inp))
    inp = V.gn_subset(V.gn_inputs(*V.LARGE), V.LARGE_SEL)             # 2 097 157 frames, 17 of its 1024 channels
    out[V.LARGE[0]] = (inp, V.gn_ref(*inp))
    return out


def test_designed_integer_cases_are_exact_and_badly_conditioned(designed):
    top_mean = 0.0
    for case in V.gn_case_list():
        if case[4] != "int":
            continue
        (wave, w, bias, _, _), _ = designed[case[0]]
        x64, x32 = V.conv0_ref(wave, w, bias), V.conv0_fp32(wave, w, bias)
        assert torch.equal(x32.double(), x64) and torch.equal(x64, x64.round()), case[0]      # exact integers in fp32
        top_mean = max(top_mean, float(x64.mean(0).abs().max()))
        if x64.shape[0] >= 999:
            var = x64.var(0, unbiased=False)
            assert 4 < float(var.min()) and float(var.max()) < 80, (case[0], float(var.min()), float(var.max()))
    assert top_mean > 1.5e4
    names = [c[0] for c in V.gn_case_list()]
    assert len(set(names)) == len(names)
    frames = {(c[1] - V.K0) // V.STRIDE0 + 1 for c in V.gn_case_list()}
    assert {1, 2, 999, 199999, 255, 256, 257, V.SWEEP - 1, V.SWEEP, V.SWEEP + 1, 262144, 262145} <= frames
    assert V.gn_slice(262144) == 256 and V.gn_slice(262145) == 257


def test_emulation_error_is_what_gn_atol_was_taken_from(designed):
    worst, where = 0.0, None
    for name, (inp, ref) in designed.items():
        e = float((V.gn_emulation(*inp).double() - ref).abs().max())
        print(f"{name}: {e:.3e}")
        if e > worst:
            worst, where = e, name
    print("worst", worst, where)
    # 5 % of room: torch's CPU erf and float64 sums differ in the last place between instruction sets
    assert worst <= V.GN_MEASURED * 1.05, (worst, where)
    assert 0.95 * 4.0 * worst <= V.GN_ATOL <= 5.0 * worst, (worst, V.GN_ATOL)
    assert float(max(ref.abs().max() for _, ref in designed.values())) < 8.0


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16])
def test_emulation_rounded_to_16_bits_meets_the_bound(designed, dtype):
    for name, (inp, ref) in designed.items():
        assert V.gn_ratio(V.gn_emulation(*inp, dtype=dtype), ref, dtype) <= 1.0, name


@pytest.mark.parametrize("mutant", V.GN_MUTANTS)
def test_every_mutant_misses_gn_atol_by_10x(designed, mutant):
    worst, where = 0.0, None
    for name, (inp, ref) in designed.items():
        r = V.gn_ratio(V.gn_emulation(*inp, mutant=mutant), ref)
        if r > worst:
            worst, where = r, name
        if worst >= 1e3 * MARGIN:
            break
    print(mutant, worst, where)
    assert worst >= MARGIN, (mutant, worst, where)


def test_short_cases_are_what_catches_the_unbiased_variance(designed):
    """0.4 at two frames, 2e-3 at 999 and below GN_ATOL x 10 at 199 999: the short cases must stay."""
    by_frames = {}
    for case in V.gn_case_list():
        if case[4] == "int":
            inp, ref = designed[case[0]]
            T0 = (case[1] - V.K0) // V.STRIDE0 + 1
            e = float((V.gn_emulation(*inp, mutant="unbiased").double() - ref).abs().max()) if T0 > 1 else float("inf")
            by_frames[T0] = max(by_frames.get(T0, 0.0), e)
    assert by_frames[2] > 0.1 and 1e-4 < by_frames[999] < 1e-2 and by_frames[199999] < MARGIN * V.GN_ATOL


# ---------------------------------------------------------------------------------------------------------------
# host-side refusals
# ---------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def host():
    from speech_decoding_amd import lib
    L = lib.load()
    buf = (ctypes.c_char * (1 << 16))()                               # host memory that no kernel may ever see
    p = (ctypes.cast(buf, ctypes.c_void_p).value + 15) // 16 * 16
    return lib, L, p, buf


def _refused(L, rc, msg, what):
    assert rc == -1, what
    assert msg in L.sda_last_error(), (what, L.sda_last_error())


def test_stats_and_groupnorm_refuse_bad_arguments_without_launch(host):
    lib, L, p, _ = host

    def stats(T=5, C=64, K=10, stride=5, n=None, floats=None):
        n = (T - 1) * stride + K if n is None else n
        floats = L.sda_w2v_conv0_stats_floats(T, C) if floats is None else floats
        return L.sda_w2v_conv0_stats(p, n, p, None, p, floats, T, C, K, stride, 1e-5, None)

    def norm(T=5, C=64, Cp=64, K=10, stride=5, n=None, dtype=lib.F32):
        n = (T - 1) * stride + K if n is None else n
        return L.sda_w2v_conv0_groupnorm(p, n, p, None, p, p, p, p, T, C, Cp, K, stride, dtype, None)
    common = (dict(T=0), dict(T=-3), dict(C=0), dict(C=1025), dict(K=0), dict(stride=0), dict(n=(5 - 1) * 5 + 10 - 1),
              dict(C=1024, K=17), dict(C=512, K=33))
    for kw in common + (dict(floats=5 * 64 - 1), dict(floats=0)):
        _refused(L, stats(**kw), b"w2v_conv0_stats: bad arguments", kw)
    for kw in common:
        kw = dict(kw, Cp=max(64, (kw.get("C", 64) + 63) // 64 * 64)) if "C" in kw else kw
        _refused(L, norm(**kw), b"w2v_conv0_groupnorm: bad arguments", kw)
    for kw in (dict(C=65, Cp=64), dict(C=64, Cp=96), dict(C=64, Cp=1088)):
        _refused(L, norm(**kw), b"w2v_conv0_groupnorm: bad arguments", kw)
    for C in (64, 512, 1024):                                         # every NI branch refuses an unknown dtype
        _refused(L, norm(C=C, Cp=C, dtype=7), b"unknown dtype", C)
    assert L.sda_w2v_conv0_stats_floats(0, 64) == -1 and L.sda_w2v_conv0_stats_floats(5, 0) == -1
    # shift, mean, rstd, then (mean, M2) per workgroup: 256-frame slices up to 1024 workgroups, longer slices beyond
    for T, n_wg in ((1, 1), (256, 1), (257, 2), (262144, 1024), (262145, 1021), (1200000, 1024)):
        assert L.sda_w2v_conv0_stats_floats(T, 512) == (3 + 2 * n_wg) * 512, T


def test_ops_wrappers_refuse_host_tensors_and_frame_counts_past_a_c_int(host):
    from speech_decoding_amd import ops
    lib = host[0]
    wave, w, vec = torch.zeros(35), torch.zeros(64, 10), torch.zeros(64)
    with pytest.raises(lib.SdaError, match="on the device"):
        ops.w2v_conv0_stats(wave, w, None, torch.zeros(5 * 64), 5, 64, 10, 5)
    with pytest.raises(lib.SdaError, match="on the device"):
        ops.w2v_conv0_groupnorm(wave, w, None, vec, vec, torch.zeros(3, 64), torch.zeros(64, 64), 5, 64, 10, 5)
    for T in (0, 2 ** 31 - 16, 2 ** 31, 2 ** 32 + 5):                 # a C int would wrap the last ones
        with pytest.raises(lib.SdaError, match=r"1 <= frames <= 2147483631"):
            ops.w2v_conv0_stats(wave, w, None, torch.zeros(5 * 64), T, 64, 10, 5)
        with pytest.raises(lib.SdaError, match=r"1 <= frames <= 2147483631"):
            ops.w2v_conv0_groupnorm(wave, w, None, vec, vec, torch.zeros(3, 64), torch.zeros(64, 64), T, 64, 10, 5)
        with pytest.raises(lib.SdaError, match=r"1 <= frames <= 2147483631"):
            ops.w2v_conv0_stats_floats(T, 64)
