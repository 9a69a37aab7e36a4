"""The wav2vec 2.0 variants beside xlsr-53's on MI355X: the layer-0 group-norm kernels on their own on the designed cases of
tests/w2v2_variant_cases.py (whose sensitivity and tolerance tests/test_w2v2_variants_cpu.py establishes), and the embedder
end to end against that file's float64 restatement on seeded weights (itself pinned to `transformers` on the CPU).  Needs
neither the reference nor `transformers` (one test takes an HF model object when `transformers` is there)."""
import os

import numpy as np
import pytest
import torch

from tests import w2v2_variant_cases as V
from tests.test_wav2vec2_gpu import REL

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
DTYPES = [torch.float32, torch.bfloat16, torch.float16]
GOLDEN = os.path.join(os.path.dirname(__file__), "golden")
_CACHE = {}


def cached(key, make):
    if key not in _CACHE:
        _CACHE[key] = make()
    return _CACHE[key]


# ---------------------------------------------------------------------------------------------------------------
# the kernels on their own
# ---------------------------------------------------------------------------------------------------------------
def run_groupnorm(inp, dtype, Cp=None):
    """-> (row-layout buffer pre-filled with the sentinel, T0, the (3, C) statistics)"""
    from speech_decoding_amd import lib, ops
    wave, w, bias, gamma, beta = [None if t is None else t.to(DEV) for t in inp]
    C = w.shape[0]
    T0 = (wave.numel() - V.K0) // V.STRIDE0 + 1
    y = torch.full((lib.rows_alloc(1, T0), Cp or lib.pad_channels(C)), V.SENTINEL, dtype=dtype, device=DEV)
    scratch = torch.full((ops.w2v_conv0_stats_floats(T0, C),), V.SENTINEL, dtype=torch.float32, device=DEV)
    stats = ops.w2v_conv0_stats(wave, w, bias, scratch, T0, C, V.K0, V.STRIDE0, V.GN_EPS)
    ops.w2v_conv0_groupnorm(wave, w, bias, gamma, beta, stats, y, T0, C, V.K0, V.STRIDE0)
    return y, T0, stats


def check_groupnorm(y, T0, C, ref, dtype, name):
    from speech_decoding_amd import lib
    PAD = lib.ROW_PAD
    got = y[PAD:PAD + T0].float().cpu()
    ratio = V.gn_ratio(got[:, :C], ref, dtype)
    print(f"{name} {dtype}: max error / bound = {ratio:.3f}")
    assert ratio <= 1.0, (name, ratio)
    assert not bool(got[:, C:].any()), "pad channels are written as zero"
    assert bool((y[:PAD] == V.SENTINEL).all()) and bool((y[PAD + T0:] == V.SENTINEL).all()), "rows outside the frames are not touched"


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("case", V.gn_case_list(), ids=lambda c: c[0])
def test_groupnorm_kernels_on_the_designed_cases(case, dtype):
    inp, ref = cached(("gn", case[0]), lambda: (lambda i: (i, V.gn_ref(*i)))(V.gn_inputs(*case)))
    y, T0, stats = run_groupnorm(inp, dtype)
    check_groupnorm(y, T0, case[2], ref, dtype, case[0])
    again, _, stats2 = run_groupnorm(inp, dtype)
    assert torch.equal(y, again) and torch.equal(stats, stats2), "two launches give the same bits"


def test_groupnorm_past_2_to_the_31_elements():
    """(16 + 2 097 157) rows x 1024 channels: row offsets past 2^31 elements (and, in bytes, past 2^32)."""
    from speech_decoding_amd import lib
    full = V.gn_inputs(*V.LARGE)
    ref = V.gn_ref(*V.gn_subset(full, V.LARGE_SEL))
    y, T0, _ = run_groupnorm(full, torch.bfloat16)
    PAD = lib.ROW_PAD
    assert T0 == 2 ** 21 + 5 and (PAD + T0) * y.shape[1] > 2 ** 31
    got = y[PAD:PAD + T0][:, V.LARGE_SEL].float().cpu()
    ratio = V.gn_ratio(got, ref, torch.bfloat16)
    print(f"{V.LARGE[0]}: max error / bound = {ratio:.3f}")
    assert ratio <= 1.0, ratio
    assert bool((y[:PAD] == V.SENTINEL).all()) and bool((y[PAD + T0:] == V.SENTINEL).all())
    assert bool((y[PAD + T0 - 1] != V.SENTINEL).all()) and bool((y[PAD] != V.SENTINEL).all()), "first and last frame are written"


def test_groupnorm_zeroes_every_pad_channel_of_a_wider_buffer():
    case = ("int_wide", 5004, 32, True, "int")
    inp = V.gn_inputs(*case)
    for dtype in DTYPES:
        y, T0, _ = run_groupnorm(inp, dtype, Cp=192)                 # two 64-lane groups past the kernel's own
        check_groupnorm(y, T0, 32, V.gn_ref(*inp), dtype, "int_wide")


def test_groupnorm_kernels_refuse_bad_arguments_before_launch():
    from speech_decoding_amd import lib, ops
    wave, w, bias, gamma, beta = [None if t is None else t.to(DEV) for t in V.gn_inputs("r", 5004, 96, True, "int")]
    scratch = torch.empty(ops.w2v_conv0_stats_floats(999, 96), dtype=torch.float32, device=DEV)
    stats = torch.zeros(3, 96, device=DEV)
    y = torch.full((lib.rows_alloc(1, 999), 128), V.SENTINEL, device=DEV)
    with pytest.raises(lib.SdaError):
        ops.w2v_conv0_stats(wave, w, bias, scratch, 0, 96, 10, 5)
    with pytest.raises(lib.SdaError):
        ops.w2v_conv0_stats(wave, w, bias, scratch, 1000, 96, 10, 5)                  # one frame more than the waveform holds
    with pytest.raises(lib.SdaError):
        ops.w2v_conv0_stats(wave, w, bias, scratch[:5 * 96], 999, 96, 10, 5)          # scratch of a single workgroup
    with pytest.raises(lib.SdaError):
        ops.w2v_conv0_stats(wave.cpu(), w, bias, scratch, 999, 96, 10, 5)
    with pytest.raises(lib.SdaError):
        ops.w2v_conv0_groupnorm(wave, w, bias, gamma, beta, stats, y, 0, 96, 10, 5)
    with pytest.raises(lib.SdaError):
        ops.w2v_conv0_groupnorm(wave, w, bias, gamma.cpu(), beta, stats, y, 999, 96, 10, 5)
    with pytest.raises(lib.SdaError):
        ops.w2v_conv0_groupnorm(wave, w, bias, gamma, beta, stats, y[:, :64].contiguous(), 999, 96, 10, 5)     # C > Cp
    with pytest.raises(lib.SdaError):
        ops.w2v_conv0_groupnorm(wave, w, bias, gamma, beta, stats, y[:500], 999, 96, 10, 5)                    # too few rows
    with pytest.raises(lib.SdaError):                                                 # C > Cp at the C entry point itself
        lib.check(lib.load().sda_w2v_conv0_groupnorm(wave.data_ptr(), wave.numel(), w.data_ptr(), None, gamma.data_ptr(), beta.data_ptr(),
                                                     stats.data_ptr(), y.data_ptr(), 999, 96, 64, 10, 5, lib.F32, None))
    torch.cuda.synchronize()
    assert bool((y == V.SENTINEL).all()), "nothing was launched"


# ---------------------------------------------------------------------------------------------------------------
# the embedder end to end
# ---------------------------------------------------------------------------------------------------------------
def variant(dims, norm, stable, seed=0, scale=1.0):
    """(VariantConfig, fp32 state dict, its float64 copy), once per test session"""
    def make():
        cfg = V.VariantConfig(**dict(dims, feat_extract_norm=norm, do_stable_layer_norm=stable, conv_bias=(norm == "layer")))
        sd = V.random_state_dict(cfg, seed, scale, parametrized=stable)
        return cfg, sd, V.to64(sd)
    return cached(("variant", tuple(sorted(dims.items())), norm, stable, seed, scale), make)


def embedder(cfg, sd, dtype):
    from speech_decoding_amd.wav2vec2 import Wav2Vec2Config, Wav2Vec2Embedder
    return Wav2Vec2Embedder(sd, Wav2Vec2Config(**cfg.embedder_kwargs()), dtype=dtype, device=DEV)


def check_hidden_states(dims, norm, stable, n, dtype, seed=0, scale=1.0):
    cfg, sd, sd64 = variant(dims, norm, stable, seed, scale)
    wave = torch.randn(n, generator=torch.Generator().manual_seed(n)) + 0.3
    ref = cached(("hs", tuple(sorted(dims.items())), norm, stable, seed, scale, n), lambda: V.hidden_states(sd64, cfg, wave[None]))
    got = embedder(cfg, sd, dtype).hidden_states(wave)
    assert len(got) == len(ref) == cfg.num_hidden_layers + 1
    assert got[0].shape == ref[0][0].shape == (V.n_frames(n, cfg), cfg.hidden_size)
    for i, (g, r) in enumerate(zip(got, ref)):
        assert torch.isfinite(g).all(), f"hidden state {i}"
        e = V.rel_l2(g.cpu(), r[0])
        print(f"{norm} stable={stable} n={n} {dtype} hidden state {i}: {e:.3e}")
        assert e < REL[dtype], f"hidden state {i}: {e:.3e}"


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("n", [6000, 3217])
@pytest.mark.parametrize("norm,stable", V.COMBOS)
def test_hidden_states_of_the_four_combinations(norm, stable, n, dtype):
    check_hidden_states(V.SMALL, norm, stable, n, dtype)


@pytest.mark.parametrize("dtype", DTYPES)
def test_hidden_states_group_post_ln_mid(dtype):
    check_hidden_states(V.MID, "group", False, 30000, dtype)


@pytest.mark.parametrize("dtype", DTYPES)
def test_hidden_states_at_wav2vec2_base_dimensions(dtype):
    """768 wide, 12 heads, 3072 FFN, 12 post-LN layers, 512 conv channels without bias, group norm: 124 frames"""
    check_hidden_states(V.BASE, "group", False, 40000, dtype, seed=3, scale=0.7)


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("norm,stable", [("group", False), ("group", True)])
def test_ten_chunk_embed_matches_the_chunked_restatement(norm, stable, dtype):
    cfg, sd, sd64 = variant(V.SMALL, norm, stable)
    waveform = torch.randn(1, 20003, generator=torch.Generator().manual_seed(2)) + 0.3
    ref = cached(("embed", norm, stable), lambda: V.w2v_last_four_layers_avg(sd64, cfg, waveform))
    emb = embedder(cfg, sd, dtype)
    got = emb.embed(waveform)
    assert got.shape == ref.shape and got.dtype == torch.float32
    assert V.rel_l2(got.cpu(), ref) < REL[dtype], V.rel_l2(got.cpu(), ref)
    assert torch.equal(emb(waveform), got), "a second call reuses workspace and graphs and gives the same bits"


@pytest.mark.parametrize("stable", [False, True])
def test_graph_replay_equals_eager_launches_for_the_group_variant(stable):
    cfg, sd, _ = variant(V.SMALL, "group", stable)
    emb = embedder(cfg, sd, torch.bfloat16)
    waveform = torch.randn(1, 30011, generator=torch.Generator().manual_seed(5)) + 0.3
    a = emb.embed(waveform)
    b = emb.embed(waveform * 0.5 + 1.0)       # replays with new input (another scale AND another mean: GroupNorm removes neither alone)
    emb.use_graphs = False
    assert torch.equal(emb.embed(waveform), a)
    assert torch.equal(emb.embed(waveform * 0.5 + 1.0), b)
    assert not torch.equal(a, b)


def _long_wave():
    n = 2000003
    g = torch.Generator().manual_seed(9)
    ramp = torch.linspace(0.0, 1.0, n)
    return (torch.randn(n, generator=g) * (0.2 + 1.6 * ramp) + 2.0 * ramp)[None]      # louder and drifting: no chunk has the file's statistics


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_conv_features_take_their_statistics_from_the_whole_file(dtype):
    cfg, sd, sd64 = variant(V.SMALL, "group", False)
    waveform = cached("long_wave", _long_wave)
    ref = cached("long_ref", lambda: V.conv_features(sd64, cfg, waveform)[0])
    n1 = V.chunk_bounds(waveform.shape[1])[0][1]
    chunk = cached("long_chunk", lambda: V.conv_features(sd64, cfg, waveform[:, :n1])[0])      # the first tenth, normalised on its own
    got = embedder(cfg, sd, dtype).conv_features(waveform)
    assert got.shape == ref.shape == (64, V.n_frames(waveform.shape[1], cfg)) and got.dtype == torch.float32 and got.is_cuda
    e = V.rel_l2(got.cpu(), ref)
    print(f"conv_features {dtype}: {e:.3e}")
    assert e < REL[dtype], e
    f1 = chunk.shape[1]
    assert V.rel_l2(got[:, :f1].cpu(), chunk) > 10 * REL[dtype], "per-chunk statistics would have passed"
    assert V.rel_l2(got[:, :f1].cpu(), ref[:, :f1]) < 10 * REL[dtype]


def test_feature_extractor_is_the_drop_in():
    cfg, sd, sd64 = variant(V.SMALL, "group", False)
    waveform = torch.randn(1, 8000, generator=torch.Generator().manual_seed(6)) + 0.3
    emb = embedder(cfg, sd, torch.float32)
    out = emb.feature_extractor(waveform)
    assert out.device.type == "cpu" and out.dtype == torch.float32 and out.shape == (1, 64, V.n_frames(8000, cfg))
    assert V.rel_l2(out, V.conv_features(sd64, cfg, waveform)) < REL[torch.float32]
    assert out.squeeze().numpy().shape == (64, V.n_frames(8000, cfg))                  # gwilliams2022.py:360
    assert torch.equal(emb.conv_features(waveform[0]).cpu(), out[0])                   # (L,) as well as (1, L)


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_speech_embeddings_without_last4layers_keeps_the_layer_norm_variants_bits(dtype):
    """speech_embeddings(last4layers=False) runs conv_features; for xlsr-53's variant the result is bit-equal to the route it
    took before: the whole transformer run for its `taps`."""
    from speech_decoding_amd import signal_prep as SP
    from speech_decoding_amd.wav2vec2 import resample_fft
    cfg, sd, _ = variant(V.SMALL, "layer", True)
    emb = embedder(cfg, sd, dtype)
    pre = {"lowpass_filter_width": 128, "last4layers": False, "brain_resample_rate": 120}
    wave = (torch.randn(1, 30000, generator=torch.Generator().manual_seed(3)) + 0.1).to(DEV)
    got = SP.speech_embeddings(emb, wave, 44100, pre)
    wave16 = SP.resample_audio(wave, 44100, 16000, lowpass_filter_width=128)
    emb.taps = {}
    emb.hidden_states(wave16[0])
    old = emb.taps["feat6"].t()
    emb.taps = None
    assert torch.equal(emb.conv_features(wave16), old)
    rate_after = 16000 * old.shape[-1] / wave16.shape[-1]
    assert torch.equal(got, resample_fft(old, up=120 / rate_after))


def _fixture(name):
    from tests.test_w2v2_variants_cpu import _fixture as load
    return load(name)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("name", ["w2v2_group_postln.npz", "w2v2_group_stable.npz"])
def test_reference_function_fixtures(name, dtype):
    """Outputs of the REFERENCE's getW2VLastFourLayersAvg, of HF `output_hidden_states` and of HF `feature_extractor` on a
    seeded HF model of each variant (tests/golden/make_w2v2_variants_golden.py)."""
    kw, sd, z = _fixture(name)
    emb = embedder(V.VariantConfig(**kw), sd, dtype)
    waveform = torch.from_numpy(z["waveform"])
    got = emb.embed(waveform)
    assert got.shape == z["expected"].shape and got.dtype == torch.float32
    assert V.rel_l2(got.cpu(), torch.from_numpy(z["expected"])) < REL[dtype]
    for i, h in enumerate(emb.hidden_states(waveform[0, :4000])):
        assert V.rel_l2(h.cpu(), torch.from_numpy(z[f"hs/{i}"])) < REL[dtype], i
    feat = emb.feature_extractor(waveform)
    assert feat.shape == z["feat"].shape
    assert V.rel_l2(feat, torch.from_numpy(z["feat"])) < REL[dtype]


def test_from_hf_builds_from_a_group_norm_post_ln_model():
    """`load_wav2vec_model("facebook/wav2vec2-base-960h")`-style use: an HF model object in, the shim's two calls out."""
    tr = pytest.importorskip("transformers")
    from speech_decoding.utils import wav2vec_util as shim
    kw, sd, z = _fixture("w2v2_group_postln.npz")
    model = tr.Wav2Vec2Model(tr.Wav2Vec2Config(**V.VariantConfig(**kw).hf_kwargs())).eval()
    missing = model.load_state_dict(sd, strict=False)
    assert set(missing.missing_keys) <= {"masked_spec_embed"}
    old, shim.COMPUTE_DTYPE = shim.COMPUTE_DTYPE, torch.float32
    try:
        out = shim.getW2VLastFourLayersAvg(model, torch.from_numpy(z["waveform"]))
        feats = model._sda_embedder.feature_extractor(torch.from_numpy(z["waveform"])).squeeze()
    finally:
        shim.COMPUTE_DTYPE = old
    assert out.device.type == "cpu" and out.dtype == torch.float32
    np.testing.assert_allclose(out.numpy(), z["expected"], rtol=1e-3, atol=1e-4)
    np.testing.assert_allclose(feats.numpy(), z["feat"][0], rtol=1e-3, atol=1e-4)
