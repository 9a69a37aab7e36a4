"""The signal-conditioning path on MI355X: `sda_window_gemm_f32` (csrc/window_gemm.hip) with torch.equal on integer operands,
its memory contract under NaN guards, the fp32 summation bound on real operands, and the public functions of
speech_decoding_amd/signal_prep.py against the float64 restatements of tests/signal_cases.py (tests/test_signal_prep_cpu.py
proves on the CPU that those cases see the bugs this kernel can have)."""
import numpy as np
import pytest
import torch

from tests import signal_cases as SC

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
SHAPE_IDS = [f"S{s}-K{k}-N{n}" for s, k, n, _ in SC.KERNEL_SHAPES]


def run_kernel(x, B, S, frames, x_stride=None, out=None, out_stride=None):
    """x (rows, Lx) fp32 device, B (K, N) fp32 device -> the raw entry point's output (rows, out_stride)"""
    from speech_decoding_amd import lib as L
    rows = x.shape[0]
    K, N = B.shape
    x_stride = x.stride(0) if x_stride is None else x_stride
    out_stride = frames * N if out_stride is None else out_stride
    if out is None:
        out = torch.empty(rows, out_stride, dtype=torch.float32, device=x.device)
    L.check(L.load().sda_window_gemm_f32(x.data_ptr(), x_stride, rows, frames, S, K, B.data_ptr(), N, out.data_ptr(), out_stride,
                                         torch.cuda.current_stream().cuda_stream), "window_gemm")
    return out


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dtype=torch.float32, device=DEV)


@pytest.mark.parametrize("S,K,N,why", SC.KERNEL_SHAPES, ids=SHAPE_IDS)
def test_integer_operands_are_reproduced_exactly(S, K, N, why):
    B = SC.ints((K, N), 4, 7 * S + K)
    for rows, frames in SC.kernel_runs(S, K, N):
        x = SC.ints((rows, (frames - 1) * S + K), 8, rows * 100 + frames)
        ref = SC.window_gemm(x, B, S, frames)
        assert np.abs(ref).max() < 2 ** 24
        got = run_kernel(dev(x), dev(B), S, frames)
        assert torch.equal(got.cpu(), torch.from_numpy(ref).float()), f"rows {rows}, frames {frames}: {why}"


@pytest.mark.parametrize("S,K,N,why", SC.KERNEL_SHAPES, ids=SHAPE_IDS)
def test_nothing_is_read_or_written_outside_the_contract(S, K, N, why):
    """every row's input ends inside a larger allocation with NaN right behind its last needed sample, the output rows are
    wider than frames * N and NaN-filled: no NaN reaches an output, every guard element stays NaN"""
    B = SC.ints((K, N), 4, 7 * S + K)
    runs = SC.kernel_runs(S, K, N)
    for rows, frames in sorted(set(runs[:1] + runs[-2:])):
        need = (frames - 1) * S + K
        x = SC.ints((rows, need), 8, rows * 100 + frames)
        xs = need + 5
        xg = torch.full((rows * xs + 64,), float("nan"), dtype=torch.float32, device=DEV)
        xg[:rows * xs].view(rows, xs)[:, :need] = dev(x)
        os_ = frames * N + 3
        og = torch.full((rows * os_ + 64,), float("nan"), dtype=torch.float32, device=DEV)
        run_kernel(xg[:rows * xs].view(rows, xs), dev(B), S, frames, x_stride=xs, out=og, out_stride=os_)
        body = og[:rows * os_].view(rows, os_).cpu()
        assert torch.equal(body[:, :frames * N], torch.from_numpy(SC.window_gemm(x, B, S, frames)).float()), why
        assert torch.isnan(body[:, frames * N:]).all() and torch.isnan(og[rows * os_:]).all(), why
        assert torch.isnan(xg[:rows * xs].view(rows, xs)[:, need:]).all()


@pytest.mark.parametrize("S,K,N,why", [c for c in SC.KERNEL_SHAPES if c[1] <= 318], ids=[i for i, c in zip(SHAPE_IDS, SC.KERNEL_SHAPES) if c[1] <= 318])
def test_real_operands_stay_inside_the_summation_bound(S, K, N, why):
    rows, frames = 3, 37
    rs = np.random.RandomState(S + K + N)
    x = rs.randn(rows, (frames - 1) * S + K).astype(np.float32).astype(np.float64)
    B = rs.randn(K, N).astype(np.float32).astype(np.float64)
    ref, lim = SC.window_gemm(x, B, S, frames), SC.bound(x, B, S, frames)
    got = run_kernel(dev(x), dev(B), S, frames).cpu().double().numpy()
    err = np.abs(got - ref)
    print(f"S {S} K {K} N {N}: max err / bound = {(err / lim).max():.3e}")
    assert (err <= lim).all(), why
    # the bound has teeth: the contribution of one tap (what a dropped tap would lose) exceeds it almost everywhere
    last = SC.windows(x, S, K, frames)[:, :, K - 1, None] * B[K - 1][None, None, :]
    assert (np.abs(last.reshape(ref.shape)) > lim).mean() > 0.9


FIR_CASES = [((3, 700), "longer than the filter"), ((2, 150), "shorter than the filter"), ((2, 3, 64), "leading dimensions")]


@pytest.mark.parametrize("shape,why", FIR_CASES, ids=[w for _, w in FIR_CASES])
def test_fir_filter_and_filter_data_match_the_restatement(shape, why):
    from speech_decoding_amd import signal_prep as SP
    taps = SP.bandpass_taps(120, 2, 30)
    assert len(taps) == 199
    x = SC.dyadic(shape, 5)                                           # fp32-exact, and so is its odd extension
    t32 = taps.astype(np.float32).astype(np.float64)                  # the taps as the kernel receives them
    rows = x.reshape(-1, shape[-1])
    ref, lim = SC.fir_same(rows, t32).reshape(shape), SC.fir_bound(rows, t32).reshape(shape)
    xd = torch.from_numpy(x).to(DEV)
    for got in (SP.fir_filter(xd, taps), SP.filter_data(xd, 120, 2, 30), SP.fir_filter(xd.float(), taps)):
        assert got.shape == xd.shape and got.dtype == torch.float32 and got.is_contiguous()
        err = np.abs(got.cpu().double().numpy() - ref)
        print(f"{why}: max err / bound = {(err / lim).max():.3e}")
        assert (err <= lim).all(), why


@pytest.mark.parametrize("rates", [(44100, 16000, 128), (16000, 44100, 6), (48000, 16000, 6)], ids=lambda r: f"{r[0]}-{r[1]}")
@pytest.mark.parametrize("rows", [1, 2])
def test_resample_audio_matches_the_restatement(rates, rows):
    from speech_decoding_amd import signal_prep as SP
    orig_f, new_f, lpw = rates
    bank, width, orig, new = SC.sinc_bank(orig_f, new_f, lpw)
    b32 = bank.astype(np.float32).astype(np.float64)
    x = np.random.RandomState(rows).randn(rows, 5000).astype(np.float32).astype(np.float64)
    ref, lim = SC.resample(x, b32, width, orig, new), SC.resample_bound(x, b32, width, orig, new)
    got = SP.resample_audio(torch.from_numpy(x).float().to(DEV), orig_f, new_f, lowpass_filter_width=lpw)
    assert got.shape == ref.shape == (rows, -(-new * 5000 // orig)) and got.dtype == torch.float32
    err = np.abs(got.cpu().double().numpy() - ref)
    print(f"{rates}: max err / bound = {(err / np.maximum(lim, 1e-300)).max():.3e}")
    assert (err <= lim).all()
    same = torch.randn(2, 10, device=DEV)
    assert SP.resample_audio(same, 16000, 16000) is same


def test_brain_preproc_is_filter_then_fft_resampling():
    from oracle import wav2vec2_oracle as W
    from speech_decoding_amd import signal_prep as SP
    pre = {"brain_filter_low": 1.0, "brain_filter_high": 60, "brain_resample_rate": 120}
    raw = torch.from_numpy(SC.dyadic((4, 3000), 9)).float().to(DEV)
    got = SP.brain_preproc(raw, 1000, pre)
    assert got.shape == (4, 360) and got.dtype == torch.float32
    # the resampling stage in float64 on the GPU filter's own fp32 output (the filter is bounded separately above) ...
    from speech_decoding_amd.wav2vec2 import resample_fft
    filtered = SP.filter_data(raw, 1000, 1.0, 60)
    ref = W.resample_fft(filtered.cpu().double().numpy(), 120 / 1000)
    y64 = resample_fft(filtered, 120 / 1000)
    assert y64.dtype == torch.float64
    np.testing.assert_allclose(y64.cpu().numpy(), ref, rtol=0, atol=1e-10 * np.abs(ref).max())
    # ... and brain_preproc is exactly that chain, stored as fp32
    assert torch.equal(got, y64.float())


@pytest.mark.parametrize("last4", [True, False])
def test_speech_embeddings_chain_shapes(last4):
    from oracle import wav2vec2_oracle as W
    from speech_decoding_amd import signal_prep as SP
    from speech_decoding_amd.wav2vec2 import Wav2Vec2Config, Wav2Vec2Embedder, chunk_bounds
    from tests.test_wav2vec2_gpu import SMALL
    ocfg = W.W2V2Config(**SMALL)
    emb = Wav2Vec2Embedder(W.random_state_dict(ocfg, 0), Wav2Vec2Config(**SMALL), dtype=torch.float32, device=DEV)
    pre = {"lowpass_filter_width": 128, "last4layers": last4, "brain_resample_rate": 120}
    n = 30000
    wave = torch.randn(1, n, generator=torch.Generator().manual_seed(3)).to(DEV)
    got = SP.speech_embeddings(emb, wave, 44100, pre)
    n16 = -(-160 * n // 441)
    if last4:
        frames, feat = sum(W.n_frames(b - a, ocfg) for a, b in chunk_bounds(n16)), ocfg.hidden_size
    else:
        frames, feat = W.n_frames(n16, ocfg), ocfg.conv_dim[-1]
    rate_after = 16000 * frames / n16
    assert got.shape == (feat, int(round(frames * (120 / rate_after)))) and got.dtype == torch.float64
    assert torch.isfinite(got).all()
    # the chain restated: the same resampled waveform through the embedder, then FFT resampling
    wave16 = SP.resample_audio(wave, 44100, 16000, lowpass_filter_width=128)
    assert wave16.shape == (1, n16)
    if last4:
        ref = W.resample_fft(emb.embed(wave16).cpu().double().numpy(), 120 / rate_after)
        np.testing.assert_allclose(got.cpu().numpy(), ref, rtol=0, atol=1e-10 * np.abs(ref).max())
