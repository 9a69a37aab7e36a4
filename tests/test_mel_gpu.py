"""The log-mel path on MI355X: `sda_mel_power_f32` (csrc/mel_power.hip) with torch.equal on integer operands, its memory
contract under NaN guards, the relative fp32 bound on real operands with and without the log, and the public functions of
speech_decoding_amd/signal_prep.py (stft, mel_spectrogram, log_mel, mel_embeddings) against the float64 restatements and
error budgets of tests/mel_cases.py (tests/test_mel_cpu.py proves on the CPU that those cases and bounds see the bugs this
path can have)."""
import math

import numpy as np
import pytest
import torch

from speech_decoding_amd import log_mel, mel_embeddings, mel_spectrogram      # noqa: F401  (the module tests this feature only)
from tests import mel_cases as MC

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
NAN = float("nan")


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dtype=torch.float32, device=DEV)


def run_kernel(spec, fb, log_eps=None, slack=(0, 0), guards=False):
    """spec (rows, frames, n_freqs, 2), fb (n_freqs, n_mels) host arrays -> the raw entry point's output (rows, n_mels, frames)
    on the host.  slack = floats added to (spec_pitch, out_pitch); rows are then further apart than they need to be as well,
    everything between and around is NaN, and `out` starts one float into its allocation (an odd float offset: no 16-byte
    alignment anywhere).  guards=True also returns (spec buffer, out buffer, out view) for the guard checks."""
    from speech_decoding_amd import lib as L
    rows, frames, n_freqs, _ = spec.shape
    n_mels = fb.shape[1]
    sp, op = 2 * n_freqs + slack[0], frames + slack[1]
    srs, ors = frames * sp + (2 if slack[0] else 0), n_mels * op + (7 if slack[1] else 0)
    lead = 1 if slack[1] else 0
    sbuf = torch.full((rows * srs + 64,), NAN, dtype=torch.float32, device=DEV)
    sview = sbuf[:rows * srs].view(rows, srs)[:, :frames * sp].reshape(rows, frames, sp)
    sview[:, :, :2 * n_freqs] = dev(spec).reshape(rows, frames, 2 * n_freqs)
    obuf = torch.full((lead + rows * ors + 64,), NAN, dtype=torch.float32, device=DEV)
    fbd = dev(fb)
    L.check(L.load().sda_mel_power_f32(sbuf.data_ptr(), srs, sp, rows, frames, n_freqs, fbd.data_ptr(), n_mels,
                                       -1.0 if log_eps is None else float(log_eps), obuf.data_ptr() + 4 * lead, ors, op,
                                       torch.cuda.current_stream().cuda_stream), "mel_power")
    oview = obuf[lead:lead + rows * ors].view(rows, ors)[:, :n_mels * op].reshape(rows, n_mels, op)
    got = oview[:, :, :frames].cpu()
    return (got, sbuf, obuf, oview) if guards else got


@pytest.mark.parametrize("n_freqs,n_mels,why", MC.KERNEL_SHAPES, ids=MC.SHAPE_IDS)
def test_integer_operands_are_reproduced_exactly(n_freqs, n_mels, why):
    for rows, frames in MC.kernel_runs():
        spec, fb = MC.int_operands(n_freqs, n_mels, rows, frames)
        ref = MC.mel_power(spec, fb)
        assert ref.max() < 2 ** 24
        for slack in MC.SLACKS:
            got = run_kernel(spec, fb, slack=slack)
            assert torch.equal(got, torch.from_numpy(ref).float()), f"rows {rows}, frames {frames}, slack {slack}: {why}"


@pytest.mark.parametrize("n_freqs,n_mels,why", MC.KERNEL_SHAPES, ids=MC.SHAPE_IDS)
def test_nothing_is_read_or_written_outside_the_contract(n_freqs, n_mels, why):
    """the slack of every frame and row of spec is NaN, `out` lies in a NaN-filled allocation at an odd float offset with pitches
    wider than frames: no NaN reaches an output, every guard element keeps its bits, and the result is the unpadded call's"""
    for rows, frames in MC.kernel_runs():
        spec, fb = MC.int_operands(n_freqs, n_mels, rows, frames)
        for log_eps in (None, MC.EPS):
            plain = run_kernel(spec, fb, log_eps)
            got, sbuf, obuf, oview = run_kernel(spec, fb, log_eps, slack=MC.SLACKS[1], guards=True)
            assert torch.isfinite(got).all(), why
            assert torch.equal(got, plain), why
            written = torch.zeros(obuf.shape, dtype=torch.bool, device=DEV)
            lead, ors, op = 1, n_mels * (frames + 5) + 7, frames + 5
            written[lead:lead + rows * ors].view(rows, ors)[:, :n_mels * op].reshape(rows, n_mels, op)[:, :, :frames] = True
            untouched = torch.full_like(obuf, NAN)
            assert torch.equal(obuf.view(torch.int32)[~written], untouched.view(torch.int32)[~written]), why
            assert int(written.sum()) == rows * n_mels * frames
            assert int(torch.isnan(sbuf).sum()) == sbuf.numel() - rows * frames * 2 * n_freqs       # the input is left alone


@pytest.mark.parametrize("n_freqs,n_mels,why", MC.KERNEL_SHAPES, ids=MC.SHAPE_IDS)
def test_real_operands_stay_inside_the_relative_bound(n_freqs, n_mels, why):
    worst = 0.0
    for rows, frames in MC.kernel_runs():
        spec, fb = MC.real_operands(n_freqs, n_mels, rows, frames)
        ref = MC.mel_power(spec, fb)
        for slack in MC.SLACKS:
            got = run_kernel(spec, fb, slack=slack).double().numpy()
            q = MC.miss(got, ref, MC.rel_bound(n_freqs) * ref)
            worst = max(worst, q)
            assert q <= 1, f"rows {rows}, frames {frames}, slack {slack}: {why}"
    print(f"F {n_freqs} M {n_mels}: max err / bound = {worst:.3e}")


@pytest.mark.parametrize("n_freqs,n_mels,why", MC.KERNEL_SHAPES, ids=MC.SHAPE_IDS)
def test_log_compression_stays_inside_its_bound(n_freqs, n_mels, why):
    worst = 0.0
    log_eps32 = math.log(float(np.float32(MC.EPS)))
    # the device's logf(log_eps + 0): one bin, one filter, all zero
    logf_eps = float(run_kernel(np.zeros((1, 1, 1, 2)), np.zeros((1, 1)), MC.EPS)[0, 0, 0])
    assert abs(logf_eps - log_eps32) <= MC.LOGF_REL * abs(log_eps32)
    for rows, frames in MC.kernel_runs():
        # small operands, so that eps matters (mel ~ 1e-5 n_freqs); one all-zero filter column
        spec, fb = MC.real_operands(n_freqs, n_mels, rows, frames, scale=2.0 ** -9, zero_column=n_mels > 1)
        ref = MC.mel_power(spec, fb, MC.EPS)
        lim = MC.log_bound(ref, MC.rel_bound(n_freqs))
        for slack in MC.SLACKS:
            got = run_kernel(spec, fb, MC.EPS, slack=slack).double().numpy()
            q = MC.miss(got, ref, lim)
            worst = max(worst, q)
            assert q <= 1, f"rows {rows}, frames {frames}, slack {slack}: {why}"
            if n_mels > 1:
                # mel is exactly zero there: every element is exactly logf(eps)
                assert (got[:, n_mels // 2, :] == logf_eps).all()
    print(f"F {n_freqs} M {n_mels}: max log err / bound = {worst:.3e}")


def test_zero_input_gives_logf_of_eps_everywhere_and_the_same_bits_on_every_call():
    spec, fb = MC.real_operands(257, 120, 3, 129)
    a = run_kernel(spec, fb, MC.EPS, slack=MC.SLACKS[1])
    for _ in range(3):
        assert torch.equal(run_kernel(spec, fb, MC.EPS, slack=MC.SLACKS[1]), a)
    z = run_kernel(np.zeros_like(spec), fb, MC.EPS)
    assert (z == z.flatten()[0]).all() and abs(float(z.flatten()[0]) - math.log(float(np.float32(MC.EPS)))) < 1e-5


# ---------------------------------------------------------------------------------------------------------------
# the public functions
# ---------------------------------------------------------------------------------------------------------------
def product_matrices(params):
    """the fp32 matrices the product uploads, as float64"""
    import warnings
    from speech_decoding_amd import signal_prep as SP
    n_fft, sr = params["n_fft"], params["sample_rate"]
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        fb = SP.mel_filterbank(n_fft // 2 + 1, 0.0, float(sr // 2), params["n_mels"], sr)
    return SP.stft_matrix(n_fft).astype(np.float32).astype(np.float64), fb.astype(np.float32).astype(np.float64)


@pytest.mark.parametrize("params", [MC.PAPER, MC.SMALL], ids=["paper", "small"])
@pytest.mark.parametrize("L", MC.E2E_LENGTHS)
def test_stft_mel_spectrogram_and_log_mel_match_the_restatement(params, L):
    from speech_decoding_amd import log_mel, mel_spectrogram
    from speech_decoding_amd import signal_prep as SP
    n_fft, hop, n_mels, sr = params["n_fft"], params["hop_length"], params["n_mels"], params["sample_rate"]
    x = MC.audio(L)
    B, fb = product_matrices(params)
    ref = MC.e2e(x, B, fb, n_fft, hop)
    frames = 1 + L // hop
    xd = torch.from_numpy(x).float().to(DEV)
    spec = SP.stft(xd, n_fft, hop)
    mel = mel_spectrogram(xd, sr, n_fft, hop, n_mels)
    lm = log_mel(xd, sr, n_fft, hop, n_mels)
    assert spec.shape == (2, frames, n_fft // 2 + 1, 2) and mel.shape == lm.shape == (2, n_mels, frames)
    for t in (spec, mel, lm):
        assert t.dtype == torch.float32 and t.is_contiguous()
    for name, got in (("spec", spec), ("mel", mel), ("logmel", lm)):
        q = MC.miss(got.cpu().double().numpy(), ref[name], ref[name + "_lim"])
        print(f"L {L} n_fft {n_fft} {name}: max err / bound = {q:.3e}")
        assert q <= 1, name
    assert (ref["rho"] < 0.5).all()
    # leading dimensions, float64 input and the default arguments (the paper's) are the same computation
    if params is MC.PAPER:
        assert torch.equal(log_mel(xd.double().reshape(2, 1, L)), lm.reshape(2, 1, n_mels, frames))
        assert torch.equal(mel_spectrogram(xd, log_eps=MC.EPS), lm)


def test_stft_refuses_what_torch_refuses():
    from speech_decoding_amd import SdaError
    from speech_decoding_amd import signal_prep as SP
    with pytest.raises(SdaError, match="reflection"):
        SP.stft(torch.zeros(2, 256, device=DEV))                     # L <= n_fft // 2
    assert SP.stft(torch.zeros(2, 257, device=DEV)).shape == (2, 3, 257, 2)
    with pytest.raises(SdaError, match="fewer"):
        SP.stft(torch.zeros(2, 511, device=DEV), center=False)
    assert SP.stft(torch.zeros(1, 512 + 128, device=DEV), center=False).shape == (1, 2, 257, 2)


def test_mel_embeddings_is_resample_log_mel_resample_and_feeds_the_segment_feed():
    from speech_decoding_amd import log_mel, mel_embeddings
    from speech_decoding_amd import signal_prep as SP
    from speech_decoding_amd.data import ResidentSegmentFeed
    from speech_decoding_amd.wav2vec2 import resample_fft
    pre = {"lowpass_filter_width": 128, "last4layers": False, "brain_resample_rate": 120}
    n = 22050
    wave = torch.from_numpy(MC.audio(n, rows=1)).float().to(DEV)
    got = mel_embeddings(wave, 44100, pre)
    wave16 = SP.resample_audio(wave, 44100, 16000, lowpass_filter_width=128)
    frames = 1 + wave16.shape[1] // 128
    ref = resample_fft(log_mel(wave16)[0], up=120 / 125)
    assert got.dtype == torch.float64 and got.shape == (120, int(round(frames * 120 / 125)))
    assert torch.equal(got, ref)
    small = mel_embeddings(wave, 44100, dict(pre, mel={"n_mels": 10, "n_fft": 64, "hop_length": 16, "eps": 1e-3}))
    assert small.shape == (10, int(round((1 + wave16.shape[1] // 16) * 120 / 1000)))
    assert torch.equal(small, resample_fft(log_mel(wave16, n_fft=64, hop_length=16, n_mels=10, eps=1e-3)[0], up=120 / 1000))
    # the speech table of a segment feed: segments of T frames cut from the result, as they are
    T, N = 15, 4
    Y = torch.stack([got[:, i * T:(i + 1) * T] for i in range(N)]).float()
    recs = [torch.randn(6, 200, generator=torch.Generator().manual_seed(r)).to(DEV) for r in range(2)]
    feed = ResidentSegmentFeed(recs, [0, 1], [0, 0], [np.arange(N) * 40] * 2, np.zeros(N, dtype=np.int64), np.arange(N), Y,
                               seq_len_samp=T, baseline_len_samp=5, clamp_lim=20.0)
    X, Yb, subj = feed.batch([2, 0, 3])
    assert X.shape == (3, 6, T) and torch.equal(Yb, Y[[2, 0, 3]]) and Yb.shape == (3, 120, T)
