"""The FFT path of the STFT on MI355X: `sda_stft_fft_f32` (csrc/stft_fft.hip) with torch.equal on the exact cases, its memory
contract under NaN guards, the derived per-frame bound on real operands at every size / hop / row / frame / pitch case, the
same bits on every call, and the public functions of speech_decoding_amd/signal_prep.py with algorithm="fft" (stft,
mel_spectrogram, log_mel, mel_embeddings) against the float64 restatement and budgets of tests/fft_cases.py
(tests/test_stft_fft_cpu.py proves on the CPU that those cases and the bound see the bugs this kernel can have)."""
import numpy as np
import pytest
import torch

from speech_decoding_amd.signal_prep import fft_twiddles, stft_window      # noqa: F401  (the module tests this feature only)
from tests import fft_cases as FC
from tests import mel_cases as MC

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
NAN = float("nan")


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dtype=torch.float32, device=DEV)


def run_kernel(x, window, twiddle, hop, frames, n_fft, slack=(0, 0), guards=False):
    """x (rows, (frames - 1) hop + n_fft), window (n_fft,), twiddle (n_fft / 2, 2) host arrays -> the raw entry point's output
    (rows, frames, n_freqs, 2) on the host.  slack = floats added to (x_row_stride, out_pitch); the rows of `out` are then
    further apart than they need to be as well, everything between and around x's rows and out's frames is NaN, and both x
    and out start one float into their allocations (odd float offsets: no 8- or 16-byte alignment anywhere).  guards=True also
    returns (x buffer, out buffer) for the guard checks."""
    from speech_decoding_amd import lib as L
    rows, need = x.shape
    assert need == (frames - 1) * hop + n_fft
    nf2 = n_fft + 2
    xrs, op = need + slack[0], nf2 + slack[1]
    ors = frames * op + (7 if slack[1] else 0)
    lead = 1 if (slack[0] or slack[1]) else 0
    xbuf = torch.full((lead + rows * xrs + 64,), NAN, dtype=torch.float32, device=DEV)
    xbuf[lead:lead + rows * xrs].view(rows, xrs)[:, :need] = dev(x)
    obuf = torch.full((lead + rows * ors + 64,), NAN, dtype=torch.float32, device=DEV)
    wd, td = dev(window), dev(twiddle)
    L.check(L.load().sda_stft_fft_f32(xbuf.data_ptr() + 4 * lead, xrs, rows, frames, hop, n_fft, wd.data_ptr(), td.data_ptr(),
                                      obuf.data_ptr() + 4 * lead, ors, op, torch.cuda.current_stream().cuda_stream), "stft_fft")
    oview = obuf[lead:lead + rows * ors].view(rows, ors)[:, :frames * op].reshape(rows, frames, op)
    got = oview[:, :, :nf2].reshape(rows, frames, nf2 // 2, 2).cpu()
    return (got, xbuf, obuf) if guards else got


@pytest.mark.parametrize("n_fft", FC.N_FFTS)
def test_constant_frames_are_reproduced_exactly(n_fft):
    """window of ones, hop = n_fft, frame (r, m) = its own small integer (with alternating sign: only the Nyquist bin): bin 0 is
    exactly n_fft c and every other float exactly zero — an addressing test for frames, rows and pitches"""
    ones, tw = np.ones(n_fft), FC.product_tables(n_fft)[1]
    for rows in FC.ROWS:
        for frames in FC.frame_counts(n_fft):
            for alternating in (False, True):
                x, ref = FC.constant_frames(n_fft, rows, frames, alternating)
                assert np.abs(ref).max() < 2 ** 24
                for slack in FC.SLACKS:
                    got = run_kernel(x, ones, tw, n_fft, frames, n_fft, slack=slack)
                    assert torch.equal(got, torch.from_numpy(ref).float()), f"rows {rows}, frames {frames}, slack {slack}, alternating {alternating}"
            z = run_kernel(np.zeros((rows, frames * n_fft)), ones, tw, n_fft, frames, n_fft, slack=FC.SLACKS[1])
            assert torch.equal(z, torch.zeros_like(z))


@pytest.mark.parametrize("n_fft", FC.N_FFTS)
def test_nothing_is_read_or_written_outside_the_contract(n_fft):
    """the slack of every row of x is NaN, `out` lies in a NaN-filled allocation at an odd float offset with a pitch wider than
    2 n_freqs: no NaN reaches an output, every guard element keeps its bits, and the result is the unpadded call's"""
    w, tw = FC.product_tables(n_fft)
    nf2 = n_fft + 2
    for hop, rows, frames in FC.kernel_runs(n_fft):
        x = FC.real_operands(n_fft, hop, rows, frames)
        plain = run_kernel(x, w, tw, hop, frames, n_fft)
        got, xbuf, obuf = run_kernel(x, w, tw, hop, frames, n_fft, slack=FC.SLACKS[1], guards=True)
        why = f"hop {hop}, rows {rows}, frames {frames}"
        assert torch.isfinite(got).all(), why
        assert torch.equal(got, plain), why
        written = torch.zeros(obuf.shape, dtype=torch.bool, device=DEV)
        lead, op = 1, nf2 + 5
        ors = frames * op + 7
        written[lead:lead + rows * ors].view(rows, ors)[:, :frames * op].reshape(rows, frames, op)[:, :, :nf2] = True
        untouched = torch.full_like(obuf, NAN)
        assert torch.equal(obuf.view(torch.int32)[~written], untouched.view(torch.int32)[~written]), why
        assert int(written.sum()) == rows * frames * nf2
        assert not torch.isnan(obuf[written]).any(), why
        assert int(torch.isnan(xbuf).sum()) == xbuf.numel() - rows * x.shape[1]          # the input is left alone
        # the imaginary parts of bin 0 and of the Nyquist bin are exact zeros
        assert (got[:, :, 0, 1] == 0).all() and (got[:, :, n_fft // 2, 1] == 0).all(), why


@pytest.mark.parametrize("n_fft", FC.N_FFTS)
def test_real_operands_stay_inside_the_derived_bound(n_fft):
    w, tw = FC.product_tables(n_fft)
    worst = worst_el = 0.0
    for hop, rows, frames in FC.kernel_runs(n_fft):
        for kind in range(4 if (rows, frames) == (3, 37) else 1):
            x = FC.real_operands(n_fft, hop, rows, frames, kind)
            ref = FC.restate(x, w, hop, frames, n_fft)
            for slack in FC.SLACKS:
                got = run_kernel(x, w, tw, hop, frames, n_fft, slack=slack).double().numpy()
                q = FC.miss(got, ref, n_fft)
                qe = MC.miss(got, ref, FC.elementwise_budget(ref, n_fft))
                worst, worst_el = max(worst, q), max(worst_el, qe)
                assert q <= 1 and qe <= 1, f"hop {hop}, rows {rows}, frames {frames}, kind {kind}, slack {slack}: {q} {qe}"
    print(f"n_fft {n_fft}: max err / bound = {worst:.3e} ({worst * FC.rel_bound(n_fft) / FC.U:.2f} u), elementwise {worst_el:.3e}")


def test_the_same_bits_on_every_call():
    for n_fft, hop, rows, frames in ((512, 128, 3, 37), (64, 67, 3, 33)):
        w, tw = FC.product_tables(n_fft)
        x = FC.real_operands(n_fft, hop, rows, frames)
        a = run_kernel(x, w, tw, hop, frames, n_fft, slack=FC.SLACKS[1])
        for _ in range(3):
            assert torch.equal(run_kernel(x, w, tw, hop, frames, n_fft, slack=FC.SLACKS[1]), a)


# ---------------------------------------------------------------------------------------------------------------
# the public functions
# ---------------------------------------------------------------------------------------------------------------
def product_matrices(params):
    """the fp32 window GEMM matrix and filterbank the product uploads, as float64"""
    import warnings
    from speech_decoding_amd import signal_prep as SP
    n_fft, sr = params["n_fft"], params["sample_rate"]
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        fb = SP.mel_filterbank(n_fft // 2 + 1, 0.0, float(sr // 2), params["n_mels"], sr)
    return SP.stft_matrix(n_fft).astype(np.float32).astype(np.float64), fb.astype(np.float32).astype(np.float64)


@pytest.mark.parametrize("params", [MC.PAPER, MC.SMALL], ids=["paper", "small"])
@pytest.mark.parametrize("L", MC.E2E_LENGTHS)
def test_stft_mel_spectrogram_and_log_mel_on_the_fft_match_the_restatement(params, L):
    from speech_decoding_amd import log_mel, mel_spectrogram
    from speech_decoding_amd import signal_prep as SP
    n_fft, hop, n_mels, sr = params["n_fft"], params["hop_length"], params["n_mels"], params["sample_rate"]
    x = MC.audio(L)
    B, fb = product_matrices(params)
    w, _ = FC.product_tables(n_fft)
    ref = FC.e2e(x, w, fb, n_fft, hop)
    ref_gemm = MC.e2e(x, B, fb, n_fft, hop)
    frames = 1 + L // hop
    xd = torch.from_numpy(x).float().to(DEV)
    gemm = {"spec": SP.stft(xd, n_fft, hop), "mel": mel_spectrogram(xd, sr, n_fft, hop, n_mels), "logmel": log_mel(xd, sr, n_fft, hop, n_mels)}
    fft = {"spec": SP.stft(xd, n_fft, hop, algorithm="fft"), "mel": mel_spectrogram(xd, sr, n_fft, hop, n_mels, algorithm="fft"),
           "logmel": log_mel(xd, sr, n_fft, hop, n_mels, algorithm="fft")}
    assert fft["spec"].shape == (2, frames, n_fft // 2 + 1, 2) and fft["mel"].shape == fft["logmel"].shape == (2, n_mels, frames)
    for name in fft:
        assert fft[name].shape == gemm[name].shape and fft[name].dtype == gemm[name].dtype == torch.float32
        assert fft[name].is_contiguous() and gemm[name].is_contiguous() and fft[name].stride() == gemm[name].stride()
    spec = fft["spec"].cpu().double().numpy()
    q = FC.miss(spec, ref["spec"], n_fft)
    print(f"L {L} n_fft {n_fft} spec: max frame err / bound = {q:.3e}")
    assert q <= 1
    for name in fft:
        q = MC.miss(fft[name].cpu().double().numpy(), ref[name], ref[name + "_lim"])
        print(f"L {L} n_fft {n_fft} {name}: max err / budget = {q:.3e}")
        assert q <= 1, name
    assert (ref["rho"] < 0.5).all()
    # the two paths differ by no more than the sum of their budgets
    q = MC.miss(spec, gemm["spec"].cpu().double().numpy(), ref["spec_lim"] + ref_gemm["spec_lim"])
    print(f"L {L} n_fft {n_fft} |fft - gemm|: max / (sum of the budgets) = {q:.3e}")
    assert q <= 1
    # with no `algorithm` argument every function returns the "gemm" bits
    assert torch.equal(gemm["spec"], SP.stft(xd, n_fft, hop, algorithm="gemm"))
    assert torch.equal(gemm["mel"], mel_spectrogram(xd, sr, n_fft, hop, n_mels, algorithm="gemm"))
    assert torch.equal(gemm["logmel"], log_mel(xd, sr, n_fft, hop, n_mels, algorithm="gemm"))
    # leading dimensions, float64 input and the default arguments (the paper's) are the same computation
    if params is MC.PAPER:
        assert torch.equal(log_mel(xd.double().reshape(2, 1, L), algorithm="fft"), fft["logmel"].reshape(2, 1, n_mels, frames))
        assert torch.equal(mel_spectrogram(xd, log_eps=MC.EPS, algorithm="fft"), fft["logmel"])


def test_stft_on_the_fft_without_centring_and_with_a_short_window():
    from speech_decoding_amd import signal_prep as SP
    n_fft, hop, wl = 128, 50, 100
    x = MC.audio(1000)
    xd = torch.from_numpy(x).float().to(DEV)
    w, _ = FC.product_tables(n_fft, wl, False)
    frames = 1 + (1000 - n_fft) // hop
    got = SP.stft(xd, n_fft, hop, win_length=wl, normalized=False, center=False, algorithm="fft")
    assert got.shape == (2, frames, n_fft // 2 + 1, 2)
    assert FC.miss(got.cpu().double().numpy(), FC.restate(x, w, hop, frames, n_fft), n_fft) <= 1


def test_a_second_call_with_the_same_setting_uploads_nothing(monkeypatch):
    from speech_decoding_amd import ops
    from speech_decoding_amd import signal_prep as SP
    xd = torch.from_numpy(MC.audio(1000)).float().to(DEV)
    first = SP.stft(xd, 256, 64, algorithm="fft")
    uploads = []
    inner = ops.UPLOADER._upload
    monkeypatch.setattr(ops.UPLOADER, "_upload", lambda array, device: uploads.append(array.shape) or inner(array, device))
    assert torch.equal(SP.stft(xd, 256, 64, algorithm="fft"), first) and uploads == []
    SP.stft(xd, 1024, 64, algorithm="fft")
    assert sorted(uploads) == [(512, 2), (1024,)]


def test_mel_embeddings_takes_the_algorithm_from_preprocs():
    from speech_decoding_amd import log_mel, mel_embeddings
    from speech_decoding_amd import signal_prep as SP
    from speech_decoding_amd.wav2vec2 import resample_fft
    pre = {"lowpass_filter_width": 128, "last4layers": False, "brain_resample_rate": 120}
    wave = torch.from_numpy(MC.audio(22050, rows=1)).float().to(DEV)
    wave16 = SP.resample_audio(wave, 44100, 16000, lowpass_filter_width=128)
    got = mel_embeddings(wave, 44100, dict(pre, mel={"algorithm": "fft"}))
    ref = resample_fft(log_mel(wave16, algorithm="fft")[0], up=120 / 125)
    assert got.dtype == torch.float64 and got.shape == ref.shape and torch.equal(got, ref)
    small = mel_embeddings(wave, 44100, dict(pre, mel={"n_mels": 10, "n_fft": 64, "hop_length": 16, "eps": 1e-3, "algorithm": "fft"}))
    assert torch.equal(small, resample_fft(log_mel(wave16, n_fft=64, hop_length=16, n_mels=10, eps=1e-3, algorithm="fft")[0], up=120 / 1000))
    # without the key, and with "gemm", the bits of before
    plain = mel_embeddings(wave, 44100, pre)
    assert torch.equal(plain, mel_embeddings(wave, 44100, dict(pre, mel={"algorithm": "gemm"})))
    assert torch.equal(plain, resample_fft(log_mel(wave16)[0], up=120 / 125))
    assert not torch.equal(plain, got)                               # the two paths round differently: "fft" did run the FFT
    from speech_decoding_amd import SdaError
    with pytest.raises(SdaError, match="nope"):
        mel_embeddings(wave, 44100, dict(pre, mel={"algorithm": "nope"}))
