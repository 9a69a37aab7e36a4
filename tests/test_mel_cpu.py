"""CPU checks of the log-mel path (speech_decoding_amd/signal_prep.py: stft_matrix, mel_filterbank, stft, mel_spectrogram on
csrc/window_gemm.hip and csrc/mel_power.hip): the product's matrices against scalar-by-scalar restatements of torch.stft's and
torchaudio's documented rules, the STFT restatement against np.fft.rfft, that the shared cases and bounds of tests/mel_cases.py
catch every planted bug by a factor of 10, and the refusals of the C entry point and of the Python layer.
No kernel is launched here."""
import math
import os
import re
import warnings

import numpy as np
import pytest
import torch

from speech_decoding_amd.signal_prep import mel_filterbank, stft_matrix      # noqa: F401  (the module tests this feature only)
from tests import mel_cases as MC

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def lib():
    from speech_decoding_amd import lib as L
    if not os.path.exists(L.LIB_PATH):
        import __graft_entry__ as g
        g.build()
    return L


def _fbank(*args):
    from speech_decoding_amd.signal_prep import mel_filterbank
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        return mel_filterbank(*args)


@pytest.mark.parametrize("n_fft,win_length,normalized", [(512, None, True), (64, None, True), (64, 40, True), (16, 7, False), (9, None, True)])
def test_stft_matrix_follows_the_rule(n_fft, win_length, normalized):
    from speech_decoding_amd.signal_prep import stft_matrix
    B = stft_matrix(n_fft, win_length, normalized)
    n_freqs = n_fft // 2 + 1
    assert B.dtype == np.float64 and B.shape == (n_fft, 2 * n_freqs)
    np.testing.assert_allclose(B, MC.stft_matrix(n_fft, win_length, normalized), rtol=0, atol=1e-12)
    # a pure cosine at bin b0: the spectrum there is sum_k w[k] cos^2(2 pi b0 k / n) / c — N^2 (sum w cos^2)^2 in power for
    # amplitude N — and its imaginary part sum_k w[k] cos sin / c
    wl = n_fft if win_length is None else win_length
    w = np.zeros(n_fft)
    w[(n_fft - wl) // 2:(n_fft - wl) // 2 + wl] = MC.hann(wl)
    c = math.sqrt((w * w).sum()) if normalized else 1.0
    b0 = min(3, n_freqs - 1)
    ang = 2 * np.pi * b0 * np.arange(n_fft) / n_fft
    spec = (n_fft * np.cos(ang)) @ B
    power = spec[2 * b0] ** 2 + spec[2 * b0 + 1] ** 2
    closed = n_fft ** 2 * ((w * np.cos(ang) ** 2).sum() ** 2 + (w * np.cos(ang) * np.sin(ang)).sum() ** 2) / c ** 2
    assert abs(power - closed) <= 1e-10 * closed


@pytest.mark.parametrize("n_freqs,n_mels,sr,f_min,f_max", [(257, 120, 16000, 0.0, 8000.0), (33, 10, 16000, 0.0, 8000.0),
                                                           (201, 40, 22050, 20.0, 7600.0), (5, 3, 8000, 0.0, 4000.0)])
def test_mel_filterbank_follows_the_rule(n_freqs, n_mels, sr, f_min, f_max):
    fb = _fbank(n_freqs, f_min, f_max, n_mels, sr)
    ref, f_pts, all_freqs = MC.mel_filterbank(n_freqs, f_min, f_max, n_mels, sr)
    assert fb.dtype == np.float64 and fb.shape == (n_freqs, n_mels)
    np.testing.assert_allclose(fb, ref, rtol=0, atol=1e-12)
    f32 = fb.astype(np.float32)
    assert (f32 >= 0).all() and (f32 <= 1).all()
    # every column is a triangle over (f_pts[j], f_pts[j + 2]) with its apex at f_pts[j + 1]: zero outside, and where the bins
    # are dense against its width its sum is the triangle's area over the bin spacing
    df = all_freqs[1] - all_freqs[0]
    for j in range(n_mels):
        outside = (all_freqs <= f_pts[j]) | (all_freqs >= f_pts[j + 2])
        assert (fb[outside, j] == 0).all() and (fb[~outside, j] > 0).all()
        width = f_pts[j + 2] - f_pts[j]
        if min(f_pts[j + 1] - f_pts[j], f_pts[j + 2] - f_pts[j + 1]) >= 4 * df:
            # sampling a piecewise-linear function: each kink (slope change s per Hz) costs at most s df / 8 of the sum — the two
            # feet 1 / 32 each and the apex 1 / 16 once both flanks span four bins
            assert abs(fb[:, j].sum() - 0.5 * width / df) <= 0.125 + 1e-9


def test_empty_filters_at_the_papers_setting_warn_once():
    from speech_decoding_amd import signal_prep as SP
    SP._warned_empty_filters = False
    with warnings.catch_warnings(record=True) as seen:
        warnings.simplefilter("always")
        fb = SP.mel_filterbank(257, 0.0, 8000.0, 120, 16000)
        SP.mel_filterbank(257, 0.0, 8000.0, 120, 16000)
        SP.mel_filterbank(33, 0.0, 8000.0, 10, 16000)           # every filter holds a bin: nothing to warn about
    assert (fb.max(axis=0) == 0).any()
    assert len([w for w in seen if "mel filters" in str(w.message)]) == 1


@pytest.mark.parametrize("params", [MC.PAPER, MC.SMALL], ids=["paper", "small"])
@pytest.mark.parametrize("L", MC.E2E_LENGTHS)
def test_stft_restatement_equals_rfft_of_the_windowed_frames(params, L):
    n_fft, hop = params["n_fft"], params["hop_length"]
    x = MC.audio(L)
    spec = MC.stft(x, MC.stft_matrix(n_fft), n_fft, hop)
    frames = 1 + L // hop
    assert spec.shape == (2, frames, n_fft // 2 + 1, 2)
    xp = np.pad(x, ((0, 0), (n_fft // 2, n_fft // 2)), mode="reflect")
    w = MC.hann(n_fft)
    for m in range(frames):
        fr = xp[:, m * hop:m * hop + n_fft] * w
        ref = np.fft.rfft(fr, axis=-1) / math.sqrt((w * w).sum())
        tol = 1e-10 * np.linalg.norm(fr, axis=-1, keepdims=True)
        assert (np.abs(spec[:, m, :, 0] - ref.real) <= tol).all() and (np.abs(spec[:, m, :, 1] - ref.imag) <= tol).all()


# ---------------------------------------------------------------------------------------------------------------
# the cases and bounds of the GPU tests have teeth
# ---------------------------------------------------------------------------------------------------------------
def test_exact_case_sums_stay_exact():
    for n_freqs, n_mels, _ in MC.KERNEL_SHAPES:
        assert n_freqs * (8 * 8 + 8 * 8) * 4 < 2 ** 24
        spec, fb = MC.int_operands(n_freqs, n_mels, 3, 37)
        assert np.abs(spec).max() <= 8 and fb.min() >= 0 and fb.max() <= 4
        assert MC.mel_power(spec, fb).max() < 2 ** 24


@pytest.mark.parametrize("mutant", [m for m in MC.KERNEL_MUTANTS if m != "log_without_eps"])
def test_kernel_level_bugs_fail_the_exact_and_the_bounded_cases(mutant):
    caught = []
    for n_freqs, n_mels, _ in MC.KERNEL_SHAPES:
        for rows, frames in MC.kernel_runs():
            spec, fb = MC.int_operands(n_freqs, n_mels, rows, frames)
            assert np.array_equal(MC.mel_power(spec, fb), MC.mel_power(spec, fb, mutant=None))
            if not np.array_equal(MC.mel_power(spec, fb, mutant=mutant), MC.mel_power(spec, fb)):
                caught.append((n_freqs, n_mels, rows, frames))
    assert caught, f"no exact case sees the bug {mutant}"
    assert any(c[:2] == (257, 120) for c in caught)
    # the real-operand bound of the GPU test, on its operands: missed by 10 x or more on every shape that can show the bug
    worst = {}
    for n_freqs, n_mels, _ in MC.KERNEL_SHAPES:
        spec, fb = MC.real_operands(n_freqs, n_mels, 3, 37)
        ref = MC.mel_power(spec, fb)
        worst[(n_freqs, n_mels)] = MC.miss(MC.mel_power(spec, fb, mutant=mutant), ref, MC.rel_bound(n_freqs) * ref)
    assert worst[(257, 120)] >= 10 and worst[(33, 33)] >= 10, worst
    if mutant != "not_transposed":                     # a 1 x 1 output has no transpose
        assert min(worst.values()) >= 10, worst


def test_log_without_eps_fails_the_log_cases():
    """the log test's operands are small enough for eps to matter: log(mel) misses the bound by 10 x on every shape, and is
    -inf on the all-zero filter column"""
    for n_freqs, n_mels, _ in MC.KERNEL_SHAPES:
        spec, fb = MC.real_operands(n_freqs, n_mels, 3, 37, scale=2.0 ** -9, zero_column=n_mels > 1)
        ref = MC.mel_power(spec, fb, MC.EPS)
        lim = MC.log_bound(ref, MC.rel_bound(n_freqs))
        assert np.isfinite(ref).all() and np.isfinite(lim).all()
        assert MC.miss(MC.mel_power(spec, fb, MC.EPS, mutant="log_without_eps"), ref, lim) >= 10
        if n_mels > 1:
            assert (ref[:, n_mels // 2, :] == math.log(float(np.float32(MC.EPS)))).all()
    # and the bound itself is tight enough to see one ulp-scale slip of the sum: 10 relative bounds of mel move the log past it
    spec, fb = MC.real_operands(257, 120, 3, 37, scale=2.0 ** -9)
    ref = MC.mel_power(spec, fb, MC.EPS)
    moved = np.log(float(np.float32(MC.EPS)) + MC.mel_power(spec, fb) * (1 + 100 * MC.rel_bound(257)))
    assert MC.miss(moved, ref, MC.log_bound(ref, MC.rel_bound(257))) > 1


@pytest.mark.parametrize("mutant", MC.PATH_MUTANTS + ("imag_dropped", "frame_off_by_one"))
def test_path_level_bugs_fail_the_end_to_end_budget(mutant):
    """the end-to-end cases of the GPU test with its budgets: every planted bug misses by 10 x or more, on every parameter set
    (a dropped last bin is the kernel cases' to see: the mel filterbank's row at f_max, the last triangle's foot, is zero)"""
    for params in (MC.PAPER, MC.SMALL):
        n_fft, hop = params["n_fft"], params["hop_length"]
        B, fb = MC.e2e_matrices(params)
        path = mutant in MC.PATH_MUTANTS
        Bm = MC.e2e_matrices(params, mutant)[0] if path else B
        worst = {"spec": 0.0, "mel": 0.0, "logmel": 0.0}
        for L in MC.E2E_LENGTHS:
            x = MC.audio(L)
            ref = MC.e2e(x, B, fb, n_fft, hop)
            assert (ref["rho"] < 0.5).all()                          # the budget never degenerates
            assert MC.miss(ref["mel"], ref["mel"], ref["mel_lim"]) == 0
            if path:
                got = MC.e2e(x, Bm, fb, n_fft, hop, mutant=mutant)
            else:
                got = {"spec": ref["spec"], "mel": MC.mel_power(ref["spec"], fb, mutant=mutant),
                       "logmel": MC.mel_power(ref["spec"], fb, MC.EPS, mutant=mutant)}
            for k in worst:
                worst[k] = max(worst[k], MC.miss(got[k], ref[k], ref[k + "_lim"]))
        if path:
            assert worst["spec"] >= 10, (params, worst)
        assert worst["mel"] >= 10 and worst["logmel"] >= 10, (params, worst)


# ---------------------------------------------------------------------------------------------------------------
# refusals and the boundary
# ---------------------------------------------------------------------------------------------------------------
def test_c_entry_point_refuses_bad_arguments_without_launch(lib):
    L = lib.load()
    p = 4096                                           # a non-null address that is never dereferenced: every call is refused
    ok = dict(spec=p, srs=4 * 10, sp=10, rows=2, frames=4, n_freqs=5, fb=p, n_mels=3, out=p, ors=3 * 4, op=4)

    def call(**kw):
        a = dict(ok, **kw)
        return L.sda_mel_power_f32(a["spec"], a["srs"], a["sp"], a["rows"], a["frames"], a["n_freqs"], a["fb"], a["n_mels"], 1e-5,
                                   a["out"], a["ors"], a["op"], None)
    for name in ("spec", "fb", "out"):
        assert call(**{name: None}) == -1
        assert b"null" in L.sda_last_error()
    for name in ("rows", "frames", "n_freqs", "n_mels"):
        for bad in (0, -1):
            assert call(**{name: bad}) == -1
            assert b"positive" in L.sda_last_error()
    assert call(sp=9) == -1 and b"spec_pitch" in L.sda_last_error()
    assert call(op=3) == -1 and b"out_pitch" in L.sda_last_error()
    assert call(srs=3 * 10 + 10 - 1) == -1 and b"spec_row_stride" in L.sda_last_error()
    assert call(ors=2 * 4 + 4 - 1) == -1 and b"out_row_stride" in L.sda_last_error()
    assert call(frames=2 ** 62, op=2 ** 62, sp=2 ** 40) == -1 and b"indexing" in L.sda_last_error()


def test_python_layer_refuses_host_tensors_and_odd_shapes():
    from speech_decoding_amd import SdaError, log_mel, mel_embeddings, mel_spectrogram, ops
    from speech_decoding_amd import signal_prep as SP
    x = torch.zeros(2, 1000)
    for fn in (SP.stft, mel_spectrogram, log_mel):
        with pytest.raises(SdaError, match="device"):
            fn(x)
    with pytest.raises(SdaError, match="device"):
        mel_embeddings(torch.zeros(1, 1000), 44100, {"lowpass_filter_width": 128, "brain_resample_rate": 120})
    with pytest.raises(SdaError, match="device"):
        ops.mel_power(torch.zeros(1, 4, 5, 2), torch.zeros(5, 3))
    if torch.cuda.is_available():
        d = torch.zeros(1, 4, 5, 2, device="cuda:0")
        for bad in (torch.zeros(4, 3, device="cuda:0"), torch.zeros(5, device="cuda:0"), torch.zeros(5, 3, 1, device="cuda:0")):
            with pytest.raises(SdaError, match="fb"):
                ops.mel_power(d, bad)
    with pytest.raises(ValueError):
        SP.stft_matrix(16, 17)
    with pytest.raises(ValueError):
        SP.mel_filterbank(5, 100.0, 50.0, 3, 8000)


def test_header_declares_and_lib_binds_the_entry_point(lib):
    header = open(os.path.join(ROOT, "include", "sd_amd.h")).read()
    code = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    m = re.search(r"int\s+sda_mel_power_f32\s*\(([^)]*)\)", code)
    assert m, "sda_mel_power_f32 is not declared in include/sd_amd.h"
    assert len(m.group(1).split(",")) == len(lib.SIGNATURES["sda_mel_power_f32"][1]) == 13
    assert "ABI 4, addition" in header[header.index("Log-mel"):header.index("int sda_mel_power_f32")]
    assert int(re.search(r"#define\s+SDA_ABI_VERSION\s+(\d+)", header).group(1)) == lib.ABI_VERSION == 4
    L = lib.load()
    assert L.sda_abi_version() == 4 and L.sda_mel_power_f32.restype is not None
    src = open(os.path.join(ROOT, "speech_decoding_amd", "csrc", "Makefile")).read()
    assert "mel_power.hip" in src
    # ops.mel_power is the product's only caller of the entry point
    callers = []
    for dirpath, _, files in os.walk(os.path.join(ROOT, "speech_decoding_amd")):
        for f in files:
            if f.endswith(".py") and f != "lib.py" and "sda_mel_power_f32(" in open(os.path.join(dirpath, f)).read():
                callers.append(f)
    assert callers == ["ops.py"]
