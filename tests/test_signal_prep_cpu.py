"""CPU checks of the signal-conditioning path (speech_decoding_amd/signal_prep.py): the window-GEMM formulation of the FIR filter
and of the sinc resampler against np.convolve / the direct formula, mne's documented band-pass design rule, that the shared
cases of tests/signal_cases.py catch every planted bug, and the refusals of the C entry point and of the Python layer.
No kernel is launched here."""
import ctypes
import os

import numpy as np
import pytest
import torch

from tests import signal_cases as SC


@pytest.fixture(scope="module")
def lib():
    from speech_decoding_amd import lib as L
    if not os.path.exists(L.LIB_PATH):
        import __graft_entry__ as g
        g.build()
    return L


def _fir_operands(R, L, K, seed):
    return SC.ints((R, L), 8, seed), SC.ints((K,), 4, seed + 1)


@pytest.mark.parametrize("R,L,K,G", SC.FIR_EXACT)
def test_fir_through_the_window_gemm_equals_convolve_exactly(R, L, K, G):
    from speech_decoding_amd.signal_prep import window_matrix
    x, h = _fir_operands(R, L, K, 10 * K + G)
    ref = SC.fir_same(x, h)
    assert ref.shape == (R, L) and np.abs(ref).max() > 0
    assert float((np.abs(SC.odd_pad(x, (K - 1) // 2)).max() * np.abs(h).sum())) < 2 ** 24
    assert np.array_equal(SC.fir_through_window_gemm(x, h, G, matrix=window_matrix), ref)
    assert np.array_equal(SC.fir_through_window_gemm(x, h, G), ref)                       # the element-by-element grouping
    assert np.array_equal(SC.fir_through_window_gemm(x, h, 1, matrix=window_matrix), ref)  # exactly independent of G
    assert np.array_equal(window_matrix(h[::-1][None, :], 1, G), SC.toeplitz_blocks(h[::-1][None, :], 1, G))


def test_window_matrix_shape_and_group_rule():
    from speech_decoding_amd.signal_prep import window_group, window_matrix
    bank = SC.ints((3, 5), 4, 0)
    Bm = window_matrix(bank, 2, 4)
    assert Bm.shape == (5 + 3 * 2, 4 * 3)
    assert np.array_equal(Bm, SC.toeplitz_blocks(bank, 2, 4))
    assert window_group(1, 1, 3301) == 64 and window_group(1, 1, 199) == 64      # FIR: one full column tile
    assert window_group(160, 441, 1155) == 1 and window_group(441, 160, 174) == 1 and window_group(320, 441, 487) == 1
    assert 1 <= window_group(1, 3, 41) <= 64
    with pytest.raises(ValueError):
        window_matrix(bank, 0, 1)


@pytest.mark.parametrize("rates,shape", SC.RESAMPLE)
def test_resampler_bank_and_grouping(rates, shape):
    from speech_decoding_amd.signal_prep import sinc_resample_bank, window_group, window_matrix
    orig_f, new_f, lpw = rates
    bank, width, orig, new = sinc_resample_bank(orig_f, new_f, lowpass_filter_width=lpw)
    rbank, rwidth, rorig, rnew = SC.sinc_bank(orig_f, new_f, lpw)
    assert bank.shape == rbank.shape == shape and (width, orig, new) == (rwidth, rorig, rnew)
    assert bank.dtype == np.float64
    np.testing.assert_allclose(bank, rbank, rtol=0, atol=1e-15)
    Lx = 3 * orig + 17
    x = np.random.RandomState(1).randn(2, Lx)
    ref = SC.resample(x, rbank, width, orig, new)
    assert ref.shape == (2, -(-new * Lx // orig))
    xp = np.concatenate([np.zeros((2, width)), x, np.zeros((2, width + orig))], axis=1)
    frames = Lx // orig + 1
    for G in (1, 2, max(window_group(new, orig, bank.shape[1]), 3)):
        Bm = window_matrix(bank, orig, G)
        assert Bm.shape == (bank.shape[1] + (G - 1) * orig, G * new)
        groups = -(-frames // G)
        need = (groups - 1) * G * orig + Bm.shape[0]
        xz = np.concatenate([xp, np.zeros((2, max(need - xp.shape[1], 0)))], axis=1)
        got = SC.emulate(xz, Bm, G * orig, groups)[:, :ref.shape[1]]
        np.testing.assert_allclose(got, ref, rtol=0, atol=1e-12)


@pytest.mark.parametrize("spec,ntaps", SC.BANDPASS)
def test_bandpass_taps_follow_the_design_rule(spec, ntaps):
    from speech_decoding_amd.signal_prep import bandpass_taps
    sfreq, lo, hi = spec
    h = bandpass_taps(sfreq, lo, hi)
    assert h.dtype == np.float64 and h.shape == (ntaps,)
    assert np.array_equal(h, h[::-1])
    assert abs(h.sum()) <= 1e-12
    l_trans = min(max(0.25 * lo, 2.0), lo)
    h_trans = min(max(0.25 * hi, 2.0), sfreq / 2.0 - hi)
    t = np.arange(ntaps) - (ntaps - 1) / 2

    def gain(f):
        return np.abs(np.exp(-2j * np.pi * np.outer(np.atleast_1d(f), t) / sfreq) @ h)
    passband = np.linspace(lo, hi, 200)
    assert np.abs(gain(passband) - 1).max() <= 0.01
    stop = np.concatenate([np.linspace(0, lo - l_trans, 50), np.linspace(hi + h_trans, sfreq / 2, 200)])
    assert gain(stop).max() <= 0.01
    assert np.abs(gain([lo - l_trans / 2, hi + h_trans / 2]) - 0.5).max() <= 0.01


def test_bandpass_taps_equal_scipy_firwin():
    """the two low-passes are scipy.signal.firwin's (the design function mne calls)"""
    sig = pytest.importorskip("scipy.signal")
    from speech_decoding_amd.signal_prep import bandpass_taps
    h = bandpass_taps(120, 2, 30)
    hp = sig.firwin(199, 1.0, window="hamming", fs=120)
    lp = sig.firwin(53, 33.75, window="hamming", fs=120)          # ceil(3.3 * 120 / 7.5) = 53
    ref = -hp
    ref[73:126] += lp
    np.testing.assert_allclose(h, ref, rtol=0, atol=1e-15)


@pytest.mark.parametrize("mutant", SC.MUTANTS)
def test_every_planted_bug_fails_the_exact_cases(mutant):
    caught = []
    for R, L, K, G in SC.FIR_EXACT:
        x, h = _fir_operands(R, L, K, 10 * K + G)
        assert not np.array_equal(h, h[::-1]) or K == 1
        if not np.array_equal(SC.fir_through_window_gemm(x, h, G, mutant=mutant), SC.fir_same(x, h)):
            caught.append((R, L, K, G))
    assert caught, f"no exact case sees the bug {mutant}"
    # the kernel-level shapes see the kernel-level bugs directly
    if mutant in ("stride_plus", "stride_minus", "dropped_k_tail", "dropped_last_column", "frame_off_by_one"):
        S, K, N = 7, 29, 5
        x, B = SC.ints((3, 36 * S + K), 8, 1), SC.ints((K, N), 4, 2)
        assert not np.array_equal(SC.emulate(x, B, S, 37, mutant), SC.window_gemm(x, B, S, 37))
    assert np.array_equal(SC.emulate(SC.ints((3, 36 * 7 + 29), 8, 1), SC.ints((29, 5), 4, 2), 7, 37),
                          SC.window_gemm(SC.ints((3, 36 * 7 + 29), 8, 1), SC.ints((29, 5), 4, 2), 7, 37))


def test_kernel_case_sums_stay_exact():
    for S, K, N, _ in SC.KERNEL_SHAPES:
        assert K * 8 * 4 < 2 ** 24


def test_c_entry_point_refuses_bad_arguments_without_launch(lib):
    L = lib.load()
    p = 4096                                           # a non-null address that is never dereferenced: every call is refused
    wg = L.sda_window_gemm_f32
    ok = dict(x=p, xs=100, rows=2, frames=4, S=3, K=10, B=p, N=5, out=p, os=20)

    def call(**kw):
        a = dict(ok, **kw)
        return wg(a["x"], a["xs"], a["rows"], a["frames"], a["S"], a["K"], a["B"], a["N"], a["out"], a["os"], None)
    for name in ("x", "B", "out"):
        assert call(**{name: None}) == -1
        assert b"null" in L.sda_last_error()
    for name in ("rows", "frames", "S", "K", "N"):
        for bad in (0, -1):
            assert call(**{name: bad}) == -1
            assert b"positive" in L.sda_last_error()
    assert call(os=19) == -1 and b"out_row_stride" in L.sda_last_error()
    assert call(xs=3 * 3 + 10 - 1) == -1 and b"x_row_stride" in L.sda_last_error()
    assert call(frames=2 ** 62, os=2 ** 62) == -1 and b"indexing" in L.sda_last_error()


def test_python_layer_refuses_host_tensors_and_even_taps():
    from speech_decoding_amd import SdaError
    from speech_decoding_amd import signal_prep as SP
    x = torch.zeros(2, 50)
    with pytest.raises(SdaError, match="device"):
        SP.fir_filter(x, [1.0, 2.0, 1.0])
    with pytest.raises(SdaError, match="odd"):
        SP.fir_filter(x, [1.0, 1.0])
    with pytest.raises(SdaError, match="device"):
        SP.filter_data(x, 120, 2, 30)
    with pytest.raises(SdaError, match="device"):
        SP.resample_audio(x, 44100, 16000)
    with pytest.raises(SdaError, match="device"):
        SP.window_gemm(x, torch.zeros(3, 2), 1, 1)
    with pytest.raises(SdaError, match="device"):
        SP.brain_preproc(x, 1000, {"brain_filter_low": 1.0, "brain_filter_high": 60, "brain_resample_rate": 120})
    with pytest.raises(SdaError, match="device"):
        SP.speech_embeddings(None, torch.zeros(1, 50), 44100, {"lowpass_filter_width": 128, "last4layers": True})
