"""CPU checks of the FFT path of the STFT (speech_decoding_amd/signal_prep.py: fft_twiddles, stft_window, stft(algorithm="fft") on
csrc/stft_fft.hip): the tables' rules, that both paths define one transform, that the restatement of tests/fft_cases.py is the
DFT, that the kernel's factorisation (emulated in numpy fp32) stays inside the derived bound on every shared case while every
planted bug misses it by a factor of 10, and the refusals of the C entry point and of the Python layer.
No kernel is launched here."""
import math
import os
import re

import numpy as np
import pytest
import torch

from speech_decoding_amd.signal_prep import fft_twiddles, stft_window      # noqa: F401  (the module tests this feature only)
from tests import fft_cases as FC

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ALL_SIZES = (32, 64, 128, 256, 512, 1024, 2048)


@pytest.fixture(scope="module")
def lib():
    from speech_decoding_amd import lib as L
    if not os.path.exists(L.LIB_PATH):
        import __graft_entry__ as g
        g.build()
    return L


@pytest.mark.parametrize("n_fft", ALL_SIZES + (8, 48))
def test_fft_twiddles_follow_the_rule(n_fft):
    tw = fft_twiddles(n_fft)
    assert tw.dtype == np.float64 and tw.shape == (n_fft // 2, 2) and not tw.flags.writeable
    assert fft_twiddles(n_fft) is tw                                  # cached
    ref = np.array([[math.cos(2 * math.pi * j / n_fft), -math.sin(2 * math.pi * j / n_fft)] for j in range(n_fft // 2)])
    np.testing.assert_allclose(tw, ref, rtol=0, atol=1e-15)
    assert tuple(tw[0]) == (1.0, 0.0) and not np.signbit(tw[0]).any()
    if n_fft % 4 == 0:
        assert tuple(tw[n_fft // 4]) == (0.0, -1.0) and not np.signbit(tw[n_fft // 4, 0])
    if n_fft % 8 == 0:
        assert tw[n_fft // 8, 0] == -tw[n_fft // 8, 1] == math.sqrt(0.5)
        assert -tw[3 * n_fft // 8, 0] == -tw[3 * n_fft // 8, 1] == math.sqrt(0.5)
    # the symmetry the integer reduction gives exactly: exp(-i (pi / 2 - a)) = -i conj(exp(-i a))
    if n_fft % 4 == 0:
        j = np.arange(1, n_fft // 4)
        assert (tw[n_fft // 4 - j, 0] == -tw[j, 1]).all() and (tw[n_fft // 4 - j, 1] == -tw[j, 0]).all()
    # the fp32 table the kernel gets is the correctly rounded one (mu = u in the bound)
    assert (np.abs(tw.astype(np.float32).astype(np.float64) - ref) <= FC.U * np.abs(ref) + 1e-15).all()
    with pytest.raises(ValueError):
        fft_twiddles(7)


@pytest.mark.parametrize("n_fft,win_length,normalized", [(512, None, True), (64, None, True), (64, 40, True), (32, 7, False), (2048, None, True)])
def test_stft_window_follows_the_rule_and_both_paths_define_one_transform(n_fft, win_length, normalized):
    from speech_decoding_amd.signal_prep import stft_matrix
    from tests import mel_cases as MC
    w = stft_window(n_fft, win_length, normalized)
    assert w.dtype == np.float64 and w.shape == (n_fft,) and not w.flags.writeable
    wl = n_fft if win_length is None else win_length
    ref = np.zeros(n_fft)
    ref[(n_fft - wl) // 2:(n_fft - wl) // 2 + wl] = MC.hann(wl)
    if normalized:
        ref = ref / math.sqrt(sum(v * v for v in ref))
    np.testing.assert_allclose(w, ref, rtol=0, atol=1e-15)
    # stft_matrix = window[:, None] x the DFT the twiddle table spells out (entry (b k) mod n_fft; the second half negated)
    tw = fft_twiddles(n_fft)
    full = np.concatenate([tw, -tw])
    k = np.arange(n_fft)[:, None]
    b = np.arange(n_fft // 2 + 1)[None, :]
    D = full[(b * k) % n_fft]                                        # (n_fft, n_freqs, 2)
    B = stft_matrix(n_fft, win_length, normalized)
    np.testing.assert_allclose(B.reshape(n_fft, -1, 2), w[:, None, None] * D, rtol=0, atol=1e-12)
    with pytest.raises(ValueError):
        stft_window(16, 17)


@pytest.mark.parametrize("n_fft", (32, 64, 512))
def test_the_restatement_is_the_direct_sum(n_fft):
    w, _ = FC.product_tables(n_fft)
    for hop in FC.hops(n_fft):
        x = FC.real_operands(n_fft, hop, 3, 5)
        a, b = FC.direct(x, w, hop, 5, n_fft), FC.restate(x, w, hop, 5, n_fft)
        assert a.shape == b.shape == (3, 5, n_fft // 2 + 1, 2)
        assert np.abs(a - b).max() <= 1e-12 * FC.frame_norms(b).max()


def test_the_bound_is_the_derived_one():
    """(k eta) with k = log2(n_fft / 2) + 3, the window's u, the one-sided sqrt 2: the figures of the module docstring"""
    for n_fft, lo, hi in ((32, 66, 68), (512, 104, 106), (2048, 123, 125)):
        assert lo * FC.U < FC.rel_bound(n_fft) < hi * FC.U


@pytest.mark.parametrize("n_fft", ALL_SIZES)
def test_the_kernels_factorisation_stays_inside_the_bound_on_every_case(n_fft):
    w, tw = FC.product_tables(n_fft)
    worst = 0.0
    runs = FC.kernel_runs(n_fft) if n_fft in FC.N_FFTS else [(n_fft // 4, 3, 37)]
    for hop, rows, frames in runs:
        for kind in range(4 if (rows, frames) == (3, 37) else 1):
            x = FC.real_operands(n_fft, hop, rows, frames, kind)
            ref = FC.restate(x, w, hop, frames, n_fft)
            got = FC.emulate(x, w, tw, hop, frames, n_fft)
            assert got.shape == ref.shape
            q = FC.miss(got, ref, n_fft)
            worst = max(worst, q)
            assert q <= 1, (hop, rows, frames, kind)
            # bins 0 and n_fft / 2 are real
            assert (got[:, :, 0, 1] == 0).all() and (got[:, :, n_fft // 2, 1] == 0).all()
            # and the elementwise budget holds with it
            assert (np.abs(got - ref) <= FC.elementwise_budget(ref, n_fft)).all()
    print(f"n_fft {n_fft}: emulation's worst err / bound = {worst:.3e} ({worst * FC.rel_bound(n_fft) / FC.U:.2f} u)")
    assert worst > 0                                                 # the emulation does round: it is not the reference again


@pytest.mark.parametrize("mutant", FC.MUTANTS)
def test_every_planted_bug_misses_the_bound_by_ten(mutant):
    """on the shared cases of the GPU test: at every size, some case misses by 10 x or more"""
    for n_fft in FC.N_FFTS:
        w, tw = FC.product_tables(n_fft)
        worst = 0.0
        for hop, rows, frames in FC.kernel_runs(n_fft):
            if rows != 3 or frames != 37:
                continue
            x = FC.real_operands(n_fft, hop, rows, frames)
            ref = FC.restate(x, w, hop, frames, n_fft)
            worst = max(worst, FC.miss(FC.emulate(x, w, tw, hop, frames, n_fft, mutant), ref, n_fft))
        assert worst >= 10, (mutant, n_fft, worst)


@pytest.mark.parametrize("alternating", (False, True))
def test_the_exact_cases_are_exact_in_the_emulation_and_see_addressing_bugs(alternating):
    for n_fft in FC.N_FFTS:
        x, ref = FC.constant_frames(n_fft, 3, 5, alternating)
        ones, tw = np.ones(n_fft), FC.product_tables(n_fft)[1]
        assert (FC.restate(x.astype(np.float64), ones, n_fft, 5, n_fft).round() == ref).all()
        got = FC.emulate(x.astype(np.float64), ones, tw, n_fft, 5, n_fft)
        assert (got == ref).all()
        assert np.abs(ref).max() < 2 ** 24
        if not alternating:
            for mutant in ("frame_start_plus", "frame_start_minus"):
                assert not (FC.emulate(x.astype(np.float64), ones, tw, n_fft, 5, n_fft, mutant) == ref).all()


# ---------------------------------------------------------------------------------------------------------------
# refusals and the boundary
# ---------------------------------------------------------------------------------------------------------------
def test_c_entry_point_refuses_bad_arguments_without_launch(lib):
    L = lib.load()
    p = 4096                                           # a non-null address that is never dereferenced: every call is refused
    ok = dict(x=p, xrs=3 * 16 + 64, rows=2, frames=4, hop=16, n_fft=64, window=p, twiddle=p, out=p, ors=4 * 66, op=66)

    def call(**kw):
        a = dict(ok, **kw)
        return L.sda_stft_fft_f32(a["x"], a["xrs"], a["rows"], a["frames"], a["hop"], a["n_fft"], a["window"], a["twiddle"], a["out"],
                                  a["ors"], a["op"], None)
    for name in ("x", "window", "twiddle", "out"):
        assert call(**{name: None}) == -1
        assert b"null" in L.sda_last_error()
    for name in ("rows", "frames", "hop", "n_fft"):
        for bad in (0, -1):
            assert call(**{name: bad}) == -1
            assert b"positive" in L.sda_last_error()
    for bad in (16, 48, 100, 4096, 2047):
        assert call(n_fft=bad, xrs=10 ** 6, ors=10 ** 6, op=10 ** 4) == -1
        assert b"power of two" in L.sda_last_error()
    assert call(op=65) == -1 and b"out_pitch" in L.sda_last_error()
    assert call(ors=3 * 66 + 66 - 1) == -1 and b"out_row_stride" in L.sda_last_error()
    assert call(xrs=3 * 16 + 64 - 1) == -1 and b"x_row_stride" in L.sda_last_error()
    assert call(hop=100, xrs=3 * 100 + 64 - 1) == -1 and b"x_row_stride" in L.sda_last_error()
    assert call(frames=2 ** 62, op=2 ** 40) == -1 and b"indexing" in L.sda_last_error()


def test_python_layer_refuses_unknown_algorithms_unsupported_sizes_and_host_tensors():
    from speech_decoding_amd import SdaError, log_mel, mel_embeddings, mel_spectrogram, ops
    from speech_decoding_amd import signal_prep as SP
    # the pure argument check
    assert SP.check_stft_algorithm("gemm", 48) == "gemm" and SP.check_stft_algorithm("fft", 512) == "fft"
    with pytest.raises(SdaError, match="nope"):
        SP.check_stft_algorithm("nope", 512)
    for n_fft in (48, 16, 4096):
        with pytest.raises(SdaError, match="no fallback"):
            SP.check_stft_algorithm("fft", n_fft)
    assert set(ops.STFT_FFT_SIZES) == set(ALL_SIZES)
    # ... comes before the device check in every public function
    x = torch.zeros(2, 5000)
    for fn in (SP.stft, mel_spectrogram, log_mel):
        with pytest.raises(SdaError, match="nope"):
            fn(x, algorithm="nope")
        for n_fft in (48, 16, 4096):
            with pytest.raises(SdaError, match="no fallback"):
                fn(x, n_fft=n_fft, algorithm="fft")
        with pytest.raises(SdaError, match="device"):
            fn(x, algorithm="fft")
    with pytest.raises(SdaError, match="device"):
        mel_embeddings(torch.zeros(1, 1000), 44100, {"lowpass_filter_width": 128, "brain_resample_rate": 120, "mel": {"algorithm": "fft"}})
    with pytest.raises(SdaError, match="device"):
        ops.stft_fft(torch.zeros(1, 64), torch.zeros(64), torch.zeros(32, 2), 1, 16, 64)
    # the keyword is the last one and defaults to the window GEMM
    import inspect
    for fn in (SP.stft, mel_spectrogram, log_mel):
        params = list(inspect.signature(fn).parameters.values())
        assert params[-1].name == "algorithm" and params[-1].default == "gemm"
    for n_fft in ALL_SIZES:
        assert ops.stft_fft_frames_per_workgroup(n_fft) == min(4096 // n_fft, 32)


def test_header_declares_and_lib_binds_the_entry_point(lib):
    header = open(os.path.join(ROOT, "include", "sd_amd.h")).read()
    code = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    m = re.search(r"int\s+sda_stft_fft_f32\s*\(([^)]*)\)", code)
    assert m, "sda_stft_fft_f32 is not declared in include/sd_amd.h"
    assert len(m.group(1).split(",")) == len(lib.SIGNATURES["sda_stft_fft_f32"][1]) == 12
    assert "ABI 4, addition" in header[header.index("The STFT as a power-of-two FFT"):header.index("int sda_stft_fft_f32")]
    assert int(re.search(r"#define\s+SDA_ABI_VERSION\s+(\d+)", header).group(1)) == lib.ABI_VERSION == 4
    L = lib.load()
    assert L.sda_abi_version() == 4 and L.sda_stft_fft_f32.restype is not None
    src = open(os.path.join(ROOT, "speech_decoding_amd", "csrc", "Makefile")).read()
    assert "stft_fft.hip" in src
    # the frames a workgroup owns: ops mirrors the kernel's two constants
    hip = open(os.path.join(ROOT, "speech_decoding_amd", "csrc", "stft_fft.hip")).read()
    samples = int(re.search(r"constexpr int SF_SAMPLES = (\d+);", hip).group(1))
    most = int(re.search(r"constexpr int SF_MAX_FRAMES = (\d+);", hip).group(1))
    from speech_decoding_amd import ops
    for n_fft in ALL_SIZES:
        assert ops.stft_fft_frames_per_workgroup(n_fft) == min(samples // n_fft, most)
    # ops.stft_fft is the product's only caller of the entry point
    callers = []
    for dirpath, _, files in os.walk(os.path.join(ROOT, "speech_decoding_amd")):
        for f in files:
            if f.endswith(".py") and f != "lib.py" and "sda_stft_fft_f32(" in open(os.path.join(dirpath, f)).read():
                callers.append(f)
    assert callers == ["ops.py"]
