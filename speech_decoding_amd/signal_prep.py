"""Signal conditioning on the GPU: from raw recordings and audio to the arrays the datasets are built from.

What the reference does with MNE and torchaudio on CPU workers before anything else can start:

    mne.filter.filter_data(raw, sfreq, l_freq, h_freq)             gwilliams2022.py:253, brennan2018.py:263   -> filter_data
    torchaudio.functional.resample(wave, sr, 16000, lowpass_filter_width=128)
                                                                   gwilliams2022.py:349, brennan2018.py:172   -> resample_audio
    mne.filter.resample(filtered, down=orig / 120)                 gwilliams2022.py:258, brennan2018.py:270   -> wav2vec2.resample_fft

The first two are one computation — a fixed matrix applied to strided windows of each row,

    out[r, m N + j] = sum_{k < K} x[r, m S + k] B[k, j]

— and run on one kernel, `sda_window_gemm_f32` (csrc/window_gemm.hip, exact-fp32 MFMA).  The polyphase resampler is it with
S = reduced input rate, N = reduced output rate, B = bank^T; the FIR filter is the degenerate resampler S = N = 1 with G
consecutive frames grouped into one, which `window_matrix` does for any bank.  `brain_preproc` and `speech_embeddings` compose
the three calls as the reference's dataset classes do.  Device tensors only: there is no CPU path.

The second speech representation of the paper (the log-mel spectrogram of its regression and "Deep Mel" baselines, which the
reference leaves to torchaudio on the host) is the same kernel once more: an STFT frame is the matrix window x DFT applied
to windows hop_length apart (S = hop_length, K = n_fft, N = 2 (n_fft / 2 + 1), `stft_matrix`, `stft`), and one more kernel,
`sda_mel_power_f32` (csrc/mel_power.hip), takes the power, applies the mel filterbank and the log and stores
(features, frames): `mel_spectrogram`, `log_mel`, `mel_embeddings`.  With algorithm="fft" the STFT runs on a power-of-two FFT
kernel instead, `sda_stft_fft_f32` (csrc/stft_fft.hip; `stft_window`, `fft_twiddles`); the default is the window GEMM.

Parity.  Neither mne nor torchaudio can be installed next to this build, so bit-parity with `mne.filter.create_filter` and
with `torchaudio.functional.resample` is UNPINNED: `bandpass_taps` follows mne's documented "firwin" design rule and
`sinc_resample_bank` torchaudio's documented `sinc_interp_hann` kernel, and both are tested against float64 restatements of
those rules, not against the libraries.  The same holds for `stft_matrix` (torch.stft with a periodic Hann window,
`normalized="window"`) and `mel_filterbank` (`torchaudio.functional.melscale_fbanks`, HTK scale, no normalisation).  `fir_filter` takes arbitrary taps, so a user with mne can pass mne's own
(`mne.filter.create_filter(...)`).
"""
from __future__ import annotations

import math
import warnings
from functools import lru_cache
from typing import Optional, Tuple

import numpy as np
import torch

from . import lib as L
from . import ops
from .wav2vec2 import resample_fft

MAX_GROUP = 64          # largest G window_group considers = the kernel's output tile width


def window_group(P: int, S: int, Kw: int) -> int:
    """The number G of consecutive frames `window_matrix` should group for a bank of P phases, stride S and Kw taps.

    The kernel computes 64-column output tiles over the grouped contraction Kw + (G - 1) S, so of the multiply-adds it issues
    the share  G P / (64 ceil(G P / 64)) * Kw / (Kw + (G - 1) S)  is useful: the first factor is the fill of the column
    tiles, the second the taps against the zeros the Toeplitz blocks add.  G = the value in 1 ... 64 with the largest share,
    the smallest such G on ties.  (FIR, P = S = 1: G = 64 once Kw > 63; 44.1 k -> 16 k, P = 160: G = 1.)"""
    best, best_g = -1.0, 1
    for g in range(1, MAX_GROUP + 1):
        share = (g * P) / (64.0 * math.ceil(g * P / 64.0)) * Kw / (Kw + (g - 1) * S)
        if share > best * (1 + 1e-12):
            best, best_g = share, g
    return best_g


def window_matrix(bank: np.ndarray, S: int, G: int) -> np.ndarray:
    """bank (P, Kw): out[m P + p] = sum_k x[m S + k] bank[p, k].  Returns the block-Toeplitz matrix B' of shape
    (Kw + (G - 1) S, G P) that computes G consecutive frames at once:  out[(m' G + g) P + p] = sum_k x[m' G S + k] B'[k, g P + p],
    B'[g S + k, g P + p] = bank[p, k] — the same sums in the same k order with zeros in between, so the result does not depend
    on G beyond rounding (and not at all on exactly representable operands)."""
    bank = np.asarray(bank)
    if bank.ndim != 2 or S < 1 or G < 1:
        raise ValueError("window_matrix: a (P, Kw) bank, S >= 1, G >= 1")
    P, Kw = bank.shape
    out = np.zeros((Kw + (G - 1) * S, G * P), dtype=bank.dtype)
    for g in range(G):
        out[g * S:g * S + Kw, g * P:(g + 1) * P] = bank.T
    return out


def _check_device(x: torch.Tensor, what: str) -> None:
    if not isinstance(x, torch.Tensor) or not x.is_cuda:
        raise L.SdaError(f"{what} needs device tensors (no CPU fallback)")
    if not x.is_floating_point() or x.dim() < 1 or x.shape[-1] < 1:
        raise L.SdaError(f"{what}: a floating-point tensor (..., L) with L >= 1")


def window_gemm(x: torch.Tensor, B: torch.Tensor, frames: int, S: int) -> torch.Tensor:
    """`sda_window_gemm_f32` on a contiguous fp32 (rows, Lx) device tensor and a (K, N) matrix: (rows, frames N).
    Lx >= (frames - 1) S + K is the caller's to provide (the kernel refuses otherwise)."""
    for t in (x, B):
        if not t.is_cuda or t.dtype != torch.float32 or t.dim() != 2 or not t.is_contiguous():
            raise L.SdaError("window_gemm: contiguous fp32 2-D device tensors")
    K, N = B.shape
    out = torch.empty((x.shape[0], frames * N), dtype=torch.float32, device=x.device)
    with torch.cuda.device(x.device):
        L.check(L.load().sda_window_gemm_f32(x.data_ptr(), x.shape[1], x.shape[0], frames, S, K, B.data_ptr(), N, out.data_ptr(),
                                             out.shape[1], torch.cuda.current_stream().cuda_stream), "window_gemm")
    return out


def _apply_bank(xp: torch.Tensor, bank: np.ndarray, S: int, n_frames: int) -> torch.Tensor:
    """xp (rows, >= (n_frames - 1) S + Kw) fp32 on the device -> (rows, n_frames P): the bank over n_frames windows, grouped by
    window_group's rule; the row is zero-extended to what the last (partly unused) group reads."""
    P, Kw = bank.shape
    G = window_group(P, S, Kw)
    Bm = torch.from_numpy(window_matrix(bank, S, G).astype(np.float32)).to(xp.device)
    groups = -(-n_frames // G)
    need = (groups - 1) * G * S + Bm.shape[0]
    if xp.shape[1] < need:
        xp = torch.cat([xp, xp.new_zeros(xp.shape[0], need - xp.shape[1])], dim=1)
    return window_gemm(xp.contiguous(), Bm, groups, G * S)[:, :n_frames * P]


def fir_filter(x: torch.Tensor, taps) -> torch.Tensor:
    """Zero-phase FIR filtering of the last axis, (..., L) -> fp32 (..., L): the "same" part of the convolution of each row with
    `taps` (odd length K, so the delay (K - 1) / 2 is whole) after mne's "reflect_limited" padding — (K - 1) / 2 samples of odd
    extension 2 x[0] - x[i] / 2 x[-1] - x[-1 - i] per side, zero-filled where the row is shorter than that.  What
    `mne.filter.filter_data` does with its FIR ("overlap-add" there; the same sums)."""
    h = np.asarray(taps, dtype=np.float64).reshape(-1)
    K = h.size
    if K % 2 == 0:
        raise L.SdaError(f"fir_filter: {K} taps — only odd lengths have a whole-sample delay (zero phase)")
    _check_device(x, "fir_filter")
    n = x.shape[-1]
    rows = x.reshape(-1, n).float()
    pad = (K - 1) // 2
    p = min(pad, n - 1)
    z = rows.new_zeros(rows.shape[0], pad - p)
    left = 2 * rows[:, :1] - rows[:, 1:p + 1].flip(-1)
    right = 2 * rows[:, -1:] - rows[:, n - 1 - p:n - 1].flip(-1)
    xp = torch.cat([z, left, rows, right, z], dim=1)                 # n + K - 1
    y = _apply_bank(xp, h[::-1][None, :].copy(), 1, n)
    return y.contiguous().reshape(x.shape)


@lru_cache(maxsize=16)
def _bandpass_taps(sfreq: float, l_freq: float, h_freq: float) -> np.ndarray:
    if not (0 < l_freq < h_freq < sfreq / 2):
        raise ValueError("bandpass_taps: 0 < l_freq < h_freq < sfreq / 2")
    l_trans = min(max(0.25 * l_freq, 2.0), l_freq)
    h_trans = min(max(0.25 * h_freq, 2.0), sfreq / 2.0 - h_freq)

    def odd_len(trans):
        n = int(math.ceil(3.3 * sfreq / trans))
        return n + (n % 2 == 0)

    def lowpass(cut, n):
        """scipy.signal.firwin(n, cut, window="hamming", fs=sfreq): windowed sinc, unit gain at DC"""
        t = np.arange(n, dtype=np.float64) - (n - 1) / 2
        h = 2 * cut / sfreq * np.sinc(2 * cut / sfreq * t) * np.hamming(n)
        return h / h.sum()

    n_tot = odd_len(min(l_trans, h_trans))
    h = np.zeros(n_tot, dtype=np.float64)
    for sign, cut, trans in ((1.0, h_freq + h_trans / 2, h_trans), (-1.0, l_freq - l_trans / 2, l_trans)):
        n = odd_len(trans)
        off = (n_tot - n) // 2
        h[off:off + n] += sign * lowpass(cut, n)
    h.setflags(write=False)
    return h


def bandpass_taps(sfreq: float, l_freq: float, h_freq: float) -> np.ndarray:
    """The band-pass `mne.filter.filter_data(..., l_freq, h_freq)` designs by default (method "fir", fir_design "firwin", Hamming
    window, "auto" lengths), by mne's documented rule: transition widths l_trans = min(max(0.25 l, 2), l) and
    h_trans = min(max(0.25 h, 2), sfreq / 2 - h); 3.3 sfreq / trans taps per edge, made odd; the filter is the centred difference
    of the two Hamming-windowed-sinc low-passes cut at the transition midpoints (h + h_trans / 2, l - l_trans / 2), each of its
    own length.  float64, odd length, symmetric.  (1000, 1, 60) -> 3301 taps.  Parity with mne's own array: unpinned (module
    docstring)."""
    return _bandpass_taps(float(sfreq), float(l_freq), float(h_freq))


def filter_data(x: torch.Tensor, sfreq: float, l_freq: float, h_freq: float) -> torch.Tensor:
    """`mne.filter.filter_data(x, sfreq, l_freq, h_freq)` with both edges given: bandpass_taps + fir_filter."""
    return fir_filter(x, bandpass_taps(sfreq, l_freq, h_freq))


@lru_cache(maxsize=16)
def _sinc_bank(orig: int, new: int, lpw: int, rolloff: float):
    base = min(orig, new) * rolloff
    width = int(math.ceil(lpw * orig / base))
    i = np.arange(-width, width + orig, dtype=np.float64)[None, :] / orig
    ph = np.arange(0, -new, -1, dtype=np.float64)[:, None] / new
    t = np.clip((ph + i) * base, -lpw, lpw)
    bank = np.sinc(t) * np.cos(t * math.pi / lpw / 2) ** 2 * (base / orig)
    bank.setflags(write=False)
    return bank, width


def sinc_resample_bank(orig_freq: int, new_freq: int, lowpass_filter_width: int = 6, rolloff: float = 0.99) -> Tuple[np.ndarray, int, int, int]:
    """torchaudio's `sinc_interp_hann` resampling kernel in float64: (bank (new', Kw), width, orig', new') with the rates divided
    by their gcd, base = min(orig', new') rolloff, width = ceil(lpw orig' / base), Kw = 2 width + orig', and
    bank[p, i] = sinc(pi t) cos^2(pi t / (2 lpw)) base / orig' at t = (-p / new' + (i - width) / orig') base clamped to +-lpw."""
    orig_freq, new_freq = int(orig_freq), int(new_freq)
    if orig_freq < 1 or new_freq < 1 or lowpass_filter_width < 1:
        raise ValueError("sinc_resample_bank: positive integer rates and filter width")
    g = math.gcd(orig_freq, new_freq)
    orig, new = orig_freq // g, new_freq // g
    bank, width = _sinc_bank(orig, new, int(lowpass_filter_width), float(rolloff))
    return bank, width, orig, new


def resample_audio(wave: torch.Tensor, orig_freq: int, new_freq: int, lowpass_filter_width: int = 6, rolloff: float = 0.99) -> torch.Tensor:
    """`torchaudio.functional.resample(wave, orig_freq, new_freq, lowpass_filter_width, rolloff)` (sinc_interp_hann), (..., L) ->
    fp32 (..., ceil(new' L / orig')): the row zero-padded by (width, width + orig'), the bank applied at stride orig'.  Equal
    rates return the input.  Parity with torchaudio's own output: unpinned (module docstring)."""
    _check_device(wave, "resample_audio")
    if int(orig_freq) == int(new_freq):
        return wave
    bank, width, orig, new = sinc_resample_bank(orig_freq, new_freq, lowpass_filter_width, rolloff)
    n = wave.shape[-1]
    rows = wave.reshape(-1, n).float()
    target = -(-new * n // orig)
    n_frames = n // orig + 1
    xp = torch.cat([rows.new_zeros(rows.shape[0], width), rows, rows.new_zeros(rows.shape[0], width + orig)], dim=1)
    y = _apply_bank(xp, bank, orig, n_frames)[:, :target]
    return y.contiguous().reshape(wave.shape[:-1] + (target,))


def brain_preproc(raw: torch.Tensor, orig_rate: float, preprocs) -> torch.Tensor:
    """Raw recording (C, L) at orig_rate -> fp32 (C, round(L brain_resample_rate / orig_rate)): the band-pass
    preprocs["brain_filter_low"] ... ["brain_filter_high"], then FFT resampling to preprocs["brain_resample_rate"]
    (gwilliams2022.py:253-260, brennan2018.py:263-272)."""
    filtered = filter_data(raw, orig_rate, preprocs["brain_filter_low"], preprocs["brain_filter_high"])
    return resample_fft(filtered, up=preprocs["brain_resample_rate"] / orig_rate).float()


def speech_embeddings(embedder, wave: torch.Tensor, sample_rate: int, preprocs, audio_resample_rate: int = 16000) -> torch.Tensor:
    """One audio file (1, L) at sample_rate -> float64 (features, frames at brain_resample_rate), gwilliams2022.py:346-373:
    resample to 16 kHz (preprocs["lowpass_filter_width"]), embed with `embedder` (a Wav2Vec2Embedder: the mean of the last four
    hidden states, or the feature encoder's output when preprocs["last4layers"] is false), FFT-resample from the embedder's
    frame rate to preprocs["brain_resample_rate"]."""
    _check_device(wave, "speech_embeddings")
    if wave.dim() != 2 or wave.shape[0] != 1:
        raise L.SdaError("speech_embeddings: a (1, L) waveform")
    wave16 = resample_audio(wave, sample_rate, audio_resample_rate, lowpass_filter_width=int(preprocs["lowpass_filter_width"]))
    if preprocs["last4layers"]:
        emb = embedder.embed(wave16)                                 # (H, frames)
    else:
        emb = embedder.conv_features(wave16)                         # (C, frames): `feature_extractor`'s output, no transformer
    rate_after = audio_resample_rate * emb.shape[-1] / wave16.shape[-1]
    return resample_fft(emb, up=preprocs["brain_resample_rate"] / rate_after)


# ---------------------------------------------------------------------------------------------------------------
# log-mel speech features: the STFT on the window GEMM (or, algorithm="fft", on sda_stft_fft_f32), then sda_mel_power_f32
# ---------------------------------------------------------------------------------------------------------------
@lru_cache(maxsize=16)
def _stft_window(n_fft: int, win_length: int) -> Tuple[np.ndarray, float]:
    """(the zero-padded periodic Hann window, its L2 norm)"""
    if n_fft < 1 or not 1 <= win_length <= n_fft:
        raise ValueError("stft_matrix: n_fft >= 1 and 1 <= win_length <= n_fft")
    w = np.zeros(n_fft, dtype=np.float64)
    left = (n_fft - win_length) // 2
    w[left:left + win_length] = 0.5 - 0.5 * np.cos(2 * np.pi * np.arange(win_length, dtype=np.float64) / win_length)
    w.setflags(write=False)
    return w, math.sqrt(float((w * w).sum()))


def stft_window(n_fft: int, win_length: Optional[int] = None, normalized: bool = True) -> np.ndarray:
    """The window of `stft_matrix` on its own, float64 (n_fft,): w / c with w the periodic Hann window of win_length zero-padded
    to n_fft ((n_fft - win_length) // 2 on the left) and c = sqrt(sum w^2) when `normalized`, else 1 — what the FFT path
    multiplies each frame by, so that both paths use one definition."""
    n_fft = int(n_fft)
    w, norm = _stft_window(n_fft, n_fft if win_length is None else int(win_length))
    out = w / (norm if normalized else 1.0)
    out.setflags(write=False)
    return out


@lru_cache(maxsize=16)
def _fft_twiddles(n_fft: int) -> np.ndarray:
    if n_fft < 2 or n_fft % 2:
        raise ValueError("fft_twiddles: an even n_fft >= 2")
    j = np.arange(n_fft // 2, dtype=np.int64)
    # the angle reduced in integers to the first octant, as _stft_matrix reduces b k mod n_fft: j = 0 gives exactly (1, 0),
    # j = n_fft / 4 exactly (0, -1), j = n_fft / 8 equal magnitudes (cos and sin of one and the same angle pi / 4)
    q, r = np.divmod(8 * j, n_fft)                                      # octant q < 4, 8 j = q n_fft + r
    odd = q % 2 == 1
    ang = 2 * np.pi * np.where(odd, n_fft - r, r).astype(np.float64) / (8 * n_fft)      # in [0, pi / 4]
    c, sn = np.cos(ang), np.sin(ang)
    c[odd & (r == 0)] = sn[odd & (r == 0)] = math.sqrt(0.5)            # pi / 4 itself: libm's cos and sin differ in the last bit
    cos = np.select([q == 0, q == 1, q == 2, q == 3], [c, sn, -sn, -c])
    sin = np.select([q == 0, q == 1, q == 2, q == 3], [sn, c, c, sn])
    tw = np.stack([cos, -sin], axis=1)
    tw[tw == 0] = 0.0                                                   # no negative zeros
    tw.setflags(write=False)
    return tw


def fft_twiddles(n_fft: int) -> np.ndarray:
    """The table `sda_stft_fft_f32` takes, float64 (n_fft / 2, 2), read-only and cached: row j = (cos, -sin)(2 pi j / n_fft) =
    exp(-2 pi i j / n_fft).  It serves the half-size complex transform (every second row) and the real-FFT split step."""
    return _fft_twiddles(int(n_fft))


@lru_cache(maxsize=16)
def _stft_matrix(n_fft: int, win_length: int, normalized: bool) -> np.ndarray:
    w, norm = _stft_window(n_fft, win_length)
    c = norm if normalized else 1.0
    k = np.arange(n_fft, dtype=np.int64)[:, None]
    b = np.arange(n_fft // 2 + 1, dtype=np.int64)[None, :]
    ang = 2 * np.pi * ((b * k) % n_fft).astype(np.float64) / n_fft      # the angle reduced in integers: exact zeros, exact symmetry
    B = np.empty((n_fft, 2 * (n_fft // 2 + 1)), dtype=np.float64)
    B[:, 0::2] = w[:, None] * np.cos(ang) / c
    B[:, 1::2] = -w[:, None] * np.sin(ang) / c
    B.setflags(write=False)
    return B


def stft_matrix(n_fft: int, win_length: Optional[int] = None, normalized: bool = True) -> np.ndarray:
    """One STFT frame as a matrix, float64 (n_fft, 2 (n_fft // 2 + 1)): frame @ B = the one-sided spectrum of the windowed
    frame, real and imaginary parts interleaved,
        B[k, 2 b] = w[k] cos(2 pi ((b k) mod n_fft) / n_fft) / c,     B[k, 2 b + 1] = -w[k] sin(2 pi ((b k) mod n_fft) / n_fft) / c.
    w = the periodic Hann window 0.5 - 0.5 cos(2 pi k / win_length) (torch.hann_window's default), zero-padded to n_fft on both
    sides with (n_fft - win_length) // 2 on the left when shorter, as torch.stft centres it; c = sqrt(sum w^2) when `normalized`
    (torchaudio's Spectrogram(normalized=True) = "window": the spectrum divided by the window's L2 norm), else 1.  Parity with
    torch.stft's own output: unpinned (module docstring)."""
    n_fft = int(n_fft)
    return _stft_matrix(n_fft, n_fft if win_length is None else int(win_length), bool(normalized))


_warned_empty_filters = False


@lru_cache(maxsize=16)
def _mel_filterbank(n_freqs: int, f_min: float, f_max: float, n_mels: int, sample_rate: int) -> np.ndarray:
    if n_freqs < 1 or n_mels < 1 or not 0 <= f_min < f_max:
        raise ValueError("mel_filterbank: n_freqs >= 1, n_mels >= 1, 0 <= f_min < f_max")
    all_freqs = np.linspace(0, sample_rate // 2, n_freqs)
    m_min, m_max = 2595.0 * math.log10(1.0 + f_min / 700.0), 2595.0 * math.log10(1.0 + f_max / 700.0)
    f_pts = 700.0 * (10.0 ** (np.linspace(m_min, m_max, n_mels + 2) / 2595.0) - 1.0)
    f_diff = f_pts[1:] - f_pts[:-1]
    slopes = f_pts[None, :] - all_freqs[:, None]                        # (n_freqs, n_mels + 2)
    down = -slopes[:, :-2] / f_diff[:-1]
    up = slopes[:, 2:] / f_diff[1:]
    fb = np.maximum(0.0, np.minimum(down, up))
    fb.setflags(write=False)
    return fb


def mel_filterbank(n_freqs: int, f_min: float, f_max: float, n_mels: int, sample_rate: int) -> np.ndarray:
    """`torchaudio.functional.melscale_fbanks(n_freqs, f_min, f_max, n_mels, sample_rate, norm=None, mel_scale="htk")` by its
    documented rule, float64 (n_freqs, n_mels): all_freqs = linspace(0, sample_rate // 2, n_freqs); mel(f) = 2595 log10(1 + f / 700);
    n_mels + 2 points equally spaced in mel from f_min to f_max, mapped back to Hz as f_pts; triangles
        fb[b, j] = max(0, min((all_freqs[b] - f_pts[j]) / (f_pts[j + 1] - f_pts[j]), (f_pts[j + 2] - all_freqs[b]) / (f_pts[j + 2] - f_pts[j + 1]))).
    A filter narrower than the bin spacing can contain no bin and is then all zero (at n_fft = 512, 16 kHz, 120 filters some of
    the lowest are): torchaudio only warns, and so does this, once.  Parity with torchaudio's own array: unpinned."""
    global _warned_empty_filters
    fb = _mel_filterbank(int(n_freqs), float(f_min), float(f_max), int(n_mels), int(sample_rate))
    empty = int((fb.max(axis=0) == 0.0).sum())
    if empty and not _warned_empty_filters:
        _warned_empty_filters = True
        warnings.warn(f"mel_filterbank: {empty} of {n_mels} mel filters contain no frequency bin and are all zero "
                      f"(n_freqs = {n_freqs} may be too low for n_mels = {n_mels})")
    return fb


STFT_ALGORITHMS = ("gemm", "fft")


def check_stft_algorithm(algorithm: str, n_fft: int) -> str:
    """The argument check of `stft(..., algorithm=)`, which needs no device: "gemm" (any n_fft) or "fft" (the sizes
    `sda_stft_fft_f32` is built for); anything else raises — there is no silent fallback from one to the other."""
    if algorithm not in STFT_ALGORITHMS:
        raise L.SdaError(f"stft: algorithm {algorithm!r} is not one of {STFT_ALGORITHMS}")
    if algorithm == "fft" and int(n_fft) not in ops.STFT_FFT_SIZES:
        raise L.SdaError(f"stft: algorithm 'fft' takes n_fft in {ops.STFT_FFT_SIZES}, got {n_fft} (no fallback to 'gemm')")
    return algorithm


def stft(wave: torch.Tensor, n_fft: int = 512, hop_length: int = 128, win_length: Optional[int] = None, normalized: bool = True,
         center: bool = True, algorithm: str = "gemm") -> torch.Tensor:
    """`torch.stft(wave, n_fft, hop_length, win_length, window=hann_window(win_length), center=center, pad_mode="reflect",
    normalized=False, onesided=True)` divided by the window's L2 norm when `normalized` (torchaudio's Spectrogram), as real
    pairs: (..., L) -> fp32 (..., frames, n_freqs = n_fft // 2 + 1, 2) — FRAME-major, the layout the window GEMM leaves and
    `sda_mel_power_f32` reads (torch.stft returns (..., n_freqs, frames)).  center: n_fft // 2 samples of EVEN reflection per side
    (x[p], ..., x[1] | x | x[-2], ..., x[-1 - p]; not the odd extension of fir_filter), which needs L > n_fft // 2 as in torch;
    frames = 1 + L // hop_length.  Without it L >= n_fft and frames = 1 + (L - n_fft) // hop_length.  `stft_matrix` through
    `_apply_bank`: S = hop_length, K = n_fft, N = 2 n_freqs.  algorithm="fft" computes the same frames with `sda_stft_fft_f32`
    (csrc/stft_fft.hip; n_fft a power of two in 32 ... 2048) from `stft_window` and `fft_twiddles` instead: the same shape, dtype
    and layout, values within the two paths' rounding."""
    check_stft_algorithm(algorithm, n_fft)
    _check_device(wave, "stft")
    n_fft, hop = int(n_fft), int(hop_length)
    if n_fft < 1 or hop < 1:
        raise L.SdaError("stft: n_fft >= 1 and hop_length >= 1")
    n = wave.shape[-1]
    rows = wave.reshape(-1, n).float()
    if center:
        p = n_fft // 2
        if n <= p:
            raise L.SdaError(f"stft: reflection padding of {p} samples needs more than {p} samples, got {n}")
        rows = torch.cat([rows[:, 1:p + 1].flip(-1), rows, rows[:, n - 1 - p:n - 1].flip(-1)], dim=1)
    elif n < n_fft:
        raise L.SdaError(f"stft: {n} samples are fewer than n_fft = {n_fft}")
    frames = 1 + (rows.shape[1] - n_fft) // hop
    if algorithm == "fft":
        w = ops.UPLOADER.upload("stft.window", stft_window(n_fft, win_length, normalized).astype(np.float32), rows.device)
        tw = ops.UPLOADER.upload("stft.twiddle", fft_twiddles(n_fft).astype(np.float32), rows.device)
        y = ops.stft_fft(rows.contiguous(), w, tw, frames, hop, n_fft)
        return y.reshape(wave.shape[:-1] + (frames, n_fft // 2 + 1, 2))
    B = stft_matrix(n_fft, win_length, normalized)
    y = _apply_bank(rows, B.T, hop, frames)
    return y.contiguous().reshape(wave.shape[:-1] + (frames, n_fft // 2 + 1, 2))


def mel_spectrogram(wave: torch.Tensor, sample_rate: int = 16000, n_fft: int = 512, hop_length: int = 128, n_mels: int = 120,
                    f_min: float = 0.0, f_max: Optional[float] = None, normalized: bool = True,
                    log_eps: Optional[float] = None, algorithm: str = "gemm") -> torch.Tensor:
    """`torchaudio.transforms.MelSpectrogram(sample_rate, n_fft, hop_length=hop_length, f_min=f_min, f_max=f_max, n_mels=n_mels,
    power=2.0, normalized=normalized)` (Hann window of n_fft, centred, reflect padding, HTK mel scale, no filterbank
    normalisation; f_max = sample_rate // 2 when None), (..., L) -> fp32 (..., n_mels, 1 + L // hop_length): `stft`, then
    `sda_mel_power_f32` with `mel_filterbank`.  log_eps (>= 0) returns log(log_eps + mel) instead — the paper's compression with
    1e-5 (`log_mel`).  The defaults are the paper's: 120 mel bands of a 512-point STFT every 128 samples (8 ms) at 16 kHz.
    `algorithm` is `stft`'s."""
    spec = stft(wave, n_fft, hop_length, None, normalized, True, algorithm)
    fmax = float(int(sample_rate) // 2) if f_max is None else float(f_max)
    fb = mel_filterbank(int(n_fft) // 2 + 1, f_min, fmax, n_mels, sample_rate)
    return ops.mel_power(spec, torch.from_numpy(fb.astype(np.float32)).to(spec.device), log_eps)


def log_mel(wave: torch.Tensor, sample_rate: int = 16000, n_fft: int = 512, hop_length: int = 128, n_mels: int = 120,
            f_min: float = 0.0, f_max: Optional[float] = None, normalized: bool = True, eps: float = 1e-5,
            algorithm: str = "gemm") -> torch.Tensor:
    """log(eps + mel_spectrogram(wave, ...)), the log inside the kernel: fp32 (..., n_mels, frames)."""
    return mel_spectrogram(wave, sample_rate, n_fft, hop_length, n_mels, f_min, f_max, normalized, log_eps=eps, algorithm=algorithm)


def mel_embeddings(wave: torch.Tensor, sample_rate: int, preprocs, audio_resample_rate: int = 16000) -> torch.Tensor:
    """One audio file (1, L) at sample_rate -> float64 (n_mels, frames at brain_resample_rate): the sibling of
    `speech_embeddings` for the log-mel representation — resample to 16 kHz (preprocs["lowpass_filter_width"]), `log_mel`,
    FFT-resample from the frame rate audio_resample_rate / hop_length (125 Hz) to preprocs["brain_resample_rate"].  The optional
    preprocs["mel"] = {n_mels, n_fft, hop_length, eps, algorithm} overrides the paper's 120 / 512 / 128 / 1e-5 and the STFT's
    "gemm" (configs/config.yaml does not list the key)."""
    _check_device(wave, "mel_embeddings")
    if wave.dim() != 2 or wave.shape[0] != 1:
        raise L.SdaError("mel_embeddings: a (1, L) waveform")
    mel = dict(preprocs["mel"]) if "mel" in preprocs else {}
    n_mels, n_fft, hop = int(mel.get("n_mels", 120)), int(mel.get("n_fft", 512)), int(mel.get("hop_length", 128))
    wave16 = resample_audio(wave, sample_rate, audio_resample_rate, lowpass_filter_width=int(preprocs["lowpass_filter_width"]))
    emb = log_mel(wave16, audio_resample_rate, n_fft, hop, n_mels, eps=float(mel.get("eps", 1e-5)),
                  algorithm=str(mel.get("algorithm", "gemm")))[0]                                             # (n_mels, frames)
    return resample_fft(emb, up=preprocs["brain_resample_rate"] * hop / audio_resample_rate)
