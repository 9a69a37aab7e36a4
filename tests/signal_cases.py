"""Cases, float64 / integer restatements and a mutable numpy emulation for the signal-conditioning path
(speech_decoding_amd/signal_prep.py on csrc/window_gemm.hip), shared by tests/test_signal_prep_cpu.py (which proves on the CPU
that the restatements agree with np.convolve and that the cases see every bug the kernel can have) and
tests/test_signal_prep_gpu.py (which runs them on the kernel).

The kernel's contract:   out[r, m N + j] = sum_{k < K} x[r, m S + k] B[k, j].
With integer operands every partial sum is an integer far below 2^24: any summation order gives the same fp32 value, so the
kernel must reproduce the integer reference with torch.equal.  On real operands a k-ordered fp32 fma chain of K terms differs
from the exact sum by at most  K u / (1 - K u) * sum |x B|,  u = 2^-24, whatever the order (Higham, Accuracy and Stability of
Numerical Algorithms, 2nd ed., eq. 3.7 with one rounding per fused step): bound() is 1.01 K u sum |x B|.  Both sides take the
SAME fp32 operands (the restatements are evaluated on what the kernel is given), so the bound is about the sum alone."""
import math

import numpy as np

# (S, K, N, why) for the direct kernel calls; rows x frames below for each, the audio shape at rows = 1, frames = 3 only
KERNEL_SHAPES = [
    (4, 10, 4, "below one tile"),
    (32, 64, 32, "one column fragment, stride of 32 words"),
    (64, 318, 64, "stride a multiple of 32 words: the skewed image"),
    (7, 29, 5, "all odd"),
    (3, 41, 1, "N = 1"),
    (160, 174, 441, "N ragged and wider than a tile; windows staged side by side"),
    (441, 1155, 160, "the audio shape"),
    (90, 1500, 7, "the span staged in two slices of the contraction"),
]
KERNEL_ROWS = (1, 3, 33)
KERNEL_FRAMES = (1, 2, 37)
AUDIO_SHAPE = (441, 1155, 160)


def kernel_runs(S, K, N):
    """(rows, frames) pairs a shape runs at"""
    if (S, K, N) == AUDIO_SHAPE:
        return [(1, 3)]
    return [(r, f) for r in KERNEL_ROWS for f in KERNEL_FRAMES]


# FIR through the window GEMM against np.convolve, exact: (rows, L, K, G)
FIR_EXACT = [(3, 100, 7, 4), (5, 257, 33, 32), (2, 20, 33, 32), (1, 1, 5, 4), (3, 1000, 255, 64)]
# (orig, new, lowpass_filter_width) -> bank shape
RESAMPLE = [((44100, 16000, 128), (160, 1155)), ((48000, 16000, 6), (1, 41)), ((16000, 44100, 6), (441, 174)),
            ((22050, 16000, 16), (320, 487))]
# (sfreq, l_freq, h_freq) -> taps
BANDPASS = [((1000, 1, 60), 3301), ((500, 1, 60), 1651), ((120, 2, 30), 199)]

U = 2.0 ** -24


def ints(shape, R, seed):
    return np.random.RandomState(seed).randint(-R, R + 1, size=shape).astype(np.int64)


def dyadic(shape, seed):
    """seeded N(0, 1) values rounded to multiples of 2^-10: fp32-exact, and so are 2 a - b of any two of them"""
    return np.round(np.random.RandomState(seed).randn(*shape) * 1024) / 1024


# ---------------------------------------------------------------------------------------------------------------
# the contract, restated
# ---------------------------------------------------------------------------------------------------------------
def windows(x, S, K, frames):
    """(rows, Lx) -> (rows, frames, K) strided windows (a copy)"""
    idx = np.arange(frames)[:, None] * S + np.arange(K)[None, :]
    return x[:, idx]


def window_gemm(x, B, S, frames):
    """out[r, m N + j] = sum_k x[r, m S + k] B[k, j] in the operands' own type (int64 or float64)"""
    K, N = B.shape
    return (windows(x, S, K, frames) @ B).reshape(x.shape[0], frames * N)


def bound(x, B, S, frames, K=None):
    """1.01 K 2^-24 (|x| (*) |B|) per output; K = the number of taps that can be nonzero (B's rows unless given)"""
    K = B.shape[0] if K is None else K
    return 1.01 * K * U * window_gemm(np.abs(x), np.abs(B), S, frames)


def odd_pad(x, pad, even=False):
    """mne's "reflect_limited": `pad` samples of odd extension per side, zero-filled where the row is shorter.
    even=True is a mutant: mirror without the point reflection."""
    n = x.shape[-1]
    p = min(pad, n - 1)
    z = np.zeros(x.shape[:-1] + (pad - p,), dtype=x.dtype)
    li, ri = x[..., p:0:-1], x[..., -2:-p - 2:-1]
    left = li if even else 2 * x[..., :1] - li
    right = ri if even else 2 * x[..., -1:] - ri
    return np.concatenate([z, left, x, right, z], axis=-1)


def fir_same(x, taps):
    """zero-phase "same" FIR: np.convolve(odd-padded row, taps, 'valid') per row"""
    K = len(taps)
    xp = odd_pad(x, (K - 1) // 2)
    return np.stack([np.convolve(row, taps, "valid") for row in xp])


def toeplitz_blocks(bank, S, G, shift=0):
    """the block-Toeplitz grouping written element by element (signal_prep.window_matrix is the vectorised product code);
    shift = 1 is a mutant: B one row late"""
    P, Kw = bank.shape
    out = np.zeros((Kw + (G - 1) * S, G * P), dtype=bank.dtype)
    for g in range(G):
        for p in range(P):
            for k in range(Kw):
                r = g * S + k + shift
                if r < out.shape[0]:
                    out[r, g * P + p] = bank[p, k]
    return out


MUTANTS = ("b_shifted_row", "stride_plus", "stride_minus", "taps_not_reversed", "even_reflection", "dropped_k_tail",
           "dropped_last_column", "frame_off_by_one")


def emulate(x, B, S, frames, mutant=None):
    """numpy emulation of the kernel's contract on (rows, Lx) x and (K, N) B, zero beyond the row like the staged image;
    `mutant` plants one of the kernel-level bugs"""
    K, N = B.shape
    if mutant == "dropped_k_tail":
        K = K // 4 * 4
        B = B[:K]
    s = S + (mutant == "stride_plus") - (mutant == "stride_minus")
    first = 1 if mutant == "frame_off_by_one" else 0
    need = (frames - 1 + first) * max(s, 1) + K
    xz = np.concatenate([x, np.zeros((x.shape[0], max(need - x.shape[1], 0)), dtype=x.dtype)], axis=1)
    idx = (np.arange(frames)[:, None] + first) * s + np.arange(K)[None, :]
    out = xz[:, idx] @ B
    if mutant == "dropped_last_column":
        out[..., N - 1] = 0
    return out.reshape(x.shape[0], frames * N)


def fir_through_window_gemm(x, taps, G, mutant=None, matrix=None):
    """fir_same by the kernel's route: odd padding, reversed taps as a one-phase bank, G frames grouped, the emulated kernel.
    `matrix` = the function that builds the grouped matrix (default: toeplitz_blocks)."""
    rows, n = x.shape
    K = len(taps)
    xp = odd_pad(x, (K - 1) // 2, even=mutant == "even_reflection")
    bank = (taps if mutant == "taps_not_reversed" else taps[::-1])[None, :]
    Bm = toeplitz_blocks(bank, 1, G, shift=1) if mutant == "b_shifted_row" else (matrix or toeplitz_blocks)(bank, 1, G)
    groups = -(-n // G)
    need = (groups - 1) * G + Bm.shape[0]
    xz = np.concatenate([xp, np.zeros((rows, max(need - xp.shape[1], 0)), dtype=xp.dtype)], axis=1)
    return emulate(xz, Bm, G, groups, mutant)[:, :n]


# ---------------------------------------------------------------------------------------------------------------
# torchaudio's sinc_interp_hann resampler, restated scalar by scalar
# ---------------------------------------------------------------------------------------------------------------
def sinc_bank(orig_freq, new_freq, lpw=6, rolloff=0.99):
    g = math.gcd(orig_freq, new_freq)
    orig, new = orig_freq // g, new_freq // g
    base = min(orig, new) * rolloff
    width = int(math.ceil(lpw * orig / base))
    bank = np.empty((new, 2 * width + orig), dtype=np.float64)
    for p in range(new):
        t = (-p / new + np.arange(-width, width + orig) / orig) * base
        t = np.minimum(np.maximum(t, -lpw), lpw)
        with np.errstate(invalid="ignore", divide="ignore"):
            s = np.where(t == 0, 1.0, np.sin(math.pi * t) / (math.pi * t))
        bank[p] = s * np.cos(math.pi * t / (2 * lpw)) ** 2 * (base / orig)
    return bank, width, orig, new


def resample(x, bank, width, orig, new):
    """(rows, L) float64 -> (rows, ceil(new L / orig)): zero-pad (width, width + orig), the bank at stride orig"""
    rows, n = x.shape
    xp = np.concatenate([np.zeros((rows, width)), x, np.zeros((rows, width + orig))], axis=1)
    frames = n // orig + 1
    return window_gemm(xp, bank.T.copy(), orig, frames)[:, :-(-new * n // orig)]


def resample_bound(x, bank, width, orig, new):
    rows, n = x.shape
    xp = np.concatenate([np.zeros((rows, width)), x, np.zeros((rows, width + orig))], axis=1)
    return bound(xp, bank.T.copy(), orig, n // orig + 1)[:, :-(-new * n // orig)]


def fir_bound(x, taps):
    K = len(taps)
    xp = odd_pad(x, (K - 1) // 2)
    return bound(xp, np.abs(taps)[::-1][:, None].copy(), 1, x.shape[-1])
