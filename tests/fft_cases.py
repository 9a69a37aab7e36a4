"""Cases, the float64 restatement, the error bound and a mutable numpy fp32 emulation for the FFT path of the STFT
(`sda_stft_fft_f32`, csrc/stft_fft.hip, behind `signal_prep.stft(..., algorithm="fft")`), shared by tests/test_stft_fft_cpu.py
(which proves on the CPU that the restatement is the DFT, that the kernel's factorisation stays inside the bound and that the
cases and the bound see every planted bug) and tests/test_stft_fft_gpu.py (which runs them on the kernel).

The contract, for r < rows, m < frames, b <= n_fft / 2:
    X[r, m, b] = sum_{k < n_fft} window[k] x[r, m hop + k] exp(-2 pi i b k / n_fft),     out[r, m, b] = (Re X, Im X).

Restatement.  `restate`: np.fft.rfft of window * frame in float64 on the SAME fp32-valued x and window the kernel is given;
test_stft_fft_cpu proves it equal to the direct sum.  The twiddles are NOT shared: the reference uses exact exponentials, the
rounding of the kernel's fp32 table is part of the kernel's error (mu below).

The error bound (u = 2^-24), per frame in the 2-norm over the one-sided spectrum, relative to the 2-norm of the reference
frame.  Higham, Accuracy and Stability of Numerical Algorithms, 2nd ed., section 24.1, Theorem 24.2: a radix-2 FFT of t stages,
each stage y = A_k x with ||A_k||_2 = || |A_k| ||_2 = sqrt 2 computed as (A_k + dA_k) x, |dA_k| <= eta |A_k|, satisfies
    ||y^ - y||_2 / ||y||_2 <= t eta / (1 - t eta),     eta = mu + gamma_4 (sqrt 2 + mu),     gamma_4 = 4 u / (1 - 4 u),
mu = u for correctly rounded twiddles; eta covers one complex product by a rounded twiddle and one complex addition per output.
The kernel's factorisation differs, so the count is redone for it:
  * The complex transform has H = n_fft / 2 points and runs as radix-4 Stockham passes plus one twiddle-free radix-2 pass when
    log2 H is odd.  A radix-4 pass is two levels of complex additions (the factors +-1, +-i in between are exact) followed by ONE
    product by a table entry: it is the product of two radix-2 stage matrices with one of the two diagonal twiddle matrices
    exact, so it is charged 2 eta; every twiddle is a single correctly rounded table entry (mu = u), never a product of two.
    The products are fused (fmaf(a, b, fl(c d)): one rounding fewer than the three gamma_4 allows for).  The radix-2 pass has
    no product: 1 eta.  Together log2 H stages, whatever the mix.
  * The split step  X[b] = E + W^b O,  E, O = (Z[b] +- conj Z[H - b]) / 2 (the halving exact),  is one more addition level,
    one product by a table entry and one addition: 2 eta as far as the operations go.  As a (real-linear) map it is sqrt 2
    times an isometry like a butterfly stage (||X_full||^2 = n_fft ||y||^2 = 2 ||Z||^2), but its matrix of absolute values has
    norm 2, not sqrt 2 (|X[b]|, |X[H - b]| <= |Z[b]| + |Z[H - b]| each), so its rounding weighs sqrt 2 more than a
    butterfly's: charged 3 eta.
  * y = fl(window x) = window x (1 + d), |d| <= u: the input of the transform is perturbed by at most u in norm, and so is,
    by linearity and Parseval, the full spectrum.
  * The theorem speaks of the full spectrum; the kernel stores, and the bound is taken over, bins 0 ... H only.  The error of
    the one-sided half is at most the full error, and ||X_full||_2 <= sqrt 2 ||X_onesided||_2: a factor sqrt 2.
So with k = log2(n_fft / 2) + 3:
    bound(n_fft) = sqrt 2 ((1 + u) (1 + k eta / (1 - k eta)) - 1)           66 u at n_fft = 32, 123 u at 2048
and, where a caller needs an elementwise budget,  |dRe|, |dIm| <= bound ||reference frame||_2.  Nothing here is fitted to what
the kernel or the emulation give (the emulation's worst relative error is 1.5 to 3 u at every size)."""
import math

import numpy as np

from tests import signal_cases as SC

U = SC.U
F32 = np.float32

N_FFTS = (32, 64, 128, 256, 512, 1024, 2048)     # every instantiation: smaller than a wavefront (32); odd / even log2(n_fft / 2)
                                                # (64, 256, 1024 against 32, 128, 512, 2048); the paper's (512); the largest
ROWS = (1, 3)
SLACKS = ((0, 0), (3, 5))                  # floats added to (x row stride, out_pitch): the minimum, then odd pitches


def hops(n_fft):
    return (1, n_fft // 4, n_fft, n_fft + 3)


def frame_counts(n_fft):
    """1, 2, 37 and one past what a workgroup owns (asked of the product, not written down here)"""
    from speech_decoding_amd import ops
    return tuple(sorted({1, 2, 37, ops.stft_fft_frames_per_workgroup(n_fft) + 1}))


def kernel_runs(n_fft):
    return [(hop, rows, frames) for hop in hops(n_fft) for rows in ROWS for frames in frame_counts(n_fft)]


def rel_bound(n_fft):
    """the module docstring's bound: per frame, 2-norm over the one-sided spectrum, relative to the reference frame's"""
    k = int(round(math.log2(n_fft // 2))) + 3
    g4 = 4 * U / (1 - 4 * U)
    eta = U + g4 * (math.sqrt(2.0) + U)
    return math.sqrt(2.0) * ((1 + U) * (1 + k * eta / (1 - k * eta)) - 1)


def product_tables(n_fft, win_length=None, normalized=True):
    """the fp32 window and twiddle table the product uploads, as float64"""
    from speech_decoding_amd import signal_prep as SP
    return (SP.stft_window(n_fft, win_length, normalized).astype(F32).astype(np.float64),
            SP.fft_twiddles(n_fft).astype(F32).astype(np.float64))


def real_operands(n_fft, hop, rows, frames, kind=0):
    """fp32-valued float64 rows of exactly (frames - 1) hop + n_fft samples.  kind 0: white noise; 1: a strong tone between two
    bins plus weak noise; 2: a DC offset plus noise; 3: noise with a dynamic range of three decades"""
    L = (frames - 1) * hop + n_fft
    rs = np.random.RandomState(n_fft + 7 * hop + 100 * rows + frames + 1000 * kind)
    k = np.arange(L)
    if kind == 0:
        x = rs.randn(rows, L)
    elif kind == 1:
        x = 100 * np.cos(2 * np.pi * 7.3 * k / n_fft)[None, :] + 1e-3 * rs.randn(rows, L)
    elif kind == 2:
        x = 3 + 1e-2 * rs.randn(rows, L)
    else:
        x = rs.randn(rows, L) * np.exp(rs.randn(rows, L) * 3)
    return x.astype(F32).astype(np.float64)


# ---------------------------------------------------------------------------------------------------------------
# the contract, restated
# ---------------------------------------------------------------------------------------------------------------
def direct(x, window, hop, frames, n_fft):
    """the sum of the contract, term by term as a float64 matrix product: (rows, frames, n_freqs, 2)"""
    k = np.arange(n_fft)[:, None]
    b = np.arange(n_fft // 2 + 1)[None, :]
    ang = 2 * np.pi * ((b * k) % n_fft) / n_fft
    fr = SC.windows(x, hop, n_fft, frames) * window
    return np.stack([fr @ np.cos(ang), -(fr @ np.sin(ang))], axis=-1)


def restate(x, window, hop, frames, n_fft):
    """np.fft.rfft of window * frame, float64: (rows, frames, n_freqs, 2)"""
    X = np.fft.rfft(SC.windows(x, hop, n_fft, frames) * window, axis=-1)
    return np.stack([X.real, X.imag], axis=-1)


def frame_norms(ref):
    """(rows, frames) 2-norms of the reference frames over the one-sided spectrum"""
    return np.sqrt((ref * ref).sum(axis=(-1, -2)))


def miss(got, ref, n_fft):
    """max over the frames of ||got - ref||_2 / (rel_bound ||ref||_2); 0 where a frame is reproduced exactly, inf for a NaN"""
    d = got - ref
    err = np.sqrt((d * d).sum(axis=(-1, -2)))
    with np.errstate(divide="ignore", invalid="ignore"):
        q = np.where(err == 0, 0.0, err / (rel_bound(n_fft) * frame_norms(ref)))
    q = np.where(np.isnan(err), np.inf, q)
    return float(q.max())


def elementwise_budget(ref, n_fft):
    """|dRe|, |dIm| <= rel_bound ||frame||_2, in the shape of ref"""
    return np.broadcast_to((rel_bound(n_fft) * frame_norms(ref))[..., None, None], ref.shape)


# ---------------------------------------------------------------------------------------------------------------
# the kernel's factorisation in numpy fp32, with planted bugs
# ---------------------------------------------------------------------------------------------------------------
MUTANTS = ("twiddle_index_off_by_one", "positive_exponent", "split_conjugate_missing", "nyquist_dropped", "nyquist_imag_kept",
           "window_skipped", "window_shifted", "frame_start_plus", "frame_start_minus", "digit_reversal_omitted",
           "twiddles_fp16")


def _fma(a, b, c):
    """fmaf: the product is exact in float64, so this rounds once (but for a double rounding of no consequence here)"""
    return (a.astype(np.float64) * b.astype(np.float64) + c.astype(np.float64)).astype(F32)


def emulate(x, window, twiddle, hop, frames, n_fft, mutant=None):
    """csrc/stft_fft.hip operation by operation in fp32 on x (rows, L), window (n_fft,), twiddle (n_fft / 2, 2):
    z = window x as n_fft / 2 complex points, radix-4 Stockham passes at strides 1, 4, 16, ... (+ one radix-2 pass), the split
    step.  Returns float64 (rows, frames, n_freqs, 2).  `mutant` plants one bug."""
    N, H = n_fft, n_fft // 2
    Q = H // 4
    w = window.astype(F32)
    tw = twiddle.astype(F32)
    if mutant == "twiddles_fp16":
        tw = tw.astype(np.float16).astype(F32)
    if mutant == "positive_exponent":
        tw = tw * np.array([1, -1], dtype=F32)
    full = np.concatenate([tw, -tw])                                 # exp(-2 pi i j / N) for j < N: the second half negated
    step = 1 if mutant == "twiddle_index_off_by_one" else 0

    def W(j):
        e = full[(j + step) % N]
        return e[:, 0], e[:, 1]

    shift = (mutant == "frame_start_plus") - (mutant == "frame_start_minus")
    xz = np.concatenate([np.zeros((x.shape[0], 1)), x, np.zeros((x.shape[0], 1))], axis=1).astype(F32)
    idx = np.arange(frames)[:, None] * hop + shift + 1 + np.arange(N)[None, :]
    y = xz[:, idx]
    if mutant == "window_shifted":
        y = y * np.roll(w, -1)
    elif mutant != "window_skipped":
        y = y * w
    zr, zi = y[..., 0::2].copy(), y[..., 1::2].copy()
    s, first = 1, True
    while 4 * s <= H:
        t = np.arange(Q)
        ps, q = t & ~(s - 1), t & (s - 1)
        ar, ai, br, bi = zr[..., t], zi[..., t], zr[..., t + Q], zi[..., t + Q]
        cr, ci, dr, di = zr[..., t + 2 * Q], zi[..., t + 2 * Q], zr[..., t + 3 * Q], zi[..., t + 3 * Q]
        pr, pi, mr, mi = ar + cr, ai + ci, ar - cr, ai - ci
        sr, si, tr, ti = br + dr, bi + di, br - dr, bi - di
        ys = [(pr + sr, pi + si), (mr + ti, mi - tr), (pr - sr, pi - si), (mr - ti, mi + tr)]
        nr, ni = np.empty_like(zr), np.empty_like(zi)
        for k in range(4):
            yr, yi = ys[k]
            if k:
                wr, wi = W(2 * k * ps)
                yr, yi = _fma(yr, wr, -(yi * wi)), _fma(yr, wi, yi * wr)
            o = t + k * Q if (mutant == "digit_reversal_omitted" and first) else q + 4 * ps + s * k
            nr[..., o], ni[..., o] = yr, yi
        zr, zi = nr, ni
        s, first = 4 * s, False
    if s < H:                                                        # log2 H odd: s = H / 2
        q = np.arange(H // 2)
        ar, ai, br, bi = zr[..., q], zi[..., q], zr[..., q + H // 2], zi[..., q + H // 2]
        zr, zi = np.concatenate([ar + br, ar - br], axis=-1), np.concatenate([ai + bi, ai - bi], axis=-1)
    out = np.zeros(zr.shape[:-1] + (H + 1, 2), dtype=F32)
    b = np.arange(1, H)
    wr, wi = full[b, 0], full[b, 1]
    ar, ai, cr, ci = zr[..., b], zi[..., b], zr[..., H - b], zi[..., H - b]
    if mutant == "split_conjugate_missing":
        ci = -ci
    half = F32(0.5)
    er, ei, pr, pi = half * (ar + cr), half * (ai - ci), half * (ai + ci), half * (cr - ar)
    out[..., 1:H, 0] = _fma(wr, pr, _fma(-wi, pi, er))
    out[..., 1:H, 1] = _fma(wr, pi, _fma(wi, pr, ei))
    out[..., 0, 0] = zr[..., 0] + zi[..., 0]
    if mutant != "nyquist_dropped":
        out[..., H, 0] = zr[..., 0] - zi[..., 0]
    if mutant == "nyquist_imag_kept":
        out[..., H, 1] = zi[..., 0]
    return out.astype(np.float64)


# ---------------------------------------------------------------------------------------------------------------
# exact cases: frames that are constant (or constant with alternating sign) under a window of ones
# ---------------------------------------------------------------------------------------------------------------
def constant_frames(n_fft, rows, frames, alternating=False):
    """hop = n_fft, window of ones, frame (r, m) = the integer c[r, m] in -8 ... 8 at every sample (times (-1)^k when
    alternating): bin 0 (the Nyquist bin when alternating) is exactly n_fft c, every other float exactly zero — in ANY
    factorisation, since every butterfly difference is an exact zero and every sum a small integer times a power of two.
    Returns (x (rows, frames n_fft) int64, expected (rows, frames, n_freqs, 2) int64)."""
    c = SC.ints((rows, frames), 8, 31 * n_fft + 5 * rows + frames + alternating)
    sign = (-1) ** np.arange(n_fft) if alternating else np.ones(n_fft, dtype=np.int64)
    x = (c[:, :, None] * sign[None, None, :]).reshape(rows, frames * n_fft)
    ref = np.zeros((rows, frames, n_fft // 2 + 1, 2), dtype=np.int64)
    ref[:, :, n_fft // 2 if alternating else 0, 0] = n_fft * c
    return x, ref


# ---------------------------------------------------------------------------------------------------------------
# the public layer: mel_cases' end-to-end budget with the FFT's elementwise budget in place of signal_cases.bound
# ---------------------------------------------------------------------------------------------------------------
def e2e(x, window, fb, n_fft, hop, log_eps=None):
    """mel_cases.e2e for the FFT path: x (rows, L) float64, `window` and `fb` as the product uploads them (fp32-valued).
    Returns spec / spec_lim, mel / mel_lim, logmel / logmel_lim and rho as mel_cases.e2e does."""
    from tests import mel_cases as MC
    log_eps = MC.EPS if log_eps is None else log_eps
    xp, s, frames = MC.stft_frames(x, n_fft, hop)
    spec = restate(xp, window, s, frames, n_fft)
    d = elementwise_budget(spec, n_fft)
    re, im, dre, dim = np.abs(spec[..., 0]), np.abs(spec[..., 1]), d[..., 0], d[..., 1]
    dP = 2 * (re * dre + im * dim) + dre * dre + dim * dim
    mel = MC.mel_power(spec, fb)
    carried = np.einsum("rmb,bj->rjm", dP, fb)
    mel_lim = carried + MC.rel_bound(fb.shape[0]) * (mel + carried)
    eps = float(np.float32(log_eps))
    with np.errstate(divide="ignore", invalid="ignore"):
        logmel = np.log(eps + mel)
        rho = mel_lim / (eps + mel) + U
    return {"spec": spec, "spec_lim": d, "mel": mel, "mel_lim": mel_lim, "logmel": logmel, "logmel_lim": MC.log_bound(logmel, rho),
            "rho": rho}
