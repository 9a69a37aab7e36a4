"""Cases, float64 / integer restatements and a mutable numpy emulation for the log-mel path (speech_decoding_amd/signal_prep.py:
stft on csrc/window_gemm.hip, then csrc/mel_power.hip), shared by tests/test_mel_cpu.py (which proves on the CPU that the
restatements agree with np.fft and that the cases and bounds see every bug the path can have) and tests/test_mel_gpu.py
(which runs them on the kernels).

The kernel's contract (`sda_mel_power_f32`):
    P[r, m, b]   = spec[r, m, b, 0]^2 + spec[r, m, b, 1]^2
    mel[r, j, m] = sum_{b < n_freqs} P[r, m, b] fb[b, j]
    out[r, j, m] = mel                      (log_eps < 0)
                 = logf(log_eps + mel)      (otherwise)

Exact case.  Integer re, im in [-8, 8] and fb in [0, 4]: P <= 128, every partial sum is an integer <= 257 * 128 * 4 < 2^24, so
any evaluation order gives the same fp32 value and the kernel must reproduce the int64 restatement with torch.equal.

Real operands, no log (u = 2^-24).  The kernel computes P^ = fmaf(im, im, fl(re re)) = (re^2 (1 + d1) + im^2)(1 + d2): both
squares are non-negative, so P^ = P (1 + t2) with |t2| <= g2 (g_k = k u / (1 - k u)).  The mel sum is one fused multiply-add
chain of n = n_freqs steps: term b is rounded by the steps b, ..., n - 1, at most n times (Higham, Accuracy and Stability of
Numerical Algorithms, 2nd ed., eq. 3.7 with one rounding per fused step — the argument of signal_cases.bound).  Every term
P fb is non-negative, so sum |terms| is the sum itself and the error is RELATIVE:
    |mel^ - mel| <= g_{n + 2} mel <= 1.01 (n_freqs + 3) u mel,
the spare unit covering the rounding of log_eps + mel below.  `ref` is evaluated in float64 on the SAME fp32 operands.

With log.  a^ = fl(log_eps + mel^) = (log_eps + mel^)(1 + d), log_eps >= 0, so a^ = a (1 + t) with |t| <= g_{n + 3}
<= rho = 1.01 (n_freqs + 3) u, and |log a^ - log a| <= -log(1 - rho).  The device logf adds its own error: LOGF_REL of
max(|log a|, 1), see below.

End to end.  The STFT is the window GEMM: re, im carry d = signal_cases.bound(padded wave, B, hop, frames) (K = n_fft).
P computed from re + dre, im + dim differs from P by at most  dP = 2 (|re| dre + |im| dim) + dre^2 + dim^2,  the exact mel sum
of the kernel's own operands from mel by at most  sum_b fb dP,  and the kernel's fp32 chain from that by the relative bound
above — `e2e()` returns all three budgets."""
import math

import numpy as np

from tests import signal_cases as SC

U = SC.U

# (n_freqs, n_mels, what it reaches)
KERNEL_SHAPES = [
    (1, 1, "smallest possible"),
    (5, 3, "below one fragment"),
    (32, 32, "whole fragments"),
    (33, 33, "one past a fragment in both axes"),
    (257, 120, "the paper's setting: odd contraction tail, ragged last column block"),
    (64, 130, "more mel columns than one workgroup's tile"),
]
KERNEL_ROWS = (1, 3)
KERNEL_FRAMES = (1, 2, 37, 129)            # 129: one past a 128-frame tile
SLACKS = ((0, 0), (3, 5))                  # floats added to (spec_pitch, out_pitch): the minimum, then odd pitches
SHAPE_IDS = [f"F{f}-M{m}" for f, m, _ in KERNEL_SHAPES]

PAPER = dict(sample_rate=16000, n_fft=512, hop_length=128, n_mels=120)
SMALL = dict(sample_rate=16000, n_fft=64, hop_length=16, n_mels=10)
E2E_LENGTHS = (257, 1000, 4096 + 77)
EPS = 1e-5

# The device logf.  Its ulp figure is in the HIP math API documentation, which is not part of the ROCm installation the tests
# run against, so it was measured once on the MI355X against float64, through the kernel itself (LABNOTES, "Log-mel"): 106 470
# arguments log_eps + mel from 1e-5 to 6.7e7, a superset of the range in these tests, max |logf(a) - log a| / max(|log a|, 1)
# = 3.06 * 2^-24 (2.3 ulp of the result, at a = 1.4e-5).  Allowed: twice that.
LOGF_REL = 2 * 3.06 * U


def kernel_runs():
    return [(r, f) for r in KERNEL_ROWS for f in KERNEL_FRAMES]


def int_operands(n_freqs, n_mels, rows, frames):
    seed = 1000 * n_freqs + 10 * n_mels + 100 * rows + frames
    return SC.ints((rows, frames, n_freqs, 2), 8, seed), SC.ints((n_freqs, n_mels), 2, seed + 1) + 2      # fb in [0, 4]


def real_operands(n_freqs, n_mels, rows, frames, scale=1.0, zero_column=False):
    """fp32-valued float64 operands: normal spectrum, uniform non-negative filterbank (optionally with one all-zero column)"""
    rs = np.random.RandomState(7 * n_freqs + n_mels + rows + frames)
    spec = (rs.randn(rows, frames, n_freqs, 2) * scale).astype(np.float32).astype(np.float64)
    fb = rs.rand(n_freqs, n_mels).astype(np.float32).astype(np.float64)
    if zero_column:
        fb[:, n_mels // 2] = 0
    return spec, fb


# ---------------------------------------------------------------------------------------------------------------
# the kernel's contract, restated; with planted bugs
# ---------------------------------------------------------------------------------------------------------------
KERNEL_MUTANTS = ("imag_dropped", "magnitude", "last_bin_dropped", "last_mel_dropped", "frame_off_by_one", "not_transposed",
                  "log_without_eps")
PATH_MUTANTS = ("symmetric_hann", "odd_reflection", "sum_w_norm", "hop_plus", "hop_minus")


def mel_power(spec, fb, log_eps=None, mutant=None):
    """spec (rows, frames, n_freqs, 2), fb (n_freqs, n_mels), int64 or float64 -> (rows, n_mels, frames) in the operands' type
    (float64 with a log: log(float32(log_eps) + mel))"""
    re, im = spec[..., 0], spec[..., 1]
    if mutant == "imag_dropped":
        im = np.zeros_like(im)
    P = re * re + im * im
    if mutant == "magnitude":
        P = np.sqrt(P.astype(np.float64))
    if mutant == "last_bin_dropped":
        P, fb = P[..., :-1], fb[:-1]
    if mutant == "frame_off_by_one":
        P = np.concatenate([P[:, 1:], np.zeros_like(P[:, :1])], axis=1)
    mel = np.einsum("rmb,bj->rjm", P, fb)
    if mutant == "last_mel_dropped":
        mel[:, -1, :] = 0
    if mutant == "not_transposed":
        mel = np.ascontiguousarray(mel.transpose(0, 2, 1)).reshape(mel.shape)
    if log_eps is None:
        return mel
    eps = 0.0 if mutant == "log_without_eps" else float(np.float32(log_eps))
    with np.errstate(divide="ignore"):
        return np.log(eps + mel.astype(np.float64))


def rel_bound(n_freqs):
    """1.01 (n_freqs + 3) u: the relative error of the fp32 chain on non-negative terms (module docstring)"""
    return 1.01 * (n_freqs + 3) * U


def log_bound(ref_log, rho):
    """|log a^ - log a| for a^ = a (1 + t), |t| <= rho, plus the device logf's own error"""
    with np.errstate(divide="ignore", invalid="ignore"):
        shift = np.where(rho < 1, -np.log1p(-np.minimum(rho, 0.5)), np.inf)
    return shift + LOGF_REL * np.maximum(np.abs(ref_log), 1.0)


# ---------------------------------------------------------------------------------------------------------------
# torch.stft / torchaudio's MelSpectrogram by their documented rules, scalar by scalar
# ---------------------------------------------------------------------------------------------------------------
def hann(win_length, symmetric=False):
    """periodic (torch.hann_window's default) or, the mutant, symmetric"""
    d = win_length - 1 if symmetric else win_length
    return np.array([0.5 - 0.5 * math.cos(2 * math.pi * k / d) for k in range(win_length)])


def stft_matrix(n_fft, win_length=None, normalized=True, mutant=None):
    win_length = n_fft if win_length is None else win_length
    w = np.zeros(n_fft)
    left = (n_fft - win_length) // 2
    w[left:left + win_length] = hann(win_length, symmetric=mutant == "symmetric_hann")
    c = 1.0
    if normalized:
        c = sum(v for v in w) if mutant == "sum_w_norm" else math.sqrt(sum(v * v for v in w))
    n_freqs = n_fft // 2 + 1
    B = np.empty((n_fft, 2 * n_freqs))
    for k in range(n_fft):
        for b in range(n_freqs):
            ang = 2 * math.pi * ((b * k) % n_fft) / n_fft
            B[k, 2 * b] = w[k] * math.cos(ang) / c
            B[k, 2 * b + 1] = -w[k] * math.sin(ang) / c
    return B


def mel_filterbank(n_freqs, f_min, f_max, n_mels, sample_rate):
    def mel(f):
        return 2595.0 * math.log10(1.0 + f / 700.0)

    def hz(m):
        return 700.0 * (10.0 ** (m / 2595.0) - 1.0)
    all_freqs = np.linspace(0, sample_rate // 2, n_freqs)
    m_pts = np.linspace(mel(f_min), mel(f_max), n_mels + 2)
    f_pts = [hz(m) for m in m_pts]
    fb = np.empty((n_freqs, n_mels))
    for b in range(n_freqs):
        for j in range(n_mels):
            up = (all_freqs[b] - f_pts[j]) / (f_pts[j + 1] - f_pts[j])
            down = (f_pts[j + 2] - all_freqs[b]) / (f_pts[j + 2] - f_pts[j + 1])
            fb[b, j] = max(0.0, min(up, down))
    return fb, np.array(f_pts), all_freqs


def reflect_pad(x, p, odd=False):
    """torch's pad_mode="reflect": x[p], ..., x[1] | x | x[-2], ..., x[-1 - p]; odd=True is a mutant (the point reflection
    fir_filter uses)"""
    li, ri = x[..., p:0:-1], x[..., -2:-p - 2:-1]
    if odd:
        li, ri = 2 * x[..., :1] - li, 2 * x[..., -1:] - ri
    return np.concatenate([li, x, ri], axis=-1)


def stft_frames(x, n_fft, hop, mutant=None):
    """(rows, L) -> (padded rows, stride, frames) as the product hands them to the window GEMM; hop_plus / hop_minus stride wrong
    (the row zero-extended to what the frames then read)"""
    xp = reflect_pad(x, n_fft // 2, odd=mutant == "odd_reflection")
    frames = 1 + x.shape[-1] // hop
    s = hop + (mutant == "hop_plus") - (mutant == "hop_minus")
    need = (frames - 1) * s + n_fft
    if need > xp.shape[1]:
        xp = np.concatenate([xp, np.zeros((xp.shape[0], need - xp.shape[1]))], axis=1)
    return xp, s, frames


def stft(x, B, n_fft, hop, mutant=None):
    """(rows, L) float64, B (n_fft, 2 n_freqs) -> (rows, frames, n_freqs, 2)"""
    xp, s, frames = stft_frames(x, n_fft, hop, mutant)
    return SC.window_gemm(xp, B, s, frames).reshape(x.shape[0], frames, n_fft // 2 + 1, 2)


def e2e(x, B, fb, n_fft, hop, log_eps=EPS, mutant=None):
    """The whole path in float64 on x (rows, L) and the matrices as given (the tests pass the fp32-rounded ones the product
    uploads), with the error budget of the module docstring.  Returns a dict: spec / spec_lim (rows, frames, n_freqs, 2),
    mel / mel_lim and logmel / logmel_lim (rows, n_mels, frames)."""
    spec = stft(x, B, n_fft, hop, mutant)
    xp, s, frames = stft_frames(x, n_fft, hop, mutant)
    d = SC.bound(xp, B, s, frames, K=n_fft).reshape(spec.shape)
    re, im, dre, dim = np.abs(spec[..., 0]), np.abs(spec[..., 1]), d[..., 0], d[..., 1]
    dP = 2 * (re * dre + im * dim) + dre * dre + dim * dim
    mel = mel_power(spec, fb)
    carried = np.einsum("rmb,bj->rjm", dP, fb)
    mel_lim = carried + rel_bound(fb.shape[0]) * (mel + carried)
    eps = float(np.float32(log_eps))
    with np.errstate(divide="ignore", invalid="ignore"):
        logmel = np.log(eps + mel)
        rho = mel_lim / (eps + mel) + U
    return {"spec": spec, "spec_lim": d, "mel": mel, "mel_lim": mel_lim, "logmel": logmel, "logmel_lim": log_bound(logmel, rho),
            "rho": rho}


def e2e_matrices(params, mutant=None):
    """fp32-rounded (B, fb) of a parameter set, from the scalar restatements"""
    n_fft, sr, n_mels = params["n_fft"], params["sample_rate"], params["n_mels"]
    B = stft_matrix(n_fft, mutant=mutant)
    fb = mel_filterbank(n_fft // 2 + 1, 0.0, float(sr // 2), n_mels, sr)[0]
    return B.astype(np.float32).astype(np.float64), fb.astype(np.float32).astype(np.float64)


def audio(L, rows=2):
    """seeded dyadic audio: fp32-exact, and so is its reflection"""
    return SC.dyadic((rows, L), L)


def miss(got, ref, lim):
    """max over the outputs of |got - ref| / lim (0 where both vanish, inf where only the bound does)"""
    err = np.abs(got - ref)
    with np.errstate(divide="ignore", invalid="ignore"):
        q = np.where(err == 0, 0.0, err / lim)
    q = np.where(np.isnan(err), np.inf, q)
    return float(q.max())
