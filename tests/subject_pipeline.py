"""NumPy restatement of the Brennan2018 input pipeline (brennan2018.py:72-152) in the arithmetic the kernels use: exact
order statistics of the float32 row, position and fraction in float64, one float32 `a + (b - a) * g`, float32 `(x - c) / s`,
clamp, segmentation, float32 baseline mean.  Pinned on tests/golden/brennan.npz (produced by the reference's own functions,
sklearn's RobustScaler included) by tests/test_subject_feed_cpu.py; the GPU tests use it at other shapes."""
import numpy as np

F32 = np.float32


def quantile_linear(sorted_row: np.ndarray, q: float) -> np.float32:
    """numpy's "linear" rule on an ascending float32 row, interpolated in float32."""
    n = len(sorted_row)
    pos = q * (n - 1)                                   # float64
    i0 = int(np.floor(pos))
    g = F32(pos - i0)
    a, b = F32(sorted_row[i0]), F32(sorted_row[min(i0 + 1, n - 1)])
    return a if g == 0 else F32(a + F32(F32(b - a) * g))


def robust_stats_rows(rows: np.ndarray):
    """rows (R, N) float32 -> (centre, scale) float32 (R,): median, 75th - 25th percentile, zero scale -> 1."""
    rows = np.asarray(rows, dtype=F32)
    centre, scale = np.empty(len(rows), F32), np.empty(len(rows), F32)
    for r, row in enumerate(rows):
        s = np.sort(row)
        centre[r] = quantile_linear(s, 0.5)
        iqr = F32(quantile_linear(s, 0.75) - quantile_linear(s, 0.25))
        scale[r] = F32(1.0) if iqr == 0 else iqr
    return centre, scale


def pooled_rows(X: np.ndarray) -> np.ndarray:
    """(S, C, L) -> (C, S * L): every subject's samples of a channel in one row (brennan2018.py:129)."""
    S, C, L = X.shape
    return np.ascontiguousarray(np.transpose(X, (1, 0, 2))).reshape(C, S * L)


def robust_stats(X: np.ndarray, subject_wise: bool):
    """X (S, C, L) -> (centre, scale) of shape (S, C), or (C,) pooled."""
    S, C, L = X.shape
    if subject_wise:
        c, s = robust_stats_rows(X.reshape(S * C, L))
        return c.reshape(S, C), s.reshape(S, C)
    return robust_stats_rows(pooled_rows(X))


def scale_clamp(X: np.ndarray, centre: np.ndarray, scale: np.ndarray, clamp_lim: float, clamp: bool) -> np.ndarray:
    """(X - centre) / scale in float32; centre / scale (S, C) or (C,)."""
    X = np.asarray(X, dtype=F32)
    c = centre[..., None] if centre.ndim == 2 else centre[None, :, None]
    s = scale[..., None] if scale.ndim == 2 else scale[None, :, None]
    out = ((X - c.astype(F32)) / s.astype(F32)).astype(F32)
    return np.clip(out, F32(-clamp_lim), F32(clamp_lim)) if clamp else out


def baseline_windows(Xs: np.ndarray, subjects, starts, T: int, nb: int) -> np.ndarray:
    """Xs (S, C, L) -> (B, C, T): window minus the float32 mean of its first nb samples (nb = 0: the window itself)."""
    out = np.stack([Xs[s, :, o: o + T] for s, o in zip(subjects, starts)]).astype(F32)
    if nb > 0:
        out = out - out[..., :nb].astype(np.float64).mean(axis=-1, keepdims=True).astype(F32)
    return out.astype(F32)


def geometry(length: int, srate: float, seq_len_sec: float, baseline_len_sec: float, shift_ms: float = 150):
    """(shift, seq_len_samp, baseline_len_samp, trim_len, num_segments) of brennan2018.py:83-92,296."""
    shift = int(srate * (shift_ms / 1000))
    seq = int(seq_len_sec * srate)
    nb = int(seq * baseline_len_sec / seq_len_sec)
    trim = ((length - shift) // seq) * seq
    return shift, seq, nb, trim, trim // seq


def pipeline(X, Y, *, srate, seq_len_sec, baseline_len_sec, clamp_lim, clamp=True, subject_wise=True, shift_ms=150, segment_len=None):
    """-> (X segments (n, S, C, seg), Y segments (n, F, seg)) as the reference's dataset holds them."""
    X, Y = np.asarray(X, dtype=F32), np.asarray(Y, dtype=F32)
    shift, seq, nb, trim, _ = geometry(X.shape[-1], srate, seq_len_sec, baseline_len_sec, shift_ms)
    seg = seq if segment_len is None else int(segment_len)
    assert trim % seg == 0
    Xs = X[..., shift: shift + trim]
    Ys = Y[:, :trim]
    centre, scale = robust_stats(Xs, subject_wise)
    Xs = scale_clamp(Xs, centre, scale, clamp_lim, clamp)
    n, S = trim // seg, X.shape[0]
    segX = np.stack([baseline_windows(Xs, range(S), [i * seg] * S, seg, nb) for i in range(n)])
    segY = np.stack([Ys[:, i * seg: (i + 1) * seg] for i in range(n)])
    return segX, segY
