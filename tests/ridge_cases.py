"""Shared cases and the float64 reference of the time-lagged ridge baseline (speech_decoding_amd/ridge.py, csrc/lagged_cov.hip),
written from the estimator's formulas:

    yhat_b(t) = ybar + sum_l W_l^T x_b(t + l),  every segment zero outside [0, T) in x and y - ybar
    A_d[i][j] = sum_b sum_u x_b[u + d, i] x_b[u, j]       R_l[c][f] = sum_b sum_t x_b[t + l, c] y_b[t, f]
    s_l[c] = sum_b sum_{u >= l} x_b[u, c]                 n = B T,  ybar = sum y / n
    G[(l, c), (l', c')] = A_{l - l'}[c][c'] (l >= l'), transposed otherwise;   (G + alpha I) W = R - s ybar^T

and the kernel's contract out[s][d][i][j] = sum_{r in slice s} a[r + d][i] b[r][j] on the lag layout.  numpy only."""
import numpy as np

U = 2.0 ** -24
TILE, GROUP, CHUNK, MIN_SLICE, TARGET_WGS = 64, 8, 64, 256, 1024          # csrc/lagged_cov.hip's LC_* constants

# (B, C, F, T, L, why) — H = L - 1 exactly in every case
KERNEL_CASES = [
    (1, 5, 7, 37, 1, "one lag: the plain Gram matrix, one sample"),
    (3, 5, 7, 37, 6, "a lag group's tail (6 of 8), one partial chunk"),
    (3, 5, 130, 37, 9, "one full lag group + 1, Fp = 192: three column tiles"),
    (1, 70, 7, 37, 17, "two full lag groups + 1, Cp = 128: two channel tiles, the d > 0 blocks are not symmetric"),
    (3, 70, 130, 37, 6, "both operands wider than a tile"),
    (5, 5, 7, 211, 6, "rows exceed one row slice and are no multiple of the chunk"),
    (5, 70, 7, 211, 9, "several slices x two channel tiles x two lag groups"),
]
ALPHAS = (1e-3, 1.0, 100.0)


def pad64(c):
    return (c + TILE - 1) // TILE * TILE


def ints(shape, R, seed):
    return np.random.RandomState(seed).randint(-R, R + 1, size=shape).astype(np.int64)


def gamma(m):
    return m * U / (1.0 - m * U)


# ------------------------------------------------------------------------------------------------------ the kernel
def lag_layout(X, H, Cp=None):
    """(B, C, T) -> (B (T + H), Cp): segment b in rows b (T + H) ... + T - 1, channels-last, everything else zero"""
    B, C, T = X.shape
    Cp = pad64(C) if Cp is None else Cp
    out = np.zeros((B, T + H, Cp), dtype=X.dtype)
    out[:, :T, :C] = X.transpose(0, 2, 1)
    return out.reshape(B * (T + H), Cp)


def slice_rule(rows, L, Ap, Bp):
    """(slices, slice length): the shape-only rule of sda_lagged_cov_slices"""
    units = (Ap // TILE) * (Bp // TILE) * ((L + GROUP - 1) // GROUP)
    by_rows = (rows + MIN_SLICE - 1) // MIN_SLICE
    n = max(1, min((TARGET_WGS + units - 1) // units, by_rows))
    length = ((rows + n - 1) // n + CHUNK - 1) // CHUNK * CHUNK
    return (rows + length - 1) // length, length


def lagged_cov(a, b, L):
    """out[d][i][j] = sum_r a[r + d][i] b[r][j] over the whole row space, rows >= len(a) zero; in the operands' own type"""
    rows = a.shape[0]
    return np.stack([a[d:].T @ b[:rows - d] if d < rows else np.zeros((a.shape[1], b.shape[1]), a.dtype) for d in range(L)])


def cov_bound(a, b, L, slabs):
    """gamma_m sum_r |a[r + d][i] b[r][j]| per entry, m = rows contracted + slabs: the bound of ANY order of summation"""
    return gamma(a.shape[0] + slabs) * lagged_cov(np.abs(a).astype(np.float64), np.abs(b).astype(np.float64), L)


KERNEL_MUTANTS = ("transposed_blocks", "minus_lag", "reads_past_end", "no_partial_chunk", "group_tail_dropped")


def emulate(a, b, L, mutant=None):
    """The kernel in fp32 arithmetic: per row slice a chain fl(acc + a[r + d][i] b[r][j]) in row order (the product of two fp32
    numbers is exact in float64, so each step is one fused multiply-add up to double rounding), the slabs then summed in
    float64.  a, b: fp32 lag-layout arrays.  `mutant` plants one of KERNEL_MUTANTS.  (A row past the end only ever meets a zero row
    of b, H >= L - 1 sees to that: reading it is a memory fault or, over non-finite bytes, 0 x NaN; the mutant reads NaN there.)"""
    rows, (Ap, Bp) = a.shape[0], (a.shape[1], b.shape[1])
    n, length = slice_rule(rows, L, pad64(Ap), pad64(Bp))
    a64, b64 = a.astype(np.float64), b.astype(np.float64)
    lags = L // GROUP * GROUP if mutant == "group_tail_dropped" else L
    total = np.zeros((L, Ap, Bp))
    for s in range(n):
        r0, r1 = s * length, min(rows, (s + 1) * length)
        if mutant == "no_partial_chunk":
            r1 = r0 + (r1 - r0) // CHUNK * CHUNK
        acc = np.zeros((L, Ap, Bp), dtype=np.float32)
        for r in range(r0, r1):
            for d in range(lags):
                q = r - d if mutant == "minus_lag" else r + d
                if mutant == "reads_past_end" and q >= rows:         # what lies behind the buffer is not zero: NaN here
                    acc[d] = acc[d] + np.float32(np.nan) * b[r][None, :]
                elif 0 <= q < rows:
                    acc[d] = (acc[d].astype(np.float64) + np.outer(a64[q], b64[r])).astype(np.float32)
        total += acc
    if mutant == "transposed_blocks":
        total[1:] = total[1:].transpose(0, 2, 1)
    return total


# ---------------------------------------------------------------------------------------------------- the estimator
def moments(X, Y, L, mutant=None):
    """(A (L, C, C), R (L, C, F), s (L, C), sum y (F,), n) of float64 segments X (B, C, T), Y (B, F, T)"""
    B, C, T = X.shape
    A = np.zeros((L, C, C))
    R = np.zeros((L, C, Y.shape[1]))
    s = np.zeros((L, C))
    for d in range(min(L, T)):
        A[d] = np.einsum("biu,bju->ij", X[:, :, d:], X[:, :, :T - d])
        R[d] = np.einsum("bcu,bfu->cf", X[:, :, d:], Y[:, :, :T - d])
        s[d] = X[:, :, 0 if mutant == "s_without_head" else d:].sum(axis=(0, 2))
    n = B * (T + L - 1) if mutant == "pad_rows_in_n" else B * T
    return A, R, s, Y.sum(axis=(0, 2)), n


ESTIMATOR_MUTANTS = ("pad_rows_in_n", "s_without_head")


def assemble(A):
    L, C, _ = A.shape
    G = np.zeros((L, C, L, C))
    for l in range(L):
        for m in range(L):
            G[l, :, m, :] = A[l - m] if l >= m else A[m - l].T
    return G.reshape(L * C, L * C)


def solve(A, R, s, sum_y, n, alphas):
    """(coef (n_alphas, L, C, F), ybar (F,)) in float64"""
    L, C, F = R.shape
    ybar = sum_y / n
    G, rhs = assemble(A), (R - s[:, :, None] * ybar[None, None, :]).reshape(L * C, F)
    return np.stack([np.linalg.solve(G + a * np.eye(L * C), rhs).reshape(L, C, F) for a in alphas]), ybar


def fit(X, Y, L, alphas, mutant=None):
    return solve(*moments(X, Y, L, mutant), alphas)


def predict(X, W, ybar):
    """yhat (B, F, T) = ybar + sum_l W_l^T x(t + l), x zero past T"""
    B, C, T = X.shape
    L, _, F = W.shape
    out = np.zeros((B, F, T)) + ybar[None, :, None]
    for l in range(min(L, T)):
        out[:, :, :T - l] += np.einsum("bcu,cf->bfu", X[:, :, l:], W[l])
    return out


def design(X, L):
    """The explicit zero-extended design matrix: one row per (b, t), t = -(L - 1) ... T - 1; column (l, c) = x_b[t + l, c]"""
    B, C, T = X.shape
    Xp = np.zeros((B, C, T + 2 * (L - 1)))
    Xp[:, :, L - 1:L - 1 + T] = X
    return np.array([np.stack([Xp[b, :, t + l + L - 1] for l in range(L)]).reshape(-1) for b in range(B) for t in range(-(L - 1), T)])


def target(Y, L, ybar):
    """(y - ybar) zero-extended to the design matrix's rows"""
    B, F, T = Y.shape
    Yp = np.zeros((B, T + L - 1, F))
    Yp[:, L - 1:, :] = (Y - ybar[None, :, None]).transpose(0, 2, 1)
    return Yp.reshape(-1, F)


def coef_bound(X, Y, L, alpha, slabs, W):
    """||coef - W||_F can be at most this when the products are summed in fp32 in any order and everything else is exact:
    from (M + dM)(W + dW) = r + dr with M = G + alpha I,
        ||dW||_F <= ||M^-1||_2 (||dr||_F + ||dM||_2 ||W||_F) / (1 - ||M^-1||_2 ||dM||_2)
    = kappa(M) x (the relative bounds of G and R), with |dG| <= gamma_m G(|x|, |x|) and |dr| <= gamma_m R(|x|, |y|) entry by
    entry and m = the rows contracted (B (T + L - 1)) + slabs.  X, Y: the fp32-rounded inputs as float64, W: the reference."""
    B, C, T = X.shape
    Aa, Ra, _, _, _ = moments(np.abs(X), np.abs(Y), L)
    g = gamma(B * (T + L - 1) + slabs)
    dM = np.linalg.norm(g * assemble(Aa), "fro")                 # >= the 2-norm
    dr = np.linalg.norm(g * Ra)
    A = moments(X, Y, L)[0]
    inv = 1.0 / np.linalg.eigvalsh(assemble(A) + alpha * np.eye(L * C))[0]
    assert inv * dM < 0.5
    return inv * (dr + dM * np.linalg.norm(W)) / (1.0 - inv * dM)


def planted_world(seed=1, n=64, C=5, F=7, T=37, L=6, noise=0.05, offset=3.0):
    """The end-to-end case: X ~ N(0, 1) rounded to fp32 with a silent head (the first L - 1 steps zero), Y = the planted lagged
    map of X + noise + feature offsets around `offset`.  (X, Y, W) in float64."""
    rng = np.random.default_rng(seed)
    W = np.random.default_rng(0).standard_normal((L, C, F))
    X = rng.standard_normal((n, C, T)).astype(np.float32).astype(np.float64)
    X[:, :, :L - 1] = 0
    Y = predict(X, W, np.zeros(F))
    Y += noise * rng.standard_normal(Y.shape)
    Y += (offset + rng.standard_normal(F))[None, :, None]
    return X, Y.astype(np.float32).astype(np.float64), W


def cosine_top1(P, Yc):
    """(top-1 accuracy of row i against candidate i, smallest margin best - second) of cosine scores over flattened segments"""
    q, c = P.reshape(len(P), -1), Yc.reshape(len(Yc), -1)
    S = (q / np.linalg.norm(q, axis=1, keepdims=True)) @ (c / np.linalg.norm(c, axis=1, keepdims=True)).T
    srt = np.sort(S, axis=1)
    return float((S.argmax(1) == np.arange(len(P))).mean()), float((srt[:, -1] - srt[:, -2]).min())
