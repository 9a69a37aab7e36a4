"""Shared inputs and yardsticks of the class-level decoding tests (test_class_decode_cpu.py, test_class_decode_gpu.py).

Three things live here, all numpy, none of them touching the device:

1. the cases: a small synthetic score matrix with every awkward class shape, one larger Zipf-like geometry, and the seeded
   segments of the whole-path tests;
2. `class_values64`, the float64 reference of what sda_retrieval_class_reduce / sda_retrieval_pool_rows compute, and
   `emulate_reduce` / `emulate_pool`, an fp32 emulation of the kernels' arithmetic IN THEIR SUMMATION ORDER (and, on request,
   with one of the planted bugs the CPU suite must see);
3. `value_bound`, the error bound of the fp32 result against the float64 reference, derived below.

The bound.  u = 2^-24 is fp32's unit roundoff.  The reference takes the fp32 cosine and the fp32 scale, widened, as exact, so
what is bounded is the arithmetic after the cosine.  First order in u throughout; the "+ 1" in every constant pays for the
second-order terms.  For one class c of row i, with n members, reduced by w lanes (w = 8 for n <= 256, w = 1024 above) in a
tree of depth d (3 for the xor tree 4, 2, 1; 6 + 15 for the xor tree inside a wave followed by the 16 waves in order):

  a. l^ = fl(scale * cos): |l^ - l| <= u |l| <= u Lc, Lc = max_{j in c} |l_j|.  log-sum-exp and max are 1-Lipschitz in the
     sup norm, so this moves f by at most u Lc.  ("max" ends here: f = max l^ is otherwise exact.)
  b. x^ = fl(l^ - m): relative error u; e^ = expf(x^) with at most 1 ulp = 2u relative error.  A term's relative error
     u |x| + 2u enters f weighted by p_j = e_j / sum_j e_j, and sum_j p_j |x_j| <= H(p) <= log n: together (log n + 2) u.
  c. the sum of positive terms, ceil(n / w) per lane in order and then the tree: relative error (ceil(n / w) - 1 + d) u,
     which is the absolute error of its logarithm; logf itself adds 1 ulp of log s <= log n: 2u log n.
  d. f^ = fl(m + log s): u |f|.
  => |f^_sum - f_sum| <= u (Lc + |f| + ceil(n / w) + d + 3 log n + 2)                                      =: B_sum(c)
     "mean" subtracts fl(log n) (1 ulp: 2u log n) and rounds once more:  B_mean = B_sum + u (2 log n + |f_mean|)
     "max":  B_max = u Lc
  e. LSE_i is the same reduction over the C "sum" values with w = 1024.  Their errors move it by at most sum_c P_c B_sum(c)
     (P_c = the class's probability: the derivative of log-sum-exp), and its own arithmetic adds, as in b-d with n := C,
     u (|LSE| + ceil(C / 1024) + 21 + 3 log C + 2)                                                          =: B_lse(i)
  f. value = fl(f^ - LSE^): B_value = B_mode(c) + B_lse(i) + u |value|.
  g. pooling a group of g rows, rows in order (w = 1, d = 0): log-mean-exp is 1-Lipschitz, so the inputs' errors enter by at
     most their maximum over the group's rows; its own arithmetic (b-d with n := g, then fl(log g) and one more rounding)
     adds u ((g - 1) + 5 log g + 2 + |res| + log g + |res|):
     B_pool = max_{r in g} B_value(r, c) + u (g + 6 log g + 2 |res| + 1).

The dominant term at the loss's temperature is a, the rounding of scale * cos.  The CPU suite checks the emulation against
this bound on every case and reports how much of it the emulation uses (worst case here: 0.49 of it, at scale = exp(5.1), so the bound has
about 2x slack over the emulation; the GPU's expf / logf are allowed the same 1 ulp as numpy's).
"""
import numpy as np

U = 2.0 ** -24
W_SMALL, W_BIG, BIG = 8, 1024, 256          # lanes per class, threads per workgroup, the size above which a class goes to the latter
SCALES = (1.0, float(np.float32(np.exp(np.float32(5.1)))), 1000.0)
MODES = ("sum", "mean", "max")


def pad64(x):
    return (x + 63) // 64 * 64


# ---------------------------------------------------------------------------------------------------------------------------
# index and layout helpers
# ---------------------------------------------------------------------------------------------------------------------------
def csr(ids, C):
    ids = np.asarray(ids, dtype=np.int64)
    order = np.argsort(ids, kind="stable").astype(np.int32)
    counts = np.bincount(ids, minlength=C)
    return order, np.concatenate([[0], np.cumsum(counts)]).astype(np.int32)


def chunk_major(S, chunk_cols, fill=np.nan):
    """The layout one GEMM per bank chunk leaves: chunk c = [n][pad64(its columns)] at float offset c * n * chunk_cols."""
    n, M = S.shape
    parts = []
    for c0 in range(0, M, chunk_cols):
        m = min(chunk_cols, M - c0)
        blk = np.full((n, pad64(m)), fill, dtype=np.float32)
        blk[:, :m] = S[:, c0: c0 + m]
        parts.append(blk.reshape(-1))
    return np.concatenate(parts)


def read_scores(flat, n, M, chunk_cols, wrong_last_pitch=False):
    """(n, M) dots back out of the chunk-major buffer, by the kernel's address arithmetic."""
    j = np.arange(M)
    c = j // chunk_cols
    rem = M - c * chunk_cols
    pitch = np.where(rem >= chunk_cols, chunk_cols, pad64(rem))
    if wrong_last_pitch:
        pitch = np.full_like(pitch, chunk_cols)
    addr = c[None, :] * n * chunk_cols + np.arange(n)[:, None] * pitch[None, :] + (j - c * chunk_cols)[None, :]
    return flat[np.minimum(addr, flat.size - 1)]


def cosine32(S, qsq, csq):
    """fp32, the kernel's formula: S / max(sqrt(qsq) sqrt(csq), 1e-8), -0 -> +0."""
    den = np.maximum(np.sqrt(qsq.astype(np.float32))[:, None] * np.sqrt(csq.astype(np.float32))[None, :], np.float32(1e-8))
    return (S.astype(np.float32) / den + np.float32(0.0)).astype(np.float32)


# ---------------------------------------------------------------------------------------------------------------------------
# float64 reference
# ---------------------------------------------------------------------------------------------------------------------------
def _segments(order, offsets):
    counts = np.diff(offsets.astype(np.int64))
    return counts, np.flatnonzero(counts > 0)


def class_stats64(cos, order, offsets, scale):
    """float64 per (row, class): m (maximum logit), fsum (log-sum-exp), Lc (largest |logit|); and the row's LSE over all
    logits.  cos: the fp32 cosine (n, M); scale: the fp32 scale.  Empty classes: m = fsum = -inf, Lc = 0."""
    counts, full = _segments(order, offsets)
    lg = np.float64(np.float32(scale)) * cos.astype(np.float64)[:, order.astype(np.int64)]
    n, C = cos.shape[0], counts.size
    starts = offsets[full].astype(np.int64)
    m = np.full((n, C), -np.inf)
    fsum = np.full((n, C), -np.inf)
    Lc = np.zeros((n, C))
    m[:, full] = np.maximum.reduceat(lg, starts, axis=1)
    Lc[:, full] = np.maximum.reduceat(np.abs(lg), starts, axis=1)
    fsum[:, full] = m[:, full] + np.log(np.add.reduceat(np.exp(lg - np.repeat(m[:, full], counts[full], axis=1)), starts, axis=1))
    top = lg.max(axis=1, keepdims=True)
    lse = (top + np.log(np.exp(lg - top).sum(axis=1, keepdims=True)))[:, 0]
    return m, fsum, Lc, lse, counts


def pool64(values, groups):
    """log mean exp over the rows of every group, float64; a column -inf in every row stays -inf."""
    groups = np.asarray(groups)
    out = np.full((int(groups.max()) + 1, values.shape[1]), -np.inf)
    for g in range(out.shape[0]):
        v = values[groups == g]
        m = v.max(axis=0)
        ok = m > -np.inf
        out[g, ok] = m[ok] + np.log(np.exp(v[:, ok] - m[ok]).sum(axis=0)) - np.log(v.shape[0])
    return out


def class_values64(cos, order, offsets, scale, mode="sum", groups=None):
    """The float64 reference: (values (R, C), row_lse (n,)); R = n, or the number of groups."""
    m, fsum, _, lse, counts = class_stats64(cos, order, offsets, scale)
    with np.errstate(divide="ignore", invalid="ignore"):
        f = {"sum": fsum, "max": m, "mean": np.where(counts > 0, fsum - np.log(np.maximum(counts, 1)), -np.inf)}[mode]
    values = f - lse[:, None]
    return (values if groups is None else pool64(values, groups)), lse


# ---------------------------------------------------------------------------------------------------------------------------
# the bound
# ---------------------------------------------------------------------------------------------------------------------------
def value_bound(cos, order, offsets, scale, mode="sum", groups=None):
    """(bound on |value - float64 value| (R, C), bound on |row_lse - float64 LSE| (n,)): B_value / B_pool and B_lse of the
    module docstring.  Entries of empty classes (value -inf) carry 0: they must be -inf exactly."""
    m, fsum, Lc, lse, counts = class_stats64(cos, order, offsets, scale)
    C = counts.size
    nz = np.maximum(counts, 1).astype(np.float64)
    w = np.where(counts <= BIG, W_SMALL, W_BIG)
    d = np.where(counts <= BIG, 3, 21)
    has = counts > 0
    fs = np.where(has, fsum, 0.0)
    b_sum = U * (Lc + np.abs(fs) + np.ceil(nz / w) + d + 3 * np.log(nz) + 2) * has
    P = np.exp(fsum - lse[:, None])
    b_lse = (P * b_sum).sum(axis=1) + U * (np.abs(lse) + np.ceil(C / W_BIG) + 21 + 3 * np.log(C) + 2)
    values, _ = class_values64(cos, order, offsets, scale, mode)
    vs = np.where(has, values, 0.0)
    if mode == "sum":
        b_mode = b_sum
    elif mode == "mean":
        b_mode = b_sum + U * (2 * np.log(nz) + np.abs(fs - np.log(nz))) * has
    else:
        b_mode = U * Lc
    b_val = (b_mode + b_lse[:, None] + U * np.abs(vs)) * has
    if groups is None:
        return b_val, b_lse
    groups = np.asarray(groups)
    pooled = pool64(values, groups)
    ps = np.where(has, pooled, 0.0)
    out = np.zeros_like(pooled)
    for g in range(pooled.shape[0]):
        rows = groups == g
        k = float(rows.sum())
        out[g] = (b_val[rows].max(axis=0) + U * (k + 6 * np.log(k) + 2 * np.abs(ps[g]) + 1)) * has
    return out, b_lse


def miss(got, want, bound):
    """max |got - want| / bound over the finite entries of `want`; inf when `got` has a NaN, or is not -inf exactly where `want`
    is -inf (and only there)."""
    got = np.asarray(got, dtype=np.float64)
    fin = np.isfinite(want)
    if np.isnan(got).any() or not np.array_equal(np.isneginf(got), np.isneginf(want)) or not np.isfinite(got[fin]).all():
        return np.inf
    if not fin.any():
        return 0.0
    return float((np.abs(got[fin] - want[fin]) / bound[fin]).max())


# ---------------------------------------------------------------------------------------------------------------------------
# fp32 emulation of the kernels, in their summation order
# ---------------------------------------------------------------------------------------------------------------------------
def _xor_tree(v, lanes, op):
    idx = np.arange(lanes)
    off = lanes // 2
    while off:
        v = op(v, v[..., idx ^ off])
        off //= 2
    return v


def _lane_reduce(terms, w, op, init):
    """terms (n, cnt) -> (n,): lane a of w takes terms a, a + w, ... in order; then, w = 8: the xor tree 4, 2, 1; w = 1024: the
    xor tree 32 ... 1 inside each wave of 64 and the 16 waves in order.  fp32 throughout."""
    n, cnt = terms.shape
    steps = max(1, -(-cnt // w))
    padded = np.full((n, steps * w), init, dtype=np.float32)
    padded[:, :cnt] = terms
    padded = padded.reshape(n, steps, w)
    acc = padded[:, 0].copy()
    for s in range(1, steps):
        acc = op(acc, padded[:, s])
    if w == W_SMALL:
        return _xor_tree(acc, w, op)[:, 0]
    waves = _xor_tree(acc.reshape(n, w // 64, 64), 64, op)[:, :, 0]
    tot = waves[:, 0].copy()
    for k in range(1, w // 64):
        tot = op(tot, waves[:, k])
    return tot


def _lse32(l, w):
    """(m, m + log sum exp(l - m)) of every row of l (n, cnt) fp32 in the kernel's order for w lanes."""
    m = _lane_reduce(l, w, np.maximum, np.float32(-np.inf))
    with np.errstate(invalid="ignore"):
        e = np.exp((l - m[:, None]).astype(np.float32)).astype(np.float32)
    s = _lane_reduce(e, w, np.add, np.float32(0.0))
    with np.errstate(divide="ignore"):
        return m, (m + np.log(s).astype(np.float32)).astype(np.float32)


def emulate_reduce(flat, qsq, csq, order, offsets, n, M, chunk_cols, scale, mode="sum", bug=None):
    """fp32 emulation of sda_retrieval_class_reduce on the chunk-major buffer `flat` -> (values (n, C), row_lse (n,)).
    bug: None, or one of 'row_max', 'no_scale', 'mean_no_logn', 'drop_last', 'take_next', 'order_ignored', 'last_pitch'."""
    cos = cosine32(read_scores(flat, n, M, chunk_cols, wrong_last_pitch=bug == "last_pitch"), qsq, csq)
    sc = np.float32(1.0 if bug == "no_scale" else scale)
    C = offsets.size - 1
    logit = (sc * cos).astype(np.float32)
    rowmax = logit.max(axis=1)
    fsum = np.full((n, C), -np.inf, dtype=np.float32)
    fmax = np.full((n, C), -np.inf, dtype=np.float32)
    for c in range(C):
        lo, hi = int(offsets[c]), int(offsets[c + 1])
        cnt = hi - lo                                   # the path a class takes depends on its true size
        if bug == "drop_last":
            hi -= 1
        if bug == "take_next":
            hi = min(hi + 1, M)
        if hi <= lo:
            continue
        members = np.arange(lo, hi) if bug == "order_ignored" else order[lo:hi].astype(np.int64)
        l = logit[:, members]
        w = W_SMALL if cnt <= BIG else W_BIG
        if bug == "row_max":
            with np.errstate(divide="ignore"):
                e = np.exp((l - rowmax[:, None]).astype(np.float32)).astype(np.float32)
                fmax[:, c] = _lane_reduce(l, w, np.maximum, np.float32(-np.inf))
                fsum[:, c] = (rowmax + np.log(_lane_reduce(e, w, np.add, np.float32(0.0))).astype(np.float32)).astype(np.float32)
        else:
            fmax[:, c], fsum[:, c] = _lse32(l, w)
    F, lse = _lse32(fsum, W_BIG)
    counts = np.diff(offsets).astype(np.int64)
    if mode == "sum":
        f = fsum
    elif mode == "max":
        f = fmax
    else:
        logn = np.zeros(C, dtype=np.float32) if bug == "mean_no_logn" else np.log(np.maximum(counts, 1).astype(np.float32)).astype(np.float32)
        f = np.where(counts > 0, (fsum - logn[None, :]).astype(np.float32), np.float32(-np.inf)).astype(np.float32)
    return (f - lse[:, None]).astype(np.float32), lse


def emulate_pool(values, groups, bug=None):
    """fp32 emulation of sda_retrieval_pool_rows (rows of a group in ascending order).  bug: None, 'arith_mean', 'nan_on_empty'."""
    groups = np.asarray(groups)
    G = int(groups.max()) + 1
    out = np.full((G, values.shape[1]), -np.inf, dtype=np.float32)
    for g in range(G):
        v = values[groups == g].astype(np.float32)
        if bug == "arith_mean":
            with np.errstate(invalid="ignore"):
                out[g] = v.astype(np.float64).mean(axis=0).astype(np.float32)
            continue
        m = v.max(axis=0)
        s = np.zeros_like(m)
        with np.errstate(invalid="ignore", divide="ignore"):
            for r in range(v.shape[0]):
                s = (s + np.exp((v[r] - m).astype(np.float32)).astype(np.float32)).astype(np.float32)
            res = ((m + np.log(s).astype(np.float32)).astype(np.float32) - np.log(np.float32(v.shape[0]))).astype(np.float32)
        out[g] = res if bug == "nan_on_empty" else np.where(m > -np.inf, res, np.float32(-np.inf))
    return out


# ---------------------------------------------------------------------------------------------------------------------------
# the cases
# ---------------------------------------------------------------------------------------------------------------------------
_cache = {}


def small_case():
    """n = 5, M = 1000, C = 37: classes 5 and 20 empty, 1-3 and 36 singletons, class 0 with 600 members spread over the whole
    bank (the workgroup's path), class 4 with 100 (more than a group keeps in registers), the rest random.  Row 0 has zero
    norm, row 1 the same cosine (exactly 0.5) everywhere but at the zero-norm candidate 7.  Norms are powers of two."""
    if "small" not in _cache:
        rng = np.random.default_rng(20251019)
        n, M, C = 5, 1000, 37
        perm = rng.permutation(M)
        ids = np.empty(M, dtype=np.int64)
        ids[perm[:600]] = 0
        ids[perm[600:700]] = 4
        for t, c in enumerate((1, 2, 3, 36)):
            ids[perm[700 + t]] = c
        rest = [c for c in range(C) if c not in (0, 1, 2, 3, 4, 5, 20, 36)]
        tail = perm[704:]
        ids[tail[: len(rest)]] = rest                                  # every remaining class has a member
        ids[tail[len(rest):]] = rng.choice(rest, size=tail.size - len(rest))
        csq = (4.0 ** rng.integers(-1, 2, size=M)).astype(np.float32)
        qsq = (4.0 ** rng.integers(0, 2, size=n)).astype(np.float32)
        cos = rng.uniform(-1.0, 1.0, size=(n, M)).astype(np.float32)
        cos[1] = 0.5
        S = (cos * np.sqrt(qsq)[:, None] * np.sqrt(csq)[None, :]).astype(np.float32)
        S[0] = 0.0; qsq[0] = 0.0
        S[:, 7] = 0.0; csq[7] = 0.0
        order, offsets = csr(ids, C)
        _cache["small"] = dict(n=n, M=M, C=C, ids=ids, order=order, offsets=offsets, S=S, qsq=qsq, csq=csq,
                               cos=cosine32(S, qsq, csq), chunks=(256, 384, 1024))
    return _cache["small"]


def large_case():
    """n = 8, M = 20000, C = 3000, Zipf-like counts: class 0 has 4200 members (several per thread of the workgroup), class 1
    about 1500, classes 2 ... 5 between 256 and 1024, the tail singletons; three chunks of 8192 columns, the last 3616 wide."""
    if "large" not in _cache:
        rng = np.random.default_rng(77)
        n, M, C = 8, 20000, 3000
        wgt = 1.0 / np.arange(1, C)
        counts = np.concatenate([[4200], 1 + np.floor(wgt * (M - 4200 - (C - 1)) / wgt.sum()).astype(np.int64)])
        counts[1] += M - counts.sum()
        ids = np.repeat(np.arange(C), counts)[rng.permutation(M)]
        cos = rng.uniform(-0.4, 1.0, size=(n, M)).astype(np.float32)
        S, qsq, csq = cos.copy(), np.ones(n, dtype=np.float32), np.ones(M, dtype=np.float32)
        order, offsets = csr(ids, C)
        _cache["large"] = dict(n=n, M=M, C=C, ids=ids, order=order, offsets=offsets, S=S, qsq=qsq, csq=csq,
                               cos=cosine32(S, qsq, csq), chunks=(8192,))
    return _cache["large"]


SHAPES = {"a": (96, 1000, 64, 90), "b": (40, 300, 24, 50)}


def path_case(shape):
    """Seeded segments of a whole-path test: bank (M, F, T), class ids (skewed, some classes empty), labels (bank rows) and the
    queries planted on them as 0.35 * bank[label] + noise; groups of sizes 1, 2 and 7, interleaved over the queries."""
    if shape not in _cache:
        import torch
        N, M, F, T = SHAPES[shape]
        g = torch.Generator().manual_seed(4321 + 13 * N + M)
        bank = torch.randn(M, F, T, generator=g)
        labels = torch.randint(M, (N,), generator=g)
        queries = 0.35 * bank[labels] + torch.randn(N, F, T, generator=g)
        rng = np.random.default_rng(N + M)
        C = M // 3
        ids = np.minimum((C * rng.random(M) ** 2).astype(np.int64), C - 2)          # class C - 1 is empty, and some others
        _cache[shape] = dict(N=N, M=M, F=F, T=T, C=C, bank=bank, labels=labels, queries=queries, ids=ids)
    return _cache[shape]


def cosine64_of(queries, bank, torch_dtype):
    """The fp32 cosine the whole path is held to, from float64 on the operands rounded to the bank's dtype."""
    import torch
    q = queries.to(torch_dtype).double().reshape(queries.shape[0], -1)
    c = bank.to(torch_dtype).double().reshape(bank.shape[0], -1)
    den = torch.clamp(q.norm(dim=-1)[:, None] * c.norm(dim=-1)[None, :], min=1e-8)
    return ((q @ c.T) / den).numpy()
