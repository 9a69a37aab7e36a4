"""Shared inputs of the WindowBank tests (test_window_bank_cpu.py, test_window_bank_gpu.py) and a numpy restatement of what
retrieve() computes against a window bank.

The cases are small because the windowed similarity GEMM can go wrong only at tile, chunk and window edges:
    a: F = 40 (padded to 64), T = 24 (K = 1536: 48 K-steps, every K slice one or two of them), two tracks of 500 and 333 rows,
       M = 600 windows (three 256-column tiles, the last ragged), N = 5 queries
    b: F = 128, T = 40, one track of 700 rows, M = 70 windows, N = 260 queries (two query tiles, the second ragged)
Every case's starts include 0 and L - T of every track, two adjacent starts s, s + 1 and one duplicate, in shuffled order;
queries are 2 * window[label] + noise.

Exact regime (`exact=True`): tracks and noise are integers in -3 ... 3, so every operand is exact in bf16 and fp16, every dot
product and squared norm an integer below 2^24 (test_window_bank_cpu.py checks the bound), and S, qsq, csq — hence every score
bit — the same in any summation order and under any K split.  Real regime: seeded normal values.

restate() follows the device path's index arithmetic on purpose (chunks of `mc` candidates, 256-column tiles inside a chunk,
the packed query rows behind ROW_PAD pad rows) so that the bugs that path can have can be planted in it: MUTANTS.
"""
import numpy as np

ROW_PAD = 16
TILE = 256
SHAPES = {"a": dict(F=40, T=24, tracks=(500, 333), M=600, N=5), "b": dict(F=128, T=40, tracks=(700,), M=70, N=260)}
MUTANTS = ("start_plus_1", "start_minus_1", "tile_offset_dropped", "chunk_offset_dropped", "regular_pitch", "k_one_row_short",
           "k_one_row_long", "norm_wrong_start", "norm_one_row_short", "norm_one_row_long", "query_pad_rows_included")

_cases = {}


def pad64(n):
    return (n + 63) // 64 * 64


def case(shape: str, exact: bool = True):
    """dict(F, T, tracks: list of (F, L) float32 arrays, local: per-track start arrays, starts: global table rows in bank order,
    table: (L_total, F) float64, queries (N, F, T) float32, labels (N,) int64); computed once, never written to."""
    key = (shape, exact)
    if key in _cases:
        return _cases[key]
    sh = SHAPES[shape]
    F, T, M, N = sh["F"], sh["T"], sh["M"], sh["N"]
    rng = np.random.RandomState(20260 + 7 * F + T + (0 if exact else 1))
    draw = (lambda *s: rng.randint(-3, 4, size=s).astype(np.float32)) if exact else (lambda *s: rng.randn(*s).astype(np.float32))
    tracks = [draw(F, Lt) for Lt in sh["tracks"]]
    # the candidates, dealt over the tracks in proportion to their length
    share = [M * Lt // sum(sh["tracks"]) for Lt in sh["tracks"]]
    share[0] += M - sum(share)
    local = []
    for Lt, m in zip(sh["tracks"], share):
        s = rng.randint(0, Lt - T + 1, size=m)
        s[:5] = (0, Lt - T, Lt // 3, Lt // 3 + 1, Lt // 3)         # both ends, two adjacent starts, one duplicate
        rng.shuffle(s)
        local.append(s.astype(np.int64))
    first = np.concatenate([[0], np.cumsum(sh["tracks"])])[:-1]
    starts = np.concatenate([s + r0 for s, r0 in zip(local, first)])
    table = np.concatenate([t.T for t in tracks]).astype(np.float64)          # (L_total, F): one row per time step
    labels = rng.randint(0, M, size=N).astype(np.int64)
    # labels in every 256-column tile, on a duplicate pair and on both ends of a track (a: M = 600; b: one tile)
    dup = np.flatnonzero(starts == first[0] + sh["tracks"][0] // 3)
    labels[:5] = (int(np.flatnonzero(starts == 0)[0]), M - 1, min(M - 1, 300), dup[0], dup[1])
    windows = windows_of(table, starts, T)
    queries = (2.0 * windows[labels] + draw(N, F, T)).astype(np.float32)
    _cases[key] = dict(F=F, T=T, M=M, N=N, tracks=tracks, local=local, starts=starts, table=table, queries=queries, labels=labels)
    return _cases[key]


def windows_of(table, starts, T):
    """(M, F, T) float32: the candidates cut out on the host, the way a SpeechBank takes them."""
    return np.stack([table[s: s + T].T for s in starts]).astype(np.float32)


def rounded(x, dtype: str):
    """x rounded to bf16 / fp16 and widened to float64 (round to nearest even, as the pack kernel's conversion)."""
    import torch
    return torch.from_numpy(np.ascontiguousarray(x, dtype=np.float32)).to({"bf16": torch.bfloat16, "fp16": torch.float16}[dtype]).double().numpy()


def cosine64(c, dtype=None):
    """Float64 brute force: (N, M) cosine of every query against every window, (M,) squared norms, (N, M) dot products."""
    T = c["T"]
    table = c["table"] if dtype is None else rounded(c["table"], dtype)
    q = c["queries"].astype(np.float64) if dtype is None else rounded(c["queries"], dtype)
    W = np.stack([table[s: s + T].T.reshape(-1) for s in c["starts"]])
    Q = q.reshape(q.shape[0], -1)
    dots = Q @ W.T
    qsq, csq = (Q * Q).sum(1), (W * W).sum(1)
    return dots / np.maximum(np.sqrt(qsq)[:, None] * np.sqrt(csq)[None, :], 1e-8), csq, dots


class Restated(tuple):
    """(indices, scores, ranks) plus .S, .qsq, .csq, and .outside: the path formed an address outside the table."""


def restate(c, k=10, mc=None, mutant=None):
    """What retrieve(Q, window_bank, k, labels) returns, restated: the device path's index arithmetic in float64 sums (exact on
    the integer cases), then the selection kernel's fp32 cosine, order (score descending, lower index first) and rank count.
    `mc`: candidates per chunk (None: one chunk).  `mutant`: one of MUTANTS, a planted bug."""
    assert mutant is None or mutant in MUTANTS
    F, T, M, N = c["F"], c["T"], c["M"], c["N"]
    starts, Ltot = c["starts"], c["table"].shape[0]
    slack = T + ROW_PAD + 2
    table = np.concatenate([np.zeros((slack, F)), c["table"], np.zeros((slack, F))])       # reads outside are noted, not faults
    outside = False
    # the packed queries: ROW_PAD zero rows in front of every segment's T rows
    Qp = np.zeros((N, ROW_PAD + T, F))
    Qp[:, ROW_PAD:] = c["queries"].astype(np.float64).transpose(0, 2, 1)
    skip, krows = ROW_PAD, T
    if mutant == "k_one_row_short":
        krows = T - 1
    if mutant == "k_one_row_long":
        krows = T + 1
    if mutant == "query_pad_rows_included":
        skip = 0
    Qp = np.concatenate([Qp.reshape(N * (ROW_PAD + T), F), np.zeros((ROW_PAD + 1, F))])    # the next segment's pad rows follow
    X = np.stack([Qp[i * (ROW_PAD + T) + skip: i * (ROW_PAD + T) + skip + krows].reshape(-1) for i in range(N)])
    mc = pad64(M) if mc is None else mc
    S = np.zeros((N, M))
    for c0 in range(0, M, mc):
        m = min(mc, M - c0)
        for jj in range(m):
            n0, r = jj // TILE * TILE, jj % TILE
            look = c0 + n0 + r
            if mutant == "tile_offset_dropped":
                look = c0 + r
            if mutant == "chunk_offset_dropped":
                look = n0 + r
            s = int(starts[look])
            if mutant == "start_plus_1":
                s += 1
            if mutant == "start_minus_1":
                s -= 1
            if mutant == "regular_pitch":
                s = (c0 + jj) * T % (Ltot - T + 1)
            outside |= s < 0 or s + krows > Ltot
            S[:, c0 + jj] = X @ table[slack + s: slack + s + krows].reshape(-1)
    nstart = starts + (1 if mutant == "norm_wrong_start" else 0)
    nrows = T + (1 if mutant == "norm_one_row_long" else -1 if mutant == "norm_one_row_short" else 0)
    row_sq = (table * table).sum(1)
    csq = np.array([row_sq[slack + s: slack + s + nrows].sum() for s in nstart])
    outside |= bool((nstart + nrows > Ltot).any())
    q = c["queries"].astype(np.float64).reshape(N, -1)
    qsq = (q * q).sum(1)
    out = Restated(select(S, qsq, csq, c["labels"], k))
    out.S, out.qsq, out.csq, out.outside = S, qsq, csq, outside
    return out


def select(S, qsq, csq, labels, k):
    """The selection kernel's formula in fp32 (csrc/retrieval.hip: dot / max(sqrt(qsq) * sqrt(csq), 1e-8), -0 = +0), a stable sort
    by (-score, index), a plain count for the ranks."""
    S32, qn, cn = S.astype(np.float32), np.sqrt(qsq.astype(np.float32)), np.sqrt(csq.astype(np.float32))
    sc = S32 / np.maximum(qn[:, None] * cn[None, :], np.float32(1e-8)) + np.float32(0.0)
    order = np.argsort(-sc, axis=1, kind="stable")[:, :k]
    N, M = S.shape
    sl = sc[np.arange(N), labels][:, None]
    j = np.arange(M)[None, :]
    ranks = ((sc > sl) | ((sc == sl) & (j < labels[:, None]))).sum(1).astype(np.int32)
    return order.astype(np.int64), np.take_along_axis(sc, order, 1), ranks


def class_ids(M: int, seed: int = 5):
    """A few large classes and many singletons: classes 0 ... 3 share half of the candidates, every other candidate is alone."""
    rng = np.random.RandomState(seed)
    ids = np.empty(M, dtype=np.int64)
    big = rng.permutation(M)[: M // 2]
    ids[big] = rng.randint(0, 4, size=big.shape[0])
    rest = np.setdiff1d(np.arange(M), big)
    ids[rest] = 4 + np.arange(rest.shape[0])
    return ids
