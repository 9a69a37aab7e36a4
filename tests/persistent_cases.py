"""Cases for the persistent kernels' multi-tile runs: (shape, CU limit) pairs at which, per the launch-plan mirrors of
tests/cu_limit.py, one workgroup walks several tiles — the compositions the full workload runs — on a few hundred rows.
Operands, regimes and check_regime conditions are those of tests/exact_cases.py; the emulations below are the reference
arithmetic laid out tile by tile and run by run, with the bugs such kernels have planted as mutants (MUTANTS).
tests/test_persistent_runs_cpu.py proves on the CPU that every composition named here occurs and every mutant is caught;
tests/test_persistent_runs_gpu.py runs the cases on the kernels."""
import functools
from collections import namedtuple

import numpy as np
import torch

from tests import cu_limit as P
from tests import exact_cases as X
from tests import track_feed_cases as K

PAD = 16
T130 = 130                 # samples are 146 rows: no sample boundary falls on a 128-row unit boundary
MUTANTS = ["skip_last_unit_of_run", "run_overlap", "pair_second_half_from_previous_tile", "pair_halo_missing",
           "stats_pair_double_count", "next_tile_prefetch_clobbers", "stride_trip_dropped"]


# ---------------------------------------------------------------------------------------------------------------
# conv3_flat / conv1_flat
# ---------------------------------------------------------------------------------------------------------------
FlatCase = namedtuple("FlatCase", "name KS shape limit one_per_cu runs")       # runs: the units per run the mirror must give
S = X.ConvShape
# (cin, cout, dil, T, B).  Cout 320 = two 160-channel tiles (n_co = 2): under limit 1 one workgroup per channel tile walks every
# unit (B = 2, 3, 4, 7: 3, 4, 5, 8 units), under limit 2 two of them share the units.  cin == cout: the residual is the input.
FLAT3_CASES = [
    FlatCase("n2_then_single", 3, S(64, 320, 16, T130, 2), 2, False, (2, 1)),          # one 256-row tile; a last run of one unit
    FlatCase("n3", 3, S(64, 320, 2, T130, 2), 1, False, (3,)),                         # 256 + 128
    FlatCase("n4", 3, S(64, 320, 16, T130, 3), 1, False, (4,)),                        # 256 + 256; the last unit partial, a second half
    FlatCase("n4_residual", 3, S(320, 320, 2, T130, 3), 1, True, (4,)),
    FlatCase("n5", 3, S(64, 320, 2, T130, 4), 1, True, (5,)),                          # 256 + 256 + 128
    FlatCase("n3_then_n2", 3, S(64, 320, 16, T130, 4), 2, False, (3, 2)),              # a last run shorter than the others
    FlatCase("n4_n4", 3, S(64, 320, 2, T130, 7), 2, False, (4, 4)),
    FlatCase("xcd_both_branches", 3, S(64, 320, 2, T130, 35), 16, False, (3,) * 13 + (1,)),
]
FLAT1_CASES = [
    FlatCase("n2_then_single", 1, S(64, 320, 0, T130, 2), 2, False, (2, 1)),
    FlatCase("n3", 1, S(64, 320, 0, T130, 2), 1, False, (3,)),
    FlatCase("n4", 1, S(64, 320, 0, T130, 3), 1, True, (4,)),
    FlatCase("n5", 1, S(64, 320, 0, T130, 4), 1, False, (5,)),
    FlatCase("n3_then_n2", 1, S(64, 320, 0, T130, 4), 2, False, (3, 2)),
    FlatCase("xcd_both_branches", 1, S(64, 320, 0, T130, 35), 16, False, (3,) * 13 + (1,)),
    # Cout 128: one 128-channel tile (n_co = 1), the width SDA_EPI_ROW_SUMSQ is built for
    FlatCase("w128_n2_then_single", 1, S(64, 128, 0, T130, 2), 1, False, (2, 1)),
    FlatCase("w128_n4", 1, S(64, 128, 0, T130, 3), 1, True, (4,)),
    FlatCase("w128_n3_then_n2", 1, S(64, 128, 0, T130, 4), 1, False, (3, 2)),
    FlatCase("w128_n8", 1, S(64, 128, 0, T130, 7), 1, True, (8,)),
]
del S
FLAT_CASES = {3: FLAT3_CASES, 1: FLAT1_CASES}
# F.glu in conv3_flat's epilogue (exact_cases.GLU_SHAPE: 2 x 320 padded channels = 4 tiles of 80 values + 80 gates, 435 rows = 4 units):
# under limit 1 every channel tile is one run of two 256-row tiles
GLU_LIMIT = 1


def flat_tile_co(c):
    return 160 if c.shape.cout % 160 == 0 else 128


def flat_plan(c, device_cus=P.DEVICE_CUS, fp32=False):
    """the mirror's plan of a case; fp32=True only for conv3_flat's fp32 storage"""
    s = c.shape
    n_co = X_pad(s.cout) // flat_tile_co(c)
    return P.flat_runs(P.flat_units(s.B, s.T), n_co, P.effective_cus(c.limit, device_cus), c.one_per_cu, fp32 and c.KS == 3)


def X_pad(c):
    return (c + 63) // 64 * 64


@functools.lru_cache(maxsize=None)
def _flat_operands(KS, shape, regime, key):
    seed = 11000 + 1000 * KS + 7 * shape.B + shape.cout + shape.dil + shape.cin
    return X._search(lambda R: X._conv_build(shape, KS, seed, R), regime, key, f"conv{KS} flat {tuple(shape)}")


def flat_case(c, regime, dtype):
    """X.ConvCase of a FlatCase: exact-regime operands are the same for every dtype, fp32 shares bf16's rounding-regime operands"""
    key = None if regime == "exact" else (torch.bfloat16 if dtype == torch.float32 else dtype)
    return _flat_operands(c.KS, c.shape, regime, key)


def epilogues(case):
    return [e for e in X.EPILOGUES if e != "bias_res" or case.res is not None]


def to_flat(x, rows):
    """(B, C, T) -> (rows, C): the flat row space, PAD zero rows in front of every sample, zeros behind the last"""
    B, C, T = x.shape
    out = torch.zeros(rows, C, dtype=torch.float64)
    for b in range(B):
        out[b * (T + PAD) + PAD: (b + 1) * (T + PAD)] = x[b].t()
    return out


def from_flat(yf, B, T):
    return torch.stack([yf[b * (T + PAD) + PAD: (b + 1) * (T + PAD)].t() for b in range(B)])


def _shifted(xf, d):
    """row f of the result = row f + d of xf, zeros outside"""
    out = torch.zeros_like(xf)
    n = xf.shape[0]
    if d >= 0:
        out[:n - d] = xf[d:]
    else:
        out[-d:] = xf[:n + d]
    return out


def flat_emulation(c, case, dtype, epilogue, plan, mutant=None):
    """The flat kernels as they are meant to compute a case under `plan` — per channel tile and run, 256- and 128-row tiles of the
    flat row space, bias and residual into the accumulator, one rounding, valid rows stored into a zeroed buffer, one `stats` row
    per unit (a 256-row tile: its sums into the first unit's row, zeros into the second) — or one mutant of that.
    Returns (y (B, Cout, T) float64, stats sum plane (n_units, Cout) float64 with NaN where nothing was written)."""
    assert mutant is None or mutant in MUTANTS
    s, KS = case.shape, c.KS
    Tp, total = s.T + PAD, s.B * (s.T + PAD)
    n_units = P.flat_units(s.B, s.T)
    rows = n_units * 128 + 512
    xf = to_flat(case.x, rows)
    w = case.w
    taps = [(k - KS // 2) * s.dil for k in range(KS)]
    acc = sum(_shifted(xf, d) @ w[:, :, k].t() for k, d in enumerate(taps))
    epi = torch.zeros(rows, s.cout, dtype=torch.float64)
    if epilogue != "bare":
        epi += case.bias[None, :]
    if epilogue == "bias_res":
        epi += xf
    f = torch.arange(rows)
    valid = (f < total) & (f % Tp >= PAD)
    yf = torch.zeros(rows, s.cout, dtype=torch.float64)
    stats = torch.full((n_units, s.cout), float("nan"), dtype=torch.float64)
    tile_co = flat_tile_co(c)
    lens = [sum(t // 128 for t in tiles) for tiles in plan.runs]
    only128 = all(t == 128 for tiles in plan.runs for t in tiles)          # conv3_flat's fp32 plan (or runs of single units)
    for co in range(s.cout // tile_co):
        ch = slice(co * tile_co, (co + 1) * tile_co)
        for r, n in enumerate(lens):
            u0 = r * plan.units_per_wg
            twice = 0
            if mutant == "run_overlap" and r >= 1:
                u0, n, twice = u0 - 1, n + 1, 1                      # this run takes the unit in front of it as well
            if mutant == "skip_last_unit_of_run":
                n -= 1
            sizes = (128,) * n if only128 else (256,) * (n >> 1) + (128,) * (n & 1)
            u, prev = u0, None
            for size in sizes:
                f0 = u * 128
                a = acc[f0: f0 + size, ch].clone()
                if size == 256 and mutant == "pair_second_half_from_previous_tile" and prev is not None:
                    back = f0 - prev                                # rows 128..255: the first K-step (tap 0, 32 channels) of the tile before
                    lo = f0 + 128 + taps[0]
                    a[128:] += (xf[lo - back: lo - back + 128, :32] - xf[lo: lo + 128, :32]) @ w[ch, :32, 0].t()
                if size == 256 and mutant == "pair_halo_missing":
                    for k, d in enumerate(taps):                    # rows 128..143 read zeros where they reach back into rows 112..127
                        for i in range(128, 144):
                            if 112 <= i + d < 128:
                                a[i] -= w[ch, :, k] @ xf[f0 + i + d]
                e = epi[f0: f0 + size, ch]
                y = X.store(a + e, dtype)
                if twice and u == u0:
                    y[:128] = X.store(a[:128] + 2 * e[:128], dtype)
                ok = valid[f0: f0 + size]
                y = torch.where(ok[:, None], y, yf[f0: f0 + size, ch])
                yf[f0: f0 + size, ch] = y
                sums = (y * ok[:, None]).sum(0)
                stats[u, ch] = sums
                if size == 256:
                    stats[u + 1, ch] = sums if mutant == "stats_pair_double_count" else 0.0
                prev, u = f0, u + size // 128
    return from_flat(yf, s.B, s.T), stats


def flat_mutant_applies(c, epilogue, plan, mutant):
    """whether a mutant can change anything of a case under its plan (the cases `meant to catch it`)"""
    tiles = P.flat_tiles(plan)
    pair = any(rows == 256 for _, _, rows in tiles)
    if mutant == "skip_last_unit_of_run":
        return True
    if mutant == "run_overlap":
        return plan.runs_per_co >= 2 and epilogue != "bare"
    if mutant == "pair_second_half_from_previous_tile":
        return any(rows == 256 and any(r2 == r and u2 < u for r2, u2, _ in tiles) for r, u, rows in tiles)
    if mutant == "pair_halo_missing":
        return pair and c.KS == 3
    if mutant == "stats_pair_double_count":
        return pair
    return False


# ---------------------------------------------------------------------------------------------------------------
# conv1_wide
# ---------------------------------------------------------------------------------------------------------------
WideCase = namedtuple("WideCase", "name shape limit")
# 16-bit only.  B = 3: 438 rows = 2 row tiles of 256; B = 19: 2774 rows = 11.  Cout 256 and 320: one channel tile; 512: two of 256.
WIDE_CASES = [
    WideCase("w256_one_workgroup", X.ConvShape(64, 256, 0, T130, 3), 1),               # one workgroup walks every tile
    WideCase("w320_one_workgroup", X.ConvShape(64, 320, 0, T130, 7), 1),
    WideCase("w256_cin96_one_workgroup", X.ConvShape(96, 256, 0, T130, 7), 1),         # four K-steps: more than the ring's depth
    WideCase("w512_one_workgroup", X.ConvShape(64, 512, 0, T130, 3), 1),
    WideCase("w320_grid3", X.ConvShape(64, 320, 0, T130, 7), 3),                       # linear map, 4 tiles: an uneven last round
    WideCase("w256_xcd_grid8", X.ConvShape(64, 256, 0, T130, 19), 8),                  # xcd_map; round 2: three of eight have a tile
    WideCase("w512_xcd_grid16", X.ConvShape(64, 512, 0, T130, 19), 16),                # xcd_map with (G / 8) % n_ch == 0, n_ch = 2
]


def wide_tn(c):
    return 256 if c.shape.cout % 256 == 0 else 320


def wide_plan(c, device_cus=P.DEVICE_CUS):
    s = c.shape
    return P.wide_tiles(P.ceil_div(s.B * (s.T + PAD), 256), s.cout // wide_tn(c), P.effective_cus(c.limit, device_cus))


@functools.lru_cache(maxsize=None)
def _wide_operands(shape, regime, key):
    seed = 13000 + 7 * shape.B + shape.cout + shape.cin
    return X._search(lambda R: X._conv_build(shape, 1, seed, R), regime, key, f"conv1 wide {tuple(shape)}")


def wide_case(c, regime, dtype):
    assert dtype in X.DTYPES16
    return _wide_operands(c.shape, regime, None if regime == "exact" else dtype)


def wide_emulation(c, case, dtype, plan, mutant=None):
    """conv + bias on 256-row x TN-channel tiles, each workgroup walking its tiles in order.  next_tile_prefetch_clobbers: the last
    K-step (32 elements of the padded contraction) of a tile holds the input rows and weight rows of the workgroup's NEXT tile."""
    assert mutant in (None, "next_tile_prefetch_clobbers")
    s = case.shape
    cin_p, tn = X_pad(s.cin), wide_tn(c)
    n_row_tiles = P.ceil_div(s.B * (s.T + PAD), 256)
    xf = torch.zeros(n_row_tiles * 256, cin_p, dtype=torch.float64)
    xf[:, :s.cin] = to_flat(case.x, n_row_tiles * 256)
    w = torch.zeros(s.cout, cin_p, dtype=torch.float64)
    w[:, :s.cin] = case.w[:, :, 0]
    yf = torch.zeros(n_row_tiles * 256, s.cout, dtype=torch.float64)
    for mine in plan.tiles:
        for i, (row, ch) in enumerate(mine):
            r, cs = slice(row * 256, row * 256 + 256), slice(ch * tn, ch * tn + tn)
            xa, wa = xf[r].clone(), w[cs].clone()
            if mutant and i + 1 < len(mine):
                nrow, nch = mine[i + 1]
                xa[:, cin_p - 32:] = xf[nrow * 256: nrow * 256 + 256, cin_p - 32:]
                wa[:, cin_p - 32:] = w[nch * tn: nch * tn + tn, cin_p - 32:]
            yf[r, cs] = X.store(xa @ wa.t() + case.bias[None, cs], dtype)
    return from_flat(yf, s.B, s.T)


def wide_mutant_applies(c, plan):
    return X_pad(c.shape.cin) - 32 < c.shape.cin and any(len(m) >= 2 for m in plan.tiles)


# ---------------------------------------------------------------------------------------------------------------
# the loss's dZ, the similarity GEMM
# ---------------------------------------------------------------------------------------------------------------
DzCase = namedtuple("DzCase", "name shape limit split")       # split: tiles per workgroup x the mirror must give
# register form (Bm <= 256, 64-column tiles): F = 64, T = 11 -> 27 rows of 64 = 27 tiles; tiled form (Bm >= 256, Bm % 32 == 0,
# 256-column tiles): F = 64, T = 28 -> 44 rows of 64 = 11 tiles.  Bn > 256: two column blocks (blockIdx.y).
DZ_CASES = [
    DzCase("registers_two_workgroups", X.ClipShape(100, 70, 64, 11), 1, (14, 13)),
    DzCase("registers_two_column_blocks", X.ClipShape(40, 260, 64, 11), 1, (27,)),
    DzCase("tiled_one_workgroup", X.ClipShape(288, 70, 64, 28), 1, (11,)),
    DzCase("tiled_two_workgroups", X.ClipShape(288, 70, 64, 28), 2, (6, 5)),
    DzCase("tiled_two_column_blocks", X.ClipShape(256, 300, 64, 28), 2, (11,)),
] + [DzCase(f"exact_cases_{i}", s, 1, None) for i, s in enumerate(X.CLIP_SHAPES)]


def dz_row_elems(s):
    return (s.T + PAD) * X_pad(s.F)


def dz_plan(c, device_cus=P.DEVICE_CUS):
    s = c.shape
    return P.dz_plan(s.Bm, s.Bn, dz_row_elems(s), P.effective_cus(c.limit, device_cus))


def dz_split(plan):
    _, _, ntiles, gx, _ = plan
    return tuple(len(range(x, ntiles, gx)) for x in range(gx))


@functools.lru_cache(maxsize=None)
def _dz_operands(name, regime, key):
    c = next(c for c in DZ_CASES if c.name == name)
    s = c.shape
    seed = 17000 + 10 * [d.name for d in DZ_CASES].index(name)

    def build(R):
        t = X._typed_build(X.TypedShape(s.Bm, s.Bn, s.F * s.T), seed, R, (0.5, 1.0))
        sh = lambda v, n: v.reshape(n, s.T, s.F).permute(0, 2, 1).contiguous()        # noqa: E731  rows are (t, f) in the row layout
        return X.ClipCase(s, R, t.G, sh(t.Y, s.Bm), sh(t.sub, s.Bn), t.acc_scale, t.rscale, t.out_scale, sh(t.ref, s.Bn))
    return X._search(build, regime, key, f"clip_dz {name}")


def dz_case(c, regime, dtype):
    assert dtype in X.DTYPES16
    if c.name.startswith("exact_cases_"):
        return X.clip_case(int(c.name.rsplit("_", 1)[1]), regime, dtype)
    return _dz_operands(c.name, regime, None if regime == "exact" else dtype)


def _layout(v, s):
    """(n, F, T) -> (n, row_elems): a sample's rows (t, f) with the PAD zero rows in front and the channel padding"""
    out = torch.zeros(v.shape[0], s.T + PAD, X_pad(s.F), dtype=torch.float64)
    out[:, PAD:, :s.F] = v.permute(0, 2, 1)
    return out.reshape(v.shape[0], -1)


def dz_emulation(case, dtype, plan, mutant=None):
    """out = out_scale * (cscale[j] * (G^T Y)[j][k] - rscale[j] * Z[j][k]) column tile by column tile, each workgroup walking tiles
    x, x + gx, ...  next_tile_prefetch_clobbers: the last 32 rows of the (padded) contraction of a tile are those of the workgroup's
    next tile.  Returns (Bn, F, T) float64."""
    assert mutant in (None, "next_tile_prefetch_clobbers")
    s = case.shape
    _, kt, ntiles, gx, _ = plan
    Y, Z = _layout(case.Y, s), _layout(case.Z, s)
    lo = (s.Bm - 1) // 32 * 32
    out = torch.zeros_like(Z)
    for t in range(ntiles):
        cols = slice(t * kt, (t + 1) * kt)
        Yt = Y[:, cols].clone()
        if mutant and t + gx < ntiles:
            Yt[lo:] = Y[lo:, (t + gx) * kt: (t + gx + 1) * kt]
        out[:, cols] = X.store(case.out_scale * (case.cscale[:, None] * (case.G.t() @ Yt) - case.rscale[:, None] * Z[:, cols]), dtype)
    return out.reshape(s.Bn, s.T + PAD, X_pad(s.F))[:, PAD:, :s.F].permute(0, 2, 1)


# the similarity GEMM's K split follows the CU count (sim_gemm.hip:235-240): X.SIM_SHAPES at the count under limit 1 and under none
SIM_LIMIT = 1
# the fixed shape whose ksplit witnesses a limit in this thread: one tile, 64 K-steps -> ceil(cus / 8) * 8, at most 64
WITNESS_SHAPE = (256, 256, 2048)


def witness_ksplit(cus):
    return P.sim_ksplit(*WITNESS_SHAPE, cus)


# ---------------------------------------------------------------------------------------------------------------
# the gathers: bytes, as tests/track_feed_cases.py keeps them
# ---------------------------------------------------------------------------------------------------------------
GATHER_LIMIT = 1
GATHER_UTYPES = {"bf16": np.uint16, "fp16": np.uint16, "fp32": np.uint32}
# whole samples: 23 samples of (52 + 16) rows x 128 channels; 9 indices with duplicates, the first and the last sample, a reversed
# stretch.  (sda_gather_samples documents no range check: every index is inside the table.)
GS = dict(N=23, F=96, T=52, idx=[22, 21, 13, 7, 5, 5, 1, 0, 22])
# windows: 53 rows x 128 channels from a 3-track table; candidates outside [0, M) and a start outside the table come back as zeros
GW = dict(F=70, T=53, lens=(61, 97, 70), idx=[6, 5, 4, 4, -1, 0, 7, 8, 3, 2])


def gather_samples_case(utype):
    N, F, T = GS["N"], GS["F"], GS["T"]
    Tp, Cp = T + PAD, K.pad64(F)
    table = np.zeros((N * Tp + K.SLACK, Cp), dtype=utype)
    body = K.make_table(N * T, F, utype, seed=41)
    for n in range(N):
        table[n * Tp + PAD: (n + 1) * Tp] = body[n * T: (n + 1) * T]
    return dict(table=table, idx=np.asarray(GS["idx"], dtype=np.int64), B=len(GS["idx"]), T=T, Cp=Cp,
                vecs=Tp * Cp * np.dtype(utype).itemsize // 16)


def gather_samples_ref(c, mutant=None, bx=1):
    """the whole destination, rows_alloc(B, T) x Cp, FILL where sda_gather_samples writes nothing (behind the last sample)"""
    assert mutant in (None, "stride_trip_dropped")
    table, Tp = c["table"], c["T"] + PAD
    out = np.full((K.rows_alloc(c["B"], c["T"]), c["Cp"]), K.FILL[table.dtype], dtype=table.dtype)
    per_vec = 16 // table.dtype.itemsize
    for b, n in enumerate(c["idx"]):
        sample = table[n * Tp: (n + 1) * Tp].copy().reshape(-1)
        if mutant:
            sample[P.gather_trips(c["vecs"], bx)[1] * per_vec:] = K.FILL[table.dtype]
        out[b * Tp: (b + 1) * Tp] = sample.reshape(Tp, -1)
    return out


def gather_windows_case(utype):
    F, T, lens = GW["F"], GW["T"], GW["lens"]
    L = sum(lens)
    starts = np.asarray([0, 8, 61, 61 + 97 - T, 61 + 97, L - T, L - T + 1, -3], dtype=np.int32)      # the last two: outside the table
    table = K.make_table(L, F, utype, seed=43)
    return dict(table=table, starts=starts, idx=np.asarray(GW["idx"], dtype=np.int64), B=len(GW["idx"]), T=T, F=F, Cp=K.pad64(F),
                vecs=T * K.pad64(F) * np.dtype(utype).itemsize // 16)


def gather_windows_ref(c, mutant=None, bx=1):
    assert mutant in (None, "stride_trip_dropped")
    out = K.gather_windows_ref(c["table"], c["starts"], c["idx"], c["T"])
    if mutant:
        per_vec, Tp = 16 // c["table"].dtype.itemsize, c["T"] + PAD
        for b in range(c["B"]):
            window = out[b * Tp + PAD: (b + 1) * Tp].reshape(-1)
            window[P.gather_trips(c["vecs"], bx)[1] * per_vec:] = K.FILL[c["table"].dtype]
            out[b * Tp + PAD: (b + 1) * Tp] = window.reshape(c["T"], -1)
    return out


# ---------------------------------------------------------------------------------------------------------------
# the robust statistics: rows of 4k + 1 distinct integers (tests/test_subject_feed_gpu.py: the statistics are elements of the row)
# ---------------------------------------------------------------------------------------------------------------
RobustCase = namedtuple("RobustCase", "name S C L pooled limit")
# 8 rows.  limit 1: want = ceil(8 / 8) = 1 slice: one workgroup per row over 12289 (12297) samples = 3+ shares of RS_WG_ELEMS;
# limit 2: want = 2 of at most 4 slices.  Pooled: a row is 3 chunks of 4099, a slice of 6149 samples runs across a chunk's end.
ROBUST_CASES = [RobustCase("subject_wise_one_slice", 2, 4, 12289, False, 1), RobustCase("subject_wise_two_slices", 2, 4, 12289, False, 2),
                RobustCase("pooled_one_slice", 3, 8, 4099, True, 1), RobustCase("pooled_two_slices", 3, 8, 4099, True, 2)]


def robust_plan(c, device_cus=P.DEVICE_CUS):
    N, rows = (c.S * c.L, c.C) if c.pooled else (c.L, c.S * c.C)
    return P.robust_slices(N, rows, P.effective_cus(c.limit, device_cus))


def robust_input(c):
    """X (S, C, L) float32: every row of the statistics (a (subject, channel) pair, or a channel over every subject) holds
    distinct integers of both signs, shuffled, a different offset per row"""
    N, rows = (c.S * c.L, c.C) if c.pooled else (c.L, c.S * c.C)
    assert N % 4 == 1
    rng = np.random.RandomState(N + rows)
    r = np.stack([rng.permutation(N).astype(np.float32) * 3 - np.float32(N + 7 * i) for i in range(rows)])
    if c.pooled:
        return np.ascontiguousarray(r.reshape(c.C, c.S, c.L).transpose(1, 0, 2))
    return r.reshape(c.S, c.C, c.L)
