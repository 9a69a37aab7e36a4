"""The handle on persistent kernels' launch plans, and those plans restated in Python.

Six kernels size their grid from the CU count launch_cus() reports (csrc/capi.hip:49-57) and then walk several tiles per
workgroup.  On a 256-CU device every small test shape gives one tile per workgroup; sda_set_cu_limit(n) (capi.hip:61-65, host
only, thread-local) lowers what launch_cus() reports, so that shapes of a few hundred rows run the compositions of the full
workload.  cu_limit(n) is the only place the tests call it.

The mirrors below are written from the C as it stands, each citing its lines.  They exist to CHOOSE cases and to STATE what a
case exercises (tests/test_persistent_runs_cpu.py asserts that through them); a kernel is never compared with a mirror except
through the witnesses of tests/test_persistent_runs_gpu.py.  In every mirror `cus` is what launch_cus() returns:
effective_cus(limit, device CUs)."""
import contextlib
from collections import namedtuple

DEVICE_CUS = 256          # MI355X; the GPU tests pass the device's own count


@contextlib.contextmanager
def cu_limit(n):
    """launch_cus() reports min(n, device CUs) to launches from THIS thread inside the block; the previous limit comes back
    afterwards, and the restoring call must find n still in force."""
    from speech_decoding_amd import lib
    L = lib.load()
    assert n > 0
    previous = L.sda_set_cu_limit(n)
    try:
        yield
    finally:
        replaced = L.sda_set_cu_limit(previous)
        assert replaced == n, f"the CU limit inside the block was {replaced}, not {n}"


def clear_cu_limit():
    """remove this thread's limit; returns the one that was in force (0: none) — a module's teardown asserts 0"""
    from speech_decoding_amd import lib
    return lib.load().sda_set_cu_limit(0)


def effective_cus(limit, device_cus=DEVICE_CUS):
    """capi.hip:56: (g_cu_limit > 0 && g_cu_limit < cus[dev]) ? g_cu_limit : cus[dev]"""
    return limit if 0 < limit < device_cus else device_cus


def ceil_div(a, b):
    return -(-a // b)


# ---------------------------------------------------------------------------------------------------------------
# conv3_flat / conv1_flat
# ---------------------------------------------------------------------------------------------------------------
FlatRuns = namedtuple("FlatRuns", "units_per_wg runs_per_co grid runs")       # runs[r] = tile sizes (rows) run r executes, in order


def flat_units(B, T, pad=16, unit_rows=128):
    """flat_tile.h:52-53: n_units = ceil(B * rows_tp(T) / unit_rows)"""
    return ceil_div(B * (T + pad), unit_rows)


def flat_runs(n_units, n_co, cus, one_per_cu, fp32=False):
    """flat_plan (flat_tile.h:50-63) and the tile plan of a run of n units.
    16-bit storage, without SDA_CONV_FLAT_STAGGER (conv3_flat.hip:505-521, conv1_flat.hip:311-315): n >> 1 256-row tiles, then
    one 128-row tile when n is odd.  fp32=True is conv3_flat's fp32 storage (conv3_flat.hip:512-517): 128-row tiles only;
    conv1_flat has no such branch and takes the 16-bit plan in every storage type."""
    slots = (1 if one_per_cu else 2) * cus
    units_per_wg = max(1, ceil_div(n_units * n_co, slots))
    runs_per_co = ceil_div(n_units, units_per_wg)
    runs = []
    for r in range(runs_per_co):
        n = min(n_units, (r + 1) * units_per_wg) - r * units_per_wg
        runs.append((128,) * n if fp32 else (256,) * (n >> 1) + (128,) * (n & 1))
    return FlatRuns(units_per_wg, runs_per_co, runs_per_co * n_co, tuple(runs))


def flat_tiles(plan):
    """[(run, first unit, rows)] of every tile of one channel tile's runs"""
    out = []
    for r, tiles in enumerate(plan.runs):
        u = r * plan.units_per_wg
        for rows in tiles:
            out.append((r, u, rows))
            u += rows // 128
    return out


def flat_second_halves(plan):
    """the units (= `stats` rows) that are rows 128..255 of a 256-row tile: the tile's sums go into its first unit's row, zeros
    into this one (conv3_flat.hip:458-463, conv1_flat.hip:278-283)"""
    return sorted(u + 1 for _, u, rows in flat_tiles(plan) if rows == 256)


def xcd_block_order(bid, grid, n_co):
    """flat_tile.h:68-80 -> (co_tile, run) of workgroup `bid`"""
    group = 8 * n_co
    full = grid // group * group
    if bid < full:
        base = bid // group * group
        rem = bid - base
        return rem // 8, base // n_co + (rem & 7)
    rem = bid - full
    return rem % n_co, full // n_co + rem // n_co


# ---------------------------------------------------------------------------------------------------------------
# conv1_wide
# ---------------------------------------------------------------------------------------------------------------
WideTiles = namedtuple("WideTiles", "grid xcd_map n_rounds tiles")            # tiles[w] = [(row_tile, ch_tile)] workgroup w walks


def wide_tiles(n_row_tiles, n_ch, cus):
    """launch_wide (conv1_wide.hip:339-346) and the kernel's tile_of / n_rounds (conv1_wide.hip:86-101); the walk ends at the
    first round without a tile (conv1_wide.hip:153-155, 204, 329)."""
    grid = cus // 8 * 8
    if grid < 8:
        grid = cus
    grid = min(grid, n_row_tiles * n_ch)
    xcd_map = grid % 8 == 0 and (grid // 8) % n_ch == 0
    rows_per_round = grid // n_ch if xcd_map else 0
    n_rounds = ceil_div(n_row_tiles, rows_per_round) if xcd_map else ceil_div(n_row_tiles * n_ch, grid)
    tiles = []
    for w in range(grid):
        mine = []
        for k in range(n_rounds):
            if xcd_map:
                x, j = w & 7, w >> 3
                row, ch = k * rows_per_round + x * ((grid // 8) // n_ch) + j // n_ch, j % n_ch
            else:
                row, ch = divmod(k * grid + w, n_ch)
            if row >= n_row_tiles:
                break
            mine.append((row, ch))
        tiles.append(mine)
    return WideTiles(grid, xcd_map, n_rounds, tiles)


# ---------------------------------------------------------------------------------------------------------------
# the loss's dZ
# ---------------------------------------------------------------------------------------------------------------
DZ_KT, DT_TILE, DZ_ROWS = 64, 256, 256        # loss_gemm.hip:28-29, 231


def dz_is_tiled(Bm, row_elems):
    """dz_tiles_ok (loss_gemm.hip:385-388), 16-bit storage assumed"""
    return Bm >= DZ_ROWS and Bm % 32 == 0 and row_elems >= DT_TILE and row_elems % DT_TILE == 0


def dz_grid(ntiles, jblocks, cus, tiled):
    """launch_dz (loss_gemm.hip:207-212: two workgroups per CU in all) / launch_dz_tiles (loss_gemm.hip:374-378: one) ->
    (gx, jblocks); workgroup x of a column block walks tiles x, x + gx, ... (loss_gemm.hip:124-128, 299-301)"""
    gx = (cus if tiled else 2 * cus) // jblocks
    return min(max(gx, 1), ntiles), jblocks


def dz_plan(Bm, Bn, row_elems, cus):
    """(tiled, tile width, ntiles, gx, jblocks) of one sda_clip_dz call (loss_gemm.hip:208-209, 374-375, 410-416)"""
    tiled = dz_is_tiled(Bm, row_elems)
    kt = DT_TILE if tiled else DZ_KT
    ntiles, jblocks = row_elems // kt, ceil_div(Bn, 256)
    gx, _ = dz_grid(ntiles, jblocks, cus, tiled)
    return tiled, kt, ntiles, gx, jblocks


def sim_ksplit(M, N, K, cus):
    """sda_sim_gemm_ksplit (sim_gemm.hip:235-240), 16-bit storage"""
    tiles = ceil_div(M, 256) * ceil_div(N, 256)
    ks = ceil_div(ceil_div(cus, tiles), 8) * 8
    return max(1, min(ks, K // 32))


# ---------------------------------------------------------------------------------------------------------------
# the gathers, the robust statistics
# ---------------------------------------------------------------------------------------------------------------
def gather_bx(vecs, B, cus, per_lane):
    """sda_gather_samples (row_layout.hip:183-187, per_lane = 4) / sda_gather_windows (row_layout.hip:206-210, per_lane = 8):
    workgroups per sample; a lane's trip is bx * 256 vectors (row_layout.hip:112-118, 134-146)"""
    return max(1, min(ceil_div(vecs, 256 * per_lane), ceil_div(8 * cus, B)))


def gather_trips(vecs, bx):
    """trips of the longest-working lane, and the first vector of the last trip"""
    step = bx * 256
    return ceil_div(vecs, step), (vecs - 1) // step * step


RS_WG_ELEMS = 4096        # robust_rows.hip:27
RobustSlices = namedtuple("RobustSlices", "slices share grid_x most")


def robust_slices(N, rows, cus):
    """sda_robust_stats (robust_rows.hip:238-242): a row of N samples is cut over grid_x workgroups of `share` samples each"""
    want = ceil_div(8 * cus, rows)
    most = ceil_div(N, RS_WG_ELEMS)
    slices = 1 if want < 1 else min(want, most)
    share = ceil_div(N, slices)
    return RobustSlices(slices, share, ceil_div(N, share), most)
