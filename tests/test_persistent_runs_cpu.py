"""CPU-side proof for tests/test_persistent_runs_gpu.py: every (shape, CU limit) pair of tests/persistent_cases.py gives, per the
launch-plan mirrors of tests/cu_limit.py, the run composition it is named for; every operand set meets the conditions of its
regime; the tile-by-tile emulations equal the plain references; and every planted mutant changes at least one stored value of
every case meant to catch it."""
import numpy as np
import pytest
import torch

from tests import cu_limit as P
from tests import exact_cases as X
from tests import persistent_cases as C
from tests import track_feed_cases as K

ALL = [(r, d) for r in X.REGIMES for d in X.DTYPES]
ALL16 = [(r, d) for r in X.REGIMES for d in X.DTYPES16]


def differs(a, b):
    """NaN-aware: some stored value is not the same"""
    return X.mismatch(a, b, axes="") is not None


# ---------------------------------------------------------------------------------------------------------------
# the mirrors themselves, on hand-worked plans
# ---------------------------------------------------------------------------------------------------------------
def test_flat_plan_mirror_on_hand_worked_plans():
    # 256 CUs, the largest exact_cases shape (3 units, 2 channel tiles): one 128-row tile per workgroup — what runs with no limit
    p = P.flat_runs(3, 2, 256, False)
    assert (p.units_per_wg, p.runs_per_co, p.grid, p.runs) == (1, 3, 6, ((128,),) * 3)
    # the stagger test's shapes: 384 units -> 2 per workgroup, 641 -> 3
    assert P.flat_runs(384, 2, 256, False).units_per_wg == 2 and P.flat_runs(641, 2, 256, False).units_per_wg == 3
    p = P.flat_runs(5, 2, 1, False)
    assert (p.units_per_wg, p.runs_per_co, p.grid, p.runs) == (5, 1, 2, ((256, 256, 128),))
    assert P.flat_runs(5, 2, 1, False, fp32=True).runs == ((128,) * 5,)
    p = P.flat_runs(5, 2, 2, False)
    assert (p.units_per_wg, p.runs, P.flat_second_halves(p)) == (3, ((256, 128), (256,)), [1, 4])
    assert P.flat_runs(5, 2, 2, True) == P.flat_runs(5, 2, 1, False)
    assert P.effective_cus(0) == 256 and P.effective_cus(16) == 16 and P.effective_cus(300) == 256 and P.effective_cus(4, 2) == 2


@pytest.mark.parametrize("grid,n_co", [(28, 2), (6, 2), (16, 2), (3, 1), (24, 1), (40, 4)])
def test_xcd_block_order_deals_every_run_of_every_channel_tile_once(grid, n_co):
    seen = sorted(P.xcd_block_order(b, grid, n_co) for b in range(grid))
    assert seen == [(c, r) for c in range(n_co) for r in range(grid // n_co)]
    group = 8 * n_co
    for b in range(grid // group * group):                 # inside a full group: blocks i and i + 8 read the same rows
        if b % group < group - 8:
            assert P.xcd_block_order(b, grid, n_co)[1] == P.xcd_block_order(b + 8, grid, n_co)[1]


def test_wide_dz_gather_and_robust_mirrors_on_hand_worked_plans():
    w = P.wide_tiles(11, 1, 256)
    assert w.grid == 11 and not w.xcd_map and all(len(t) == 1 for t in w.tiles)             # no limit: one tile per workgroup
    w = P.wide_tiles(11, 1, 8)
    assert w.grid == 8 and w.xcd_map and w.n_rounds == 2 and w.tiles[2] == [(2, 0), (10, 0)] and w.tiles[3] == [(3, 0)]
    w = P.wide_tiles(4, 1, 3)
    assert w.grid == 3 and not w.xcd_map and w.tiles == [[(0, 0), (3, 0)], [(1, 0)], [(2, 0)]]
    assert P.dz_grid(27, 1, 1, False) == (2, 1) and P.dz_grid(27, 2, 1, False) == (1, 2) and P.dz_grid(27, 1, 256, False) == (27, 1)
    assert P.dz_grid(11, 1, 1, True) == (1, 1) and P.dz_grid(11, 1, 2, True) == (2, 1) and P.dz_grid(11, 2, 2, True) == (1, 2)
    assert P.gather_bx(1088, 9, 256, 4) == 2 and P.gather_bx(1088, 9, 1, 4) == 1 and P.gather_trips(1088, 1) == (5, 1024)
    assert P.robust_slices(70001, 3, 256) == P.RobustSlices(18, 3889, 18, 18)
    assert P.sim_ksplit(300, 200, 512, 256) == 16 and P.sim_ksplit(300, 200, 512, 1) == 8


# ---------------------------------------------------------------------------------------------------------------
# the flat kernels
# ---------------------------------------------------------------------------------------------------------------
def test_flat_cases_give_the_compositions_they_are_named_for():
    for KS, cases in C.FLAT_CASES.items():
        seen, partial_second_half, last_single, shorter_last = set(), False, False, False
        for c in cases:
            s = c.shape
            assert s.T == C.T130 and (s.T + C.PAD) == 146 and s.cin in (64, 320)
            plan = C.flat_plan(c)
            lens = tuple(sum(t // 128 for t in tiles) for tiles in plan.runs)
            assert lens == c.runs, (KS, c.name, lens)
            assert sum(lens) == P.flat_units(s.B, s.T)
            for tiles in plan.runs:
                n = sum(t // 128 for t in tiles)
                assert tiles == (256,) * (n // 2) + (128,) * (n % 2)
                seen.add(n)
            if KS == 3:
                assert C.flat_plan(c, fp32=True).runs == tuple((128,) * n for n in lens)
            else:
                assert C.flat_plan(c, fp32=True) == plan                   # conv1_flat: the same tiles in every storage type
            last_single |= len(lens) > 1 and lens[-1] == 1
            shorter_last |= len(lens) > 1 and lens[-1] < lens[0]
            n_units = sum(lens)
            partial_second_half |= (s.B * 146) % 128 != 0 and (n_units - 1) in P.flat_second_halves(plan)
            if c.name == "xcd_both_branches":
                n_co = 2
                assert P.flat_units(s.B, s.T) == 40 and (plan.units_per_wg, plan.runs_per_co, plan.grid) == (3, 14, 28)
                full = plan.grid // (8 * n_co) * (8 * n_co)
                assert plan.grid >= 8 * n_co and full == 16 and plan.grid - full == 12
                runs_full = {P.xcd_block_order(b, plan.grid, n_co)[1] for b in range(full)}
                runs_rest = {P.xcd_block_order(b, plan.grid, n_co)[1] for b in range(full, plan.grid)}
                assert all(lens[r] >= 2 for r in runs_full) and any(lens[r] >= 2 for r in runs_rest)
        assert {2, 3, 4, 5} <= seen, (KS, seen)
        assert partial_second_half and last_single and shorter_last, KS
    # widths: Cout 320 = two 160-channel tiles in both kernels, Cout 128 = conv1_flat's row-sums width
    assert {c.shape.cout for c in C.FLAT3_CASES} == {320} and {c.shape.cout for c in C.FLAT1_CASES} == {320, 128}
    assert {c.shape.dil for c in C.FLAT3_CASES} == {16, 2}
    assert any(c.one_per_cu for c in C.FLAT3_CASES) and any(not c.one_per_cu for c in C.FLAT3_CASES)
    # the GLU case: 4 units in one run per channel tile under limit 1
    g = X.GLU_SHAPE
    p = P.flat_runs(P.flat_units(g.B, g.T), 2 * C.X_pad(X.GLU_HALF) // 160, P.effective_cus(C.GLU_LIMIT), False)
    assert p.runs == ((256, 256),) and p.grid == 4


@pytest.mark.parametrize("regime,dtype", ALL)
@pytest.mark.parametrize("KS", [3, 1])
def test_flat_cases_meet_their_regime_and_the_emulation_equals_the_reference(KS, regime, dtype):
    for c in C.FLAT_CASES[KS]:
        case = C.flat_case(c, regime, dtype)
        X.operand(case.x, dtype), X.operand(case.w, dtype)
        plan = C.flat_plan(c, fp32=dtype == torch.float32)
        for epi in C.epilogues(case):
            want = X.conv_expected(case, epi)
            X.check_regime(want, regime, dtype, f"conv{KS} flat {c.name} {epi}")
            y, stats = C.flat_emulation(c, case, dtype, epi, plan)
            X.assert_same(y, X.store(want, dtype), f"conv{KS} flat {c.name} {epi}")
            assert not bool(torch.isnan(stats).any())
            zero_rows = [u for u in range(stats.shape[0]) if not bool(stats[u].any())]
            assert zero_rows == ([] if (dtype == torch.float32 and KS == 3) else P.flat_second_halves(plan)), (c.name, epi)
            if regime == "exact":
                assert float(want.abs().sum(dim=(0, 2)).max()) < 2 ** 24
                X.assert_same(stats.sum(0), want.sum(dim=(0, 2)), f"conv{KS} flat {c.name} {epi} stats", axes="c")
        if KS == 1 and regime == "exact" and case.shape.cout % 128 == 0:
            assert float(X.row_sumsq_ref(X.conv_expected(case, "bias")).max()) < 2 ** 24
    assert any(C.flat_case(c, regime, dtype).res is not None for c in C.FLAT_CASES[3])
    g = X.glu_case(regime, dtype)
    X.check_regime(g.ref[:, X.GLU_HALF:], regime, dtype, "glu gate")


FLAT_MUTANTS = ["skip_last_unit_of_run", "run_overlap", "pair_second_half_from_previous_tile", "pair_halo_missing", "stats_pair_double_count"]


@pytest.mark.parametrize("mutant", FLAT_MUTANTS)
@pytest.mark.parametrize("KS", [3, 1])
def test_flat_mutants_are_caught_by_every_case_meant_for_them(KS, mutant):
    meant = 0
    for regime, dtype in ALL16:
        for c in C.FLAT_CASES[KS]:
            case = C.flat_case(c, regime, dtype)
            plan = C.flat_plan(c)
            for epi in C.epilogues(case):
                if not C.flat_mutant_applies(c, epi, plan, mutant):
                    continue
                y0, s0 = C.flat_emulation(c, case, dtype, epi, plan)
                y1, s1 = C.flat_emulation(c, case, dtype, epi, plan, mutant)
                if mutant == "stats_pair_double_count":
                    assert not differs(y0, y1) and differs(s0, s1), (c.name, epi)
                else:
                    assert differs(y0, y1), (KS, c.name, regime, dtype, epi)
                meant += 1
    assert meant >= (0 if (KS == 1 and mutant == "pair_halo_missing") else 8), meant
    # no limit (256 CUs): one 128-row tile per workgroup, and none of the pair mutants can show — the gap these cases close
    if mutant.startswith("pair") or mutant == "stats_pair_double_count":
        for c in C.FLAT_CASES[KS][:5]:
            free = c._replace(limit=0)
            assert not C.flat_mutant_applies(free, "bias", C.flat_plan(free), mutant)


# ---------------------------------------------------------------------------------------------------------------
# conv1_wide, clip_dz, sim_gemm
# ---------------------------------------------------------------------------------------------------------------
def test_wide_cases_give_the_compositions_they_are_named_for():
    by = {c.name: (c, C.wide_plan(c)) for c in C.WIDE_CASES}
    for name in ("w256_one_workgroup", "w320_one_workgroup", "w256_cin96_one_workgroup", "w512_one_workgroup"):
        c, p = by[name]
        assert c.limit == 1 and p.grid == 1 and len(p.tiles[0]) >= 2 and not p.xcd_map          # every tile, a prefetch under each epilogue
    assert len(by["w512_one_workgroup"][1].tiles[0]) == 4 and {ch for _, ch in by["w512_one_workgroup"][1].tiles[0]} == {0, 1}
    c, p = by["w320_grid3"]
    assert p.grid == 3 and not p.xcd_map and [len(t) for t in p.tiles] == [2, 1, 1]             # an uneven last round
    c, p = by["w256_xcd_grid8"]
    assert p.grid == 8 and p.xcd_map and p.n_rounds == 2 and [len(t) for t in p.tiles] == [2, 2, 2, 1, 1, 1, 1, 1]
    assert sum(len(t) for t in p.tiles) == 11 >= 9
    c, p = by["w512_xcd_grid16"]
    assert p.grid == 16 and p.xcd_map and (p.grid // 8) % 2 == 0 and sum(len(t) for t in p.tiles) == 22
    assert [len(t) for t in p.tiles] == [2, 2, 2, 1, 1, 1, 1, 1] * 2
    for c, p in by.values():                                                                     # every tile exactly once
        s = c.shape
        n_row, n_ch = P.ceil_div(s.B * 146, 256), s.cout // C.wide_tn(c)
        assert sorted(t for mine in p.tiles for t in mine) == [(r, ch) for r in range(n_row) for ch in range(n_ch)]
        free = C.wide_plan(c._replace(limit=0))
        assert all(len(t) == 1 for t in free.tiles)                                              # no limit: `have_next` is never true
    assert {C.wide_tn(c) for c in C.WIDE_CASES} == {256, 320} and {c.shape.cin for c in C.WIDE_CASES} == {64, 96}


@pytest.mark.parametrize("regime,dtype", ALL16)
def test_wide_cases_meet_their_regime_and_the_prefetch_mutant_is_caught(regime, dtype):
    meant = 0
    for c in C.WIDE_CASES:
        case = C.wide_case(c, regime, dtype)
        X.operand(case.x, dtype), X.operand(case.w, dtype)
        want = X.conv_expected(case, "bias")
        X.check_regime(want, regime, dtype, f"conv1 wide {c.name}")
        plan = C.wide_plan(c)
        X.assert_same(C.wide_emulation(c, case, dtype, plan), X.store(want, dtype), c.name)
        if regime == "exact" and C.wide_tn(c) == 256:
            assert float(X.row_sumsq_ref(want).max()) < 2 ** 24
        if C.wide_mutant_applies(c, plan):
            assert differs(C.wide_emulation(c, case, dtype, plan, "next_tile_prefetch_clobbers"), X.store(want, dtype)), c.name
            meant += 1
    assert meant == len(C.WIDE_CASES) - 1                   # all but the Cin = 96 case, whose last 32 padded channels are zeros


def test_dz_cases_give_the_compositions_they_are_named_for():
    for c in C.DZ_CASES:
        s = c.shape
        tiled, kt, ntiles, gx, jblocks = plan = C.dz_plan(c)
        assert tiled == ("tiled" in c.name or (c.split is None and s.Bm >= 256))
        assert (s.Bm <= 256 and C.dz_row_elems(s) % 64 == 0) or tiled
        if c.split is not None:
            assert C.dz_split(plan) == c.split, (c.name, C.dz_split(plan))
            assert jblocks == (2 if "column_blocks" in c.name else 1) and ntiles <= 27
        assert max(C.dz_split(plan)) >= 2                                                        # `more` / `next < ntiles` is true
        free = C.dz_plan(c._replace(limit=0))
        assert max(C.dz_split(free)) == 1                                                        # no limit: never
    assert {c.shape.Bn > 256 for c in C.DZ_CASES if "registers" in c.name} == {True, False}
    assert {c.shape.Bn > 256 for c in C.DZ_CASES if "tiled" in c.name} == {True, False}


@pytest.mark.parametrize("regime,dtype", ALL16)
def test_dz_cases_meet_their_regime_and_the_prefetch_mutant_is_caught(regime, dtype):
    for c in C.DZ_CASES:
        case = C.dz_case(c, regime, dtype)
        X.check_regime(case.ref, regime, dtype, f"clip_dz {c.name}")
        for t in (case.G, case.Y, case.Z):
            X.operand(t, dtype)
        plan = C.dz_plan(c)
        X.assert_same(C.dz_emulation(case, dtype, plan), X.store(case.ref, dtype), c.name)
        assert differs(C.dz_emulation(case, dtype, plan, "next_tile_prefetch_clobbers"), X.store(case.ref, dtype)), c.name


def test_sim_gemm_split_counts_and_the_witness_shape():
    counts = [(P.sim_ksplit(s.M, s.N, s.K, P.effective_cus(C.SIM_LIMIT)), P.sim_ksplit(s.M, s.N, s.K, P.DEVICE_CUS)) for s in X.SIM_SHAPES]
    # the split count is ceil(cus / tiles) in multiples of 8, capped by the K-steps: it can differ only where K has more than 8
    assert counts == [(8, 16), (8, 8), (4, 4)]
    for s, (a, b) in zip(X.SIM_SHAPES, counts):
        assert (a != b) == (s.K // 32 > 8)
    assert [C.witness_ksplit(n) for n in (1, 2, 3, 8, 16, 256)] == [8, 8, 8, 8, 16, 64]


# ---------------------------------------------------------------------------------------------------------------
# the gathers, the robust statistics
# ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("width", sorted(C.GATHER_UTYPES))
def test_gather_cases_make_several_trips_and_the_dropped_trip_is_caught(width):
    utype = C.GATHER_UTYPES[width]
    cus = P.effective_cus(C.GATHER_LIMIT)
    for case, ref, per_lane in ((C.gather_samples_case(utype), C.gather_samples_ref, 4), (C.gather_windows_case(utype), C.gather_windows_ref, 8)):
        assert case["B"] >= 8
        bx = P.gather_bx(case["vecs"], case["B"], cus, per_lane)
        trips, _ = P.gather_trips(case["vecs"], bx)
        assert bx == 1 and trips >= 3 and case["vecs"] % (bx * 256) != 0, (width, case["vecs"])
        free = P.gather_bx(case["vecs"], case["B"], P.DEVICE_CUS, per_lane)
        assert P.gather_trips(case["vecs"], free)[0] <= per_lane                                 # no limit: the unrolled trips at most
        idx = case["idx"]
        assert len(set(idx.tolist())) < len(idx) and bool((np.diff(idx) < 0).any())              # duplicates, a reversed stretch
        good, bad = ref(case), ref(case, "stride_trip_dropped", bx)
        assert not np.array_equal(good, bad)
        assert (good == K.FILL[np.dtype(utype)]).sum() < (bad == K.FILL[np.dtype(utype)]).sum()
    s, w = C.gather_samples_case(utype), C.gather_windows_case(utype)
    assert s["idx"].min() == 0 and s["idx"].max() == C.GS["N"] - 1                               # inside the table: no range check there
    M, L = len(w["starts"]), w["table"].shape[0]
    assert (w["idx"] < 0).any() and (w["idx"] >= M).any()                                        # candidates outside [0, M)
    picked = w["starts"][w["idx"][(w["idx"] >= 0) & (w["idx"] < M)]]
    assert (picked < 0).any() and (picked > L - w["T"]).any() and (picked == L - w["T"]).any() and (picked == 0).any()


def test_robust_cases_give_the_slices_they_are_named_for():
    for c in C.ROBUST_CASES:
        p = C.robust_plan(c)
        rows = c.C if c.pooled else c.S * c.C
        N = c.S * c.L if c.pooled else c.L
        assert rows >= 8 and N % 4 == 1
        if c.limit == 1:
            assert p.slices == 1 and p.grid_x == 1 and p.share == N >= 3 * P.RS_WG_ELEMS       # one workgroup, several 4096-sample shares
        else:
            assert 1 < p.slices < p.most and p.grid_x == p.slices
            if c.pooled:
                assert p.share % c.L != 0 and p.share > c.L                                      # a slice runs across a chunk's end
        assert C.robust_plan(c._replace(limit=0)).slices == p.most                               # no limit: one share each
        Xr = C.robust_input(c)
        assert Xr.shape == (c.S, c.C, c.L) and Xr.dtype == np.float32
        r = Xr.transpose(1, 0, 2).reshape(c.C, -1) if c.pooled else Xr.reshape(rows, -1)
        assert all(len(np.unique(row)) == N for row in r)
