"""The persistent kernels' multi-tile runs on a real MI355X, at small shapes and exactly.

conv3_flat, conv1_flat, conv1_wide, the two clip_dz kernels, the two gathers and the robust statistics size their grids from
the CU count; on 256 CUs every small shape is one tile per workgroup, so the flat kernels' 256-row tile, the prefetch of the
next tile under an epilogue and second grid-stride trips never met a reference.  Here each case of tests/persistent_cases.py
runs under tests/cu_limit.cu_limit(n), which makes launches from this thread plan for n CUs, and the outputs are compared
with the exact-arithmetic references of tests/exact_cases.py by torch.equal — no tolerance.  tests/test_persistent_runs_cpu.py
proves on the CPU which run composition each case gives and that the planted mutants of such kernels fail them.

Witnesses that the intended path ran are asserted BEFORE the comparison: for the flat kernels with statistics in 16-bit storage
the `stats` rows the mirror names as second halves of 256-row tiles are zero in both planes and no other row is (fp32 storage in
conv3_flat: none is); everywhere, inside the `with` block, sda_sim_gemm_ksplit on a fixed shape returns the value of the limit."""
import time

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from tests import cu_limit as P               # noqa: E402
from tests import exact_cases as X            # noqa: E402
from tests import persistent_cases as C       # noqa: E402
from tests import subject_pipeline as SP      # noqa: E402
from tests import test_exact_gpu as E         # noqa: E402
from tests import track_feed_cases as K       # noqa: E402
from tests.test_exact_gpu import DEV, NAN, name, padding_is_zero, rows, unrows, weight      # noqa: E402


@pytest.fixture(scope="module")
def ops():
    from speech_decoding_amd import ops as _ops
    from speech_decoding_amd import lib
    lib.load()
    assert torch.cuda.is_available(), "these tests need the MI355X"
    return _ops


@pytest.fixture(scope="module", autouse=True)
def no_limit_is_left_behind():
    t0 = time.time()
    assert P.clear_cu_limit() == 0, "a CU limit was in force before this module"
    yield
    print(f"\ntests/test_persistent_runs_gpu.py: {time.time() - t0:.1f} s wall")
    assert P.clear_cu_limit() == 0, "a test of this module left its CU limit in force"


def device_cus():
    return torch.cuda.get_device_properties(0).multi_processor_count


def limit_in_force(n):
    """inside `with cu_limit(n)`: this thread's launches plan for min(n, device CUs) — the library's K split of a fixed shape follows"""
    from speech_decoding_amd import lib as L, ops
    got = L.load().sda_sim_gemm_ksplit(*C.WITNESS_SHAPE, ops.dt_code(torch.bfloat16))
    assert got == C.witness_ksplit(P.effective_cus(n, device_cus())) != C.witness_ksplit(device_cus()), (n, got)
    return True


def ids(cases):
    return [c.name for c in cases]


# ---------------------------------------------------------------------------------------------------------------
# the flat kernels
# ---------------------------------------------------------------------------------------------------------------
def assert_pair_rows_are_the_zero_rows(stats, plan, cout, fp32_tiles, what):
    """the witness: `stats` rows (both planes, every channel) that are exactly zero = the second halves of 256-row tiles"""
    assert not bool(torch.isnan(stats).any()), what + ": a statistics row was not written"
    zero = [u for u in range(stats.shape[0]) if not bool(stats[u, :, :cout].any())]
    assert zero == ([] if fp32_tiles else P.flat_second_halves(plan)), f"{what}: zero statistics rows {zero}, plan {plan.runs}"


@pytest.mark.parametrize("dtype", X.DTYPES, ids=name)
@pytest.mark.parametrize("regime", X.REGIMES)
@pytest.mark.parametrize("c", C.FLAT3_CASES, ids=ids(C.FLAT3_CASES))
def test_conv3_flat_runs_of_several_tiles(ops, c, regime, dtype):
    """conv3_flat under a CU limit: runs of 1 to 5 units (256-row tiles, back to back, with and without a 128-row tail), a
    shorter last run, a partial last unit in the second half of a 256-row tile, both branches of xcd_block_order — bare, with
    bias, with bias + residual, statistics with the last two."""
    from speech_decoding_amd import lib as L
    case = C.flat_case(c, regime, dtype)
    s = case.shape
    Cin_p, Cout_p = L.pad_channels(s.cin), L.pad_channels(s.cout)
    fp32 = dtype == torch.float32
    plan = C.flat_plan(c, device_cus(), fp32=fp32)
    assert tuple(sum(t // 128 for t in r) for r in plan.runs) == c.runs and plan.grid == len(c.runs) * (Cout_p // 160)
    flags = L.CONV_FLAT_TILES | (L.CONV_ONE_PER_CU if c.one_per_cu else 0)
    assert ops.conv_kernel(3, Cout_p, flags, dtype) == L.CONV_KERNEL_FLAT3
    xb = rows(ops, case.x, dtype)
    wp = weight(ops, case.w, Cout_p, Cin_p, dtype)
    bias = ops.pack_vector(case.bias.float().to(DEV), Cout_p)
    n_units = ops.conv_stats_rows(s.B, s.T, 3, Cout_p, flags)
    assert n_units == sum(c.runs)
    for epi in C.epilogues(case):
        what = f"conv3_flat {c.name} {regime} {name(dtype)} {epi}"
        want = X.store(X.conv_expected(case, epi), dtype)
        yb = ops.new_rows(s.B, s.T, Cout_p, dtype, DEV)
        stats = None if epi == "bare" else torch.full((n_units, 2, Cout_p), NAN, device=DEV)
        with P.cu_limit(c.limit):
            assert limit_in_force(c.limit)
            ops.conv_gemm(xb, wp, yb, B=s.B, T=s.T, KS=3, dil=s.dil, bias=None if epi == "bare" else bias,
                          res=xb if epi == "bias_res" else None, stats=stats, flags=flags)
        if stats is not None:
            assert_pair_rows_are_the_zero_rows(stats.cpu(), plan, s.cout, fp32, what)
        X.assert_same(unrows(ops, yb, s.B, s.cout, s.T), want, what)
        assert padding_is_zero(yb, s.B, s.cout, s.T), what
        if stats is not None and regime == "exact":
            assert float(want.abs().sum(dim=(0, 2)).max()) < 2 ** 24
            X.assert_same(stats[:, 0, :s.cout].double().sum(0).cpu(), want.sum(dim=(0, 2)), what + " stats sums", axes="c")


@pytest.mark.parametrize("dtype", X.DTYPES, ids=name)
@pytest.mark.parametrize("regime", X.REGIMES)
def test_conv3_flat_glu_epilogue_over_a_run_of_pairs(ops, regime, dtype):
    """SDA_EPI_GLU on the 600-channel case: under limit 1 every channel tile is one run of four units"""
    with P.cu_limit(C.GLU_LIMIT):
        assert limit_in_force(C.GLU_LIMIT)
        E.check_glu_gate(ops, regime, dtype)


@pytest.mark.parametrize("dtype", X.DTYPES, ids=name)
@pytest.mark.parametrize("regime", X.REGIMES)
@pytest.mark.parametrize("c", C.FLAT1_CASES, ids=ids(C.FLAT1_CASES))
def test_conv1_flat_runs_of_several_tiles(ops, c, regime, dtype):
    """conv1_flat under a CU limit (256-row tiles in every storage type): conv + bias as stored, bare, and as the pre-activation
    kept under SDA_EPI_GELU; SDA_EPI_ROW_SUMSQ on the 128-channel width in the exact regime."""
    from speech_decoding_amd import lib as L
    case = C.flat_case(c, regime, dtype)
    s = case.shape
    Cin_p, Cout_p = L.pad_channels(s.cin), L.pad_channels(s.cout)
    plan = C.flat_plan(c, device_cus())
    assert tuple(sum(t // 128 for t in r) for r in plan.runs) == c.runs and plan.grid == len(c.runs) * (Cout_p // C.flat_tile_co(c))
    flags = L.CONV_FLAT_TILES | (L.CONV_ONE_PER_CU if c.one_per_cu else 0)
    assert ops.conv_kernel(1, Cout_p, flags, dtype) == L.CONV_KERNEL_FLAT1
    xb = rows(ops, case.x, dtype)
    wp = weight(ops, case.w, Cout_p, Cin_p, dtype)
    bias = ops.pack_vector(case.bias.float().to(DEV), Cout_p)
    kw = dict(B=s.B, T=s.T, KS=1, dil=0, flags=flags)
    for epi in ("bare", "bias"):
        what = f"conv1_flat {c.name} {regime} {name(dtype)} {epi}"
        want = X.store(X.conv_expected(case, epi), dtype)
        b = None if epi == "bare" else bias
        yb, post, pre = (ops.new_rows(s.B, s.T, Cout_p, dtype, DEV) for _ in range(3))
        with P.cu_limit(c.limit):
            assert limit_in_force(c.limit)
            ops.conv_gemm(xb, wp, yb, bias=b, **kw)
            ops.conv_gemm(xb, wp, post, y_pre=pre, gelu=True, bias=b, **kw)
        X.assert_same(unrows(ops, yb, s.B, s.cout, s.T), want, what)
        assert padding_is_zero(yb, s.B, s.cout, s.T), what
        X.assert_same(unrows(ops, pre, s.B, s.cout, s.T), want, what + " y_pre under GELU")
        assert padding_is_zero(pre, s.B, s.cout, s.T) and padding_is_zero(post, s.B, s.cout, s.T), what
    if regime == "exact" and Cout_p % 128 == 0 and C.flat_tile_co(c) == 128:
        what = f"conv1_flat {c.name} {name(dtype)} row sums of squares"
        want = X.store(X.conv_expected(case, "bias"), dtype)
        parts = torch.full((L.rows_alloc(s.B, s.T), Cout_p // 128), NAN, device=DEV)
        with P.cu_limit(c.limit):
            assert limit_in_force(c.limit)
            yb = ops.conv_gemm(xb, wp, ops.new_rows(s.B, s.T, Cout_p, dtype, DEV), bias=bias, row_sumsq=parts, **kw)
        X.assert_same(unrows(ops, yb, s.B, s.cout, s.T), want, what)
        ref = X.row_sumsq_ref(want)
        assert float(ref.max()) < 2 ** 24
        Tp = L.rows_tp(s.T)
        got = torch.stack([parts[b * Tp + L.ROW_PAD: b * Tp + L.ROW_PAD + s.T] for b in range(s.B)]).cpu()
        X.assert_same(got, ref, what, axes="btj")


# ---------------------------------------------------------------------------------------------------------------
# conv1_wide
# ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", X.DTYPES16, ids=name)
@pytest.mark.parametrize("regime", X.REGIMES)
@pytest.mark.parametrize("c", C.WIDE_CASES, ids=ids(C.WIDE_CASES))
def test_conv1_wide_walks_its_tiles_with_the_prefetch_under_the_epilogue(ops, c, regime, dtype):
    """conv1_wide under a CU limit: one workgroup over every tile, a grid of 3 with an uneven last round, the XCD-aware map with a
    ragged second round and with two channel tiles — conv + bias, the pre-activation under GELU, and SDA_EPI_ROW_SUMSQ on the
    256-channel tiles in the exact regime."""
    from speech_decoding_amd import lib as L
    case = C.wide_case(c, regime, dtype)
    s = case.shape
    Cin_p, Cout_p = L.pad_channels(s.cin), L.pad_channels(s.cout)
    plan, free = C.wide_plan(c, device_cus()), C.wide_plan(c._replace(limit=0), device_cus())
    assert plan == C.wide_plan(c) and max(len(t) for t in plan.tiles) >= 2 and max(len(t) for t in free.tiles) == 1
    assert ops.conv_kernel(1, Cout_p, L.CONV_WIDE_TILES, dtype) == L.CONV_KERNEL_WIDE
    xb = rows(ops, case.x, dtype)
    wp = weight(ops, case.w, Cout_p, Cin_p, dtype)
    bias = ops.pack_vector(case.bias.float().to(DEV), Cout_p)
    want = X.store(case.ref, dtype)
    kw = dict(B=s.B, T=s.T, KS=1, dil=0, bias=bias, flags=L.CONV_WIDE_TILES)
    what = f"conv1_wide {c.name} {regime} {name(dtype)}"
    yb, post, pre = (ops.new_rows(s.B, s.T, Cout_p, dtype, DEV) for _ in range(3))
    rsq = regime == "exact" and C.wide_tn(c) == 256
    parts = torch.full((L.rows_alloc(s.B, s.T), Cout_p // 128), NAN, device=DEV) if rsq else None
    ysq = ops.new_rows(s.B, s.T, Cout_p, dtype, DEV)
    with P.cu_limit(c.limit):
        assert limit_in_force(c.limit)
        ops.conv_gemm(xb, wp, yb, **kw)
        ops.conv_gemm(xb, wp, post, y_pre=pre, gelu=True, **kw)
        if rsq:
            ops.conv_gemm(xb, wp, ysq, row_sumsq=parts, **kw)
    X.assert_same(unrows(ops, yb, s.B, s.cout, s.T), want, what)
    assert padding_is_zero(yb, s.B, s.cout, s.T), what
    X.assert_same(unrows(ops, pre, s.B, s.cout, s.T), want, what + " y_pre under GELU")
    assert padding_is_zero(pre, s.B, s.cout, s.T) and padding_is_zero(post, s.B, s.cout, s.T), what
    if rsq:
        X.assert_same(unrows(ops, ysq, s.B, s.cout, s.T), want, what + " with row sums of squares")
        ref = X.row_sumsq_ref(want)
        assert float(ref.max()) < 2 ** 24
        Tp = L.rows_tp(s.T)
        got = torch.stack([parts[b * Tp + L.ROW_PAD: b * Tp + L.ROW_PAD + s.T] for b in range(s.B)]).cpu()
        X.assert_same(got, ref, what + " row sums of squares", axes="btj")


# ---------------------------------------------------------------------------------------------------------------
# the epilogues that are not integer-exact: the bodies of tests/test_kernels_gpu.py, their references and tolerances, under a limit
# ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("limit", [1, 2])
@pytest.mark.parametrize("dtype", X.DTYPES, ids=name)
@pytest.mark.parametrize("cin,cout,T,B", [(128, 256, 77, 3), (64, 320, 130, 6)])
def test_conv1_flat_gelu_backward_epilogue_over_runs(ops, limit, dtype, cin, cout, T, B):
    from tests import test_kernels_gpu as KG
    n_co = cout // (160 if cout % 160 == 0 else 128)
    plan = P.flat_runs(P.flat_units(B, T), n_co, P.effective_cus(limit, device_cus()), False)
    assert any(256 in r for r in plan.runs)
    with P.cu_limit(limit):
        assert limit_in_force(limit)
        KG.check_conv1_flat_gelu_backward_epilogue(ops, dtype, cin, cout, T, B)


@pytest.mark.parametrize("limit", [1, 3])
@pytest.mark.parametrize("dtype", X.DTYPES16, ids=name)
@pytest.mark.parametrize("cin,cout,T,B", [(128, 256, 77, 3), (64, 320, 130, 6)])
def test_conv1_wide_gelu_backward_epilogue_over_tiles(ops, limit, dtype, cin, cout, T, B):
    from tests import test_kernels_gpu as KG
    plan = P.wide_tiles(P.ceil_div(B * (T + 16), 256), 1, P.effective_cus(limit, device_cus()))
    assert max(len(t) for t in plan.tiles) >= 2 or limit == 3
    with P.cu_limit(limit):
        assert limit_in_force(limit)
        KG.check_conv1_wide_gelu_backward_epilogue(ops, dtype, cin, cout, T, B)


@pytest.mark.parametrize("limit", [1, 2])
@pytest.mark.parametrize("dtype", X.DTYPES, ids=name)
@pytest.mark.parametrize("cin,cout,dil,T", [(640, 320, 2, 300), (320, 320, 8, 360)])
def test_conv3_bn_backward_statistics_epilogue_over_runs(ops, limit, dtype, cin, cout, dil, T):
    from speech_decoding_amd import lib as L
    from tests import test_kernels_gpu as KG
    plan = P.flat_runs(P.flat_units(3, T), cout // 160, P.effective_cus(limit, device_cus()), False, fp32=dtype == torch.float32)
    assert plan.units_per_wg >= 4
    with P.cu_limit(limit):
        assert limit_in_force(limit)
        KG.check_conv3_bn_backward_statistics_epilogue(ops, dtype, cin, cout, dil, T, L.CONV_FLAT_TILES)


@pytest.mark.parametrize("limit", [1, 2])
@pytest.mark.parametrize("dtype", X.DTYPES, ids=name)
@pytest.mark.parametrize("regime", X.REGIMES)
@pytest.mark.parametrize("i", [2, 4], ids=lambda i: "x".join(map(str, X.DGRAD_SHAPES[i])))
def test_data_gradient_on_flat_tiles_over_runs(ops, i, regime, dtype, limit):
    """the DGRAD_SHAPES that the flat kernels serve (320 input channels for k = 3, 128 padded for k = 1), 3 units: one run of
    three under limit 1, runs of two and one under limit 2 (k = 3, two channel tiles)"""
    from speech_decoding_amd import lib as L
    s = X.DGRAD_SHAPES[i]
    Cin_p = L.pad_channels(s.cin)
    assert ops.conv_kernel(s.KS, Cin_p, L.CONV_FLAT_TILES, dtype) == (L.CONV_KERNEL_FLAT3 if s.KS == 3 else L.CONV_KERNEL_FLAT1)
    tile = 160 if Cin_p % 160 == 0 else 128
    plans = [P.flat_runs(P.flat_units(s.B, s.T), Cin_p // tile, P.effective_cus(limit, device_cus()), one) for one in (False, True)]
    assert any(256 in r for plan in plans for r in plan.runs)
    with P.cu_limit(limit):
        assert limit_in_force(limit)
        E.check_data_gradient(ops, i, regime, dtype, (L.CONV_FLAT_TILES, L.CONV_FLAT_TILES | L.CONV_ONE_PER_CU))


# ---------------------------------------------------------------------------------------------------------------
# the loss's dZ, the similarity GEMM
# ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", X.DTYPES16, ids=name)
@pytest.mark.parametrize("regime", X.REGIMES)
@pytest.mark.parametrize("c", C.DZ_CASES, ids=ids(C.DZ_CASES))
def test_clip_dz_walks_several_tiles_per_workgroup(ops, c, regime, dtype):
    """sda_clip_dz under a CU limit, both forms: the double-buffered stage of the register form (27 tiles split 14 / 13, or all
    on one workgroup per column block) and the tiled form's prefetch under the epilogue (11 tiles on one workgroup, 6 / 5)"""
    from speech_decoding_amd import lib as L
    case = C.dz_case(c, regime, dtype)
    s = case.shape
    Yt, Zt = rows(ops, case.Y, dtype), rows(ops, case.Z, dtype)
    Fp = Yt.shape[1]
    re = L.rows_tp(s.T) * Fp
    assert re == C.dz_row_elems(s) and L.load().sda_clip_dz_supported(s.Bm, s.Bn, re, ops.dt_code(dtype))
    plan = C.dz_plan(c, device_cus())
    assert plan == C.dz_plan(c) and max(C.dz_split(plan)) >= 2 and (c.split is None or C.dz_split(plan) == c.split)
    G = torch.zeros((s.Bm + 1, L.pad_channels(s.Bn)), dtype=dtype, device=DEV)
    G[:s.Bm, :s.Bn] = X.operand(case.G, dtype).to(DEV)
    cs, rs = case.cscale.float().to(DEV), case.rscale.float().to(DEV)
    scale = torch.tensor([case.out_scale], device=DEV)
    want = X.store(case.ref, dtype)
    what = f"clip_dz {c.name} {regime} {name(dtype)}"
    out = ops.new_rows_uninit(s.Bn, s.T, Fp, dtype, DEV)
    with P.cu_limit(c.limit):
        assert limit_in_force(c.limit)
        ops.clip_dz(G, Yt, Zt, out, rs, cs, Bm=s.Bm, Bn=s.Bn, row_elems=re, out_scale=scale)
    X.assert_same(ops.rows_view(out, s.Bn, s.F, s.T).cpu().double(), want, what)
    full, Tp = out.float().cpu(), L.rows_tp(s.T)
    for b in range(s.Bn):
        assert bool((full[b * Tp: b * Tp + L.ROW_PAD] == 0).all()), what
    assert Fp == s.F or bool((full[:, s.F:] == 0).all()), what


@pytest.mark.parametrize("dtype", X.DTYPES16, ids=name)
@pytest.mark.parametrize("i", range(len(X.SIM_SHAPES)), ids=lambda i: "x".join(map(str, X.SIM_SHAPES[i])))
def test_sim_gemm_at_the_split_counts_of_a_limit_and_of_none(ops, i, dtype):
    """sda_sim_gemm at the K split sda_sim_gemm_ksplit returns under limit 1 and under no limit; the two counts are the mirror's,
    and they differ wherever the contraction has more than 8 K-steps (the count comes in multiples of 8, capped by the K-steps)"""
    from speech_decoding_amd import lib as L
    s = X.SIM_SHAPES[i]
    A, Bm, ref = X.sim_case(i)
    Np = L.pad_channels(s.N)
    xm = torch.full((s.M, s.pitch), 7.0, dtype=dtype, device=DEV)
    wm = torch.full((s.N, s.pitch), 7.0, dtype=dtype, device=DEV)
    xm[:, :s.K], wm[:, :s.K] = X.operand(A, dtype).to(DEV), X.operand(Bm, dtype).to(DEV)
    free = L.load().sda_sim_gemm_ksplit(s.M, s.N, s.K, ops.dt_code(dtype))
    with P.cu_limit(C.SIM_LIMIT):
        assert limit_in_force(C.SIM_LIMIT)
        limited = L.load().sda_sim_gemm_ksplit(s.M, s.N, s.K, ops.dt_code(dtype))
    assert limited == P.sim_ksplit(s.M, s.N, s.K, 1) and free == P.sim_ksplit(s.M, s.N, s.K, device_cus())
    assert (limited != free) == (s.K // 32 > 8), (limited, free)
    if i == 0:
        assert limited != free
    for ks in (limited, free):
        partial = torch.full((ks, s.M, Np), NAN, device=DEV)
        out = torch.full((s.M, Np), NAN, device=DEV)
        with P.cu_limit(C.SIM_LIMIT):
            ops.matmul_nt_splitk_into(xm, wm, s.M, s.N, s.K, s.pitch, True, ks, partial, out)
        X.assert_same(out[:, :s.N].cpu().double(), ref, f"sim_gemm {tuple(s)} {name(dtype)} ksplit={ks}", axes="ij")


# ---------------------------------------------------------------------------------------------------------------
# the gathers
# ---------------------------------------------------------------------------------------------------------------
INT = {np.dtype(np.uint16): (np.int16, torch.int16), np.dtype(np.uint32): (np.int32, torch.int32)}
DT = {"bf16": torch.bfloat16, "fp16": torch.float16, "fp32": torch.float32}


def to_dev(u, dtype=None):
    t = torch.from_numpy(np.ascontiguousarray(u).view(INT[u.dtype][0])).to(DEV)
    return t if dtype is None else t.view(dtype)


def bits(t, utype):
    return t.contiguous().view(INT[np.dtype(utype)][1]).cpu().numpy().view(utype)


def filled(c, utype):
    from speech_decoding_amd import lib as L
    return torch.full((L.rows_alloc(c["B"], c["T"]), c["Cp"]), K.FILL[np.dtype(utype)], dtype=INT[np.dtype(utype)][1], device=DEV)


@pytest.mark.parametrize("width", sorted(C.GATHER_UTYPES))
def test_gather_samples_makes_several_trips_per_block(ops, width):
    """sda_gather_samples under limit 1: one block per sample walks its 4 to 9 trips of 256 vectors (the four-fold loop and its
    tail) — into a destination of NaN patterns, equal to index_select of the table's samples; nothing behind the last sample is
    written.  Then ops.gather_samples in the storage type: the same samples, zero pad rows and slack."""
    from speech_decoding_amd import lib as L
    utype = C.GATHER_UTYPES[width]
    c = C.gather_samples_case(utype)
    bx = P.gather_bx(c["vecs"], c["B"], P.effective_cus(C.GATHER_LIMIT, device_cus()), 4)
    assert bx == 1 and P.gather_trips(c["vecs"], bx)[0] >= 3 and c["vecs"] % 256
    want = C.gather_samples_ref(c)
    table, idx, dst = to_dev(c["table"]), torch.from_numpy(c["idx"]).to(DEV), filled(c, utype)
    with P.cu_limit(C.GATHER_LIMIT):
        assert limit_in_force(C.GATHER_LIMIT)
        L.check(L.load().sda_gather_samples(table.data_ptr(), idx.data_ptr(), dst.data_ptr(), c["B"], c["vecs"] * 16,
                                            torch.cuda.current_stream().cuda_stream), "gather_samples")
        out = ops.gather_samples(table.view(DT[width]), idx, c["B"], c["T"])
    assert torch.equal(dst, to_dev(want))
    Tp, n = c["T"] + 16, c["B"] * (c["T"] + 16)
    picked = table[:C.GS["N"] * Tp].view(C.GS["N"], Tp, c["Cp"]).index_select(0, idx).reshape(n, c["Cp"])
    got = out.view(INT[np.dtype(utype)][1])
    assert torch.equal(got[:n], picked) and not bool(got[n:].any())
    assert all(not bool(got[b * Tp: b * Tp + 16].any()) for b in range(c["B"]))


@pytest.mark.parametrize("width", sorted(C.GATHER_UTYPES))
def test_gather_windows_makes_several_trips_per_block(ops, width):
    """sda_gather_windows under limit 1 (one block per sample, 4 to 7 trips, the slack shared out in second trips too), with
    duplicate and reversed candidates, candidates outside [0, M) and starts outside the table: every byte of a destination of NaN
    patterns is written, windows equal index_select of the table's rows, everything else is zero."""
    from speech_decoding_amd import lib as L
    utype = C.GATHER_UTYPES[width]
    c = C.gather_windows_case(utype)
    bx = P.gather_bx(c["vecs"], c["B"], P.effective_cus(C.GATHER_LIMIT, device_cus()), 8)
    assert bx == 1 and P.gather_trips(c["vecs"], bx)[0] >= 3 and c["vecs"] % 256
    want = C.gather_windows_ref(c)
    assert not (want == K.FILL[np.dtype(utype)]).any()
    table, idx, starts, dst = to_dev(c["table"]), torch.from_numpy(c["idx"]).to(DEV), torch.from_numpy(c["starts"]).to(DEV), filled(c, utype)
    with P.cu_limit(C.GATHER_LIMIT):
        assert limit_in_force(C.GATHER_LIMIT)
        L.check(L.load().sda_gather_windows(table.data_ptr(), table.shape[0], starts.data_ptr(), starts.numel(), idx.data_ptr(),
                                            dst.data_ptr(), c["B"], c["T"], c["Cp"] * table.element_size(),
                                            torch.cuda.current_stream().cuda_stream), "gather_windows")
        out = ops.gather_windows(table.view(DT[width]), starts, idx, c["B"], c["T"])
    assert torch.equal(dst, to_dev(want))
    assert torch.equal(out.view(INT[np.dtype(utype)][1]), dst)
    # index_select plus zero padding, written here: valid candidates' windows are table rows, everything else is zero
    M, rows_, Tp = len(c["starts"]), table.shape[0], c["T"] + 16
    for b, m in enumerate(c["idx"].tolist()):
        s0 = int(c["starts"][m]) if 0 <= m < M else -1
        window = dst[b * Tp + 16: (b + 1) * Tp]
        assert not bool(dst[b * Tp: b * Tp + 16].any())
        if 0 <= s0 <= rows_ - c["T"]:
            assert torch.equal(window, table.index_select(0, torch.arange(s0, s0 + c["T"], device=DEV)))
        else:
            assert not bool(window.any())
    assert not bool(dst[c["B"] * Tp:].any())


# ---------------------------------------------------------------------------------------------------------------
# the robust statistics
# ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("c", C.ROBUST_CASES, ids=ids(C.ROBUST_CASES))
def test_robust_stats_with_one_and_two_slices_per_row(c):
    """sda_robust_stats under limits 1 (one workgroup per row over three shares of 4096 samples) and 2 (two slices of at most
    four), subject-wise and pooled.  Rows of 4k + 1 distinct integers: centre and scale are elements of the row (and one exact
    difference), equal to numpy's float64 percentiles rounded once; the scaled output within tests/test_subject_feed_gpu.py's
    bound of the restatement."""
    from speech_decoding_amd.collate import robust_stats, scale_clamp_rows
    plan = C.robust_plan(c, device_cus())
    assert plan == C.robust_plan(c) and (plan.slices == 1 if c.limit == 1 else 1 < plan.slices < plan.most)
    Xn = C.robust_input(c)
    Xd = torch.from_numpy(Xn).to(DEV)
    with P.cu_limit(c.limit):
        assert limit_in_force(c.limit)
        centre, scale = robust_stats(Xd, pooled=c.pooled)
    r = SP.pooled_rows(Xn) if c.pooled else Xn.reshape(c.S * c.C, c.L)
    q = np.percentile(r.astype(np.float64), [25, 50, 75], axis=1)
    assert np.array_equal(q.astype(np.float32), q)                               # integer positions: elements of the row
    wc, ws = q[1].astype(np.float32), (q[2] - q[0]).astype(np.float32)
    assert (ws != 0).all()
    assert np.array_equal(centre.cpu().numpy().reshape(-1), wc) and np.array_equal(scale.cpu().numpy().reshape(-1), ws)
    pc, ps = SP.robust_stats(Xn, not c.pooled)
    assert np.array_equal(pc.reshape(-1), wc) and np.array_equal(ps.reshape(-1), ws)
    got = scale_clamp_rows(Xd, centre, scale, 20.0, True, pooled=c.pooled)
    np.testing.assert_allclose(got.cpu().numpy(), SP.scale_clamp(Xn, pc, ps, 20.0, True), rtol=1e-5, atol=1e-5)
