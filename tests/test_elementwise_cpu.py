"""What tests/test_elementwise_gpu.py relies on, shown without a GPU:
1. the cases of tests/elementwise_cases.py reach the edges they are named for (the geometry is recomputed from the kernels' own
   formulas and asserted);
2. the constants of the tolerance table are 4 x what the fp32 emulation of each device formula measures against float64;
3. the unmutated emulation of every kernel passes every case with the GPU test's own comparison code, and each of the 21
   planted bugs misses its tolerance by 10 x or more (an exactness check: is not equal) on the case recorded next to it;
4. host-side refusals: a width the kernels cannot take returns -1 with sda_last_error set before anything is launched (the
   pointers passed are host memory)."""
import ctypes
import math

import pytest
import torch

from tests import elementwise_cases as E

F32, BF16, F16 = torch.float32, torch.bfloat16, torch.float16
CAUGHT = {}          # mutant -> (case, ratio): which case catches which mutant, printed at the end


@pytest.fixture(scope="module", autouse=True)
def _report():
    yield
    print("\nmutant -> case that catches it (error / tolerance; inf = an exact comparison failed or NaN)")
    for m, (case, r) in sorted(CAUGHT.items()):
        print(f"  {m:24s} {case:48s} {r:.3g}")


def caught(mutant, case, r):
    assert r >= 10.0, (mutant, case, r)
    if mutant not in CAUGHT or CAUGHT[mutant][1] < r:
        CAUGHT[mutant] = (case, r)


def check_rows(got_rl, ref, tol, B, T):
    """(error / tolerance over the valid rows, every other row still holds the sentinel)"""
    idx = E.mem_rows(B, T)
    other = torch.ones(got_rl.shape[0], dtype=torch.bool)
    other[idx] = False
    return E.ratio(got_rl[idx], ref, tol), bool((got_rl[other] == E.SENT).all())


# ---------------------------------------------------------------------------------------------------------------
# 1. geometry
# ---------------------------------------------------------------------------------------------------------------
def test_row_cursor_counts_cover_every_batch_remainder():
    """U = 4 (bn_gelu_forward) and U = 2 (bn_gelu_backward apply, glu_forward): (5, 33, 128) alone gives n = 6, 7 in fp32 and
    n = 5, 6 in 16-bit storage (remainders 2, 3 and 1, 2 of 4; both of 2); the table as a whole gives all four in every dtype."""
    assert E.thread_row_counts(5, 33, 128, F32) == {6, 7}
    assert E.thread_row_counts(5, 33, 128, BF16) == {5, 6}
    for dtype in E.DTYPES:
        ns = set()
        for B, T, C in E.STREAM_SHAPES + (E.WIDE_SHAPE[dtype],):
            ns |= E.thread_row_counts(B, T, C, dtype)
        assert {n % 4 for n in ns} == {0, 1, 2, 3} and {n % 2 for n in ns} == {0, 1}, (dtype, ns)
        assert any(n >= 4 for n in ns)


def test_shapes_reach_the_edges_they_are_named_for():
    for dtype in E.DTYPES:
        CH = E.chunk(dtype)
        assert E.row_group(64 // CH) > 5                                         # (7, 5, 64): several wraps per step
        assert E.stream_blocks(7, 5, 64 // CH) == 1 and E.red_blocks(1, 1) == 1
        assert 256 % (320 // CH) != 0                                            # idle threads
        assert E.stream_blocks(3, 77, 320 // CH) > 1 and (3 * 77) % E.stream_blocks(3, 77, 320 // CH) != 0
        assert E.WIDE_SHAPE[dtype][2] // CH > 256 and E.WIDE_SHAPE[dtype][2] % 64 == 0
        B, T, C = E.stream_cap_shape(dtype)
        RG = E.row_group(C // CH)
        assert B * T > 2048 * 8 * RG and E.stream_blocks(B, T, C // CH) == 2048
        assert E.L.rows_alloc(B, T) * C * (4 if dtype == F32 else 2) < 100e6
    assert 1024 // 4 == 256 and E.row_group(256) == 1                            # (2, 9, 1024) in fp32: RG = 1
    B, T, C = E.REDUCE_CAP_SHAPE
    assert B * T > 32768 and E.red_blocks(B, T) == 1024
    assert 65540 // 4 > 64 * 256 and 252 // 4 < 64 and 256 // 4 == 64


# ---------------------------------------------------------------------------------------------------------------
# 2. the tolerance table
# ---------------------------------------------------------------------------------------------------------------
def _sweep_inputs():
    return torch.cat([E.finite_values(BF16), E.finite_values(F16), E.loguniform_values()])


def _measure():
    x = _sweep_inputs()
    out = {}
    worst = lambda f, ref, mag: max(float(((f(hw).double() - ref).abs() / mag).max()) for hw in E.HW_VARIANTS)
    mag = x.double().abs().clamp(min=1.0)
    out["C_GELU16"] = worst(lambda hw: E.gelu_emul(x, BF16, hw), E.gelu64(x), mag)
    out["C_GGRAD16"] = worst(lambda hw: E.ggrad_emul(x, BF16, hw), E.ggrad64(x), 1.0)
    out["C_GELU32"] = worst(lambda hw: E.gelu_emul(x, F32, hw), E.gelu64(x), mag)
    out["C_GGRAD32"] = worst(lambda hw: E.ggrad_emul(x, F32, hw), E.ggrad64(x), 1.0)
    sg = E.sig64(x)
    keep = sg >= E.FTZ                      # below fp32's smallest normal the instruction may flush: the 2^-126 term, not C_SIG
    out["C_SIG"] = worst(lambda hw: E.sigmoid_emul(x, hw)[keep], sg[keep], (mag * sg)[keep])
    return out


def _measure_bn():
    worst = 0.0
    for dtype in E.DTYPES:
        case = E.bn_backward_case(4, 40, 64, dtype, designed=True)
        r = E.ref_bn_backward(case, dtype, dg_form=True)
        got = E.emul_bn_backward_apply(case, r["mean"].float(), r["rstd"].float(), r["dgamma"].float(), r["dbeta"].float(), dtype,
                                       True, dg=r["dg"])
        mag = (r["a"] * r["dg"]).abs() + r["p"].abs() + (r["q"] * case["x"].double()).abs()
        ok = mag > 0
        worst = max(worst, float(((got.double() - r["dx"]).abs()[ok.expand_as(got)] / mag.expand_as(got)[ok.expand_as(got)]).max()))
    return worst


def _adam_single(n=4096, steps=7, mutant=None):
    g = torch.Generator().manual_seed(3)
    p0 = torch.randn(n, generator=g)
    grads = [torch.randn(n, generator=g) * 10.0 ** float(torch.randint(-3, 4, (1,), generator=g)) for _ in range(steps)]
    p, m, v = p0.clone(), torch.zeros(n), torch.zeros(n)
    pr = torch.nn.Parameter(p0.double())
    opt = torch.optim.Adam([pr], lr=1e-3)
    got, ref = [], []
    for k, gk in enumerate(grads, 1):
        p, m, v = E.emul_adam(p, gk, m, v, k, mutant=mutant)
        pr.grad = gk.double()
        opt.step()
        got.append((p, m, v))
        ref.append((pr.detach().clone(), opt.state[pr]["exp_avg"].clone(), opt.state[pr]["exp_avg_sq"].clone()))
    return grads, p0, got, ref


def test_tolerance_table_matches_the_emulation():
    """chosen constant = 4 x measured, rounded up by at most a quarter"""
    m = _measure()
    m["C_BN"] = _measure_bn()
    print("\nmeasured on the CPU (fp32 emulation against float64, exp2 / rcp moved by -1, 0, +1 ulp) and chosen:")
    chosen = dict(C_GELU16=E.C_GELU16, C_GGRAD16=E.C_GGRAD16, C_GELU32=E.C_GELU32, C_GGRAD32=E.C_GGRAD32, C_SIG=E.C_SIG, C_BN=E.C_BN)
    for k, v in m.items():
        print(f"  {k:10s} measured {v:.3e} ({v / E.U32:.2f} u)  chosen {chosen[k]:.3e}")
    for k, v in m.items():
        assert 4.0 * v <= chosen[k] <= 5.0 * v, (k, v, chosen[k])
    # sd_common.h's statement about the 16-bit form: Abramowitz-Stegun's 7.5e-8 plus fp32 evaluation
    assert m["C_GELU16"] <= 7.5e-8 + 2 * E.U32


def test_adam_constant_is_four_times_the_measured_rounding():
    """C_ADAM: the emulated fp32 update against float64 Adam, in units of the bound's own magnitudes with C_ADAM = 1 u"""
    grads, p0, got, ref = _adam_single()
    z = torch.zeros_like(p0)
    saved, E.C_ADAM = E.C_ADAM, E.U32
    try:
        tols = E.adam_tolerances(grads, p0, z, z, 0)
    finally:
        E.C_ADAM = saved
    worst = max(E.ratio(got[k][i], ref[k][i], tols[k][i]) for k in range(len(grads)) for i in range(3))
    print(f"\n  C_ADAM     measured {worst:.2f} u  chosen {E.C_ADAM / E.U32:.1f} u")
    assert 4.0 * worst <= E.C_ADAM / E.U32 <= 5.0 * worst


# ---------------------------------------------------------------------------------------------------------------
# 3a. row walk: streaming kernels
# ---------------------------------------------------------------------------------------------------------------
def _emul_streaming(kernel, B, T, C, dtype, mutant=None, ops=None):
    """row-layout output image of the emulated kernel (storage dtype widened to fp32), reference and tolerance"""
    o = ops or E.real_operands(B * T, C, dtype)
    rl = lambda v: E.to_rl(v, B, T)
    if kernel == "bn_gelu_forward":
        full = E.emul_bn_gelu_forward(rl(o["x"]), o["scale"], o["shift"], dtype, mutant=mutant)
        ref, tol = E.ref_bn_gelu_forward(o["x"], o["scale"], o["shift"], dtype)
        W, U = C, 4
    elif kernel == "glu_forward":
        full = E.emul_glu_forward(rl(o["val"]), rl(o["gate"]))
        ref, tol = E.ref_glu_forward(o["val"], o["gate"], dtype)
        W, U = C, 2
    elif kernel == "gelu_backward":
        full = E.emul_gelu_backward(rl(o["x"]), rl(o["d"]), dtype, mutant=mutant)
        ref, tol = E.ref_gelu_backward(o["x"], o["d"], dtype)
        W, U = C, 1
    elif kernel == "glu_backward":
        full = E.emul_glu_backward(rl(o["val"]), rl(o["gate"]), rl(o["d"]), mutant=mutant)
        ref, tol = E.ref_glu_backward(o["val"], o["gate"], o["d"], dtype)
        W, U = C, 1
    else:
        out = E.q(o["val"].double().mul(E.sig64(o["gate"])).float(), dtype)
        full = E.emul_glu_backward_og(rl(out), rl(o["gate"]), rl(o["d"]), mutant=mutant, val=rl(o["val"]))
        ref, tol = E.ref_glu_backward_og(out, o["gate"], o["d"], dtype)
        W, U = C, 1
    mask = E.stream_mask(B, T, W, dtype, U, mutant)
    if full.shape[1] == 2 * W:
        mask = torch.cat([mask, mask], 1)
    img = torch.where(mask, E.q(full, dtype), torch.full_like(full, E.SENT))
    return img, ref, tol


STREAM_KERNELS = ("bn_gelu_forward", "glu_forward", "gelu_backward", "glu_backward", "glu_backward_og")


@pytest.mark.parametrize("dtype", E.DTYPES, ids=str)
@pytest.mark.parametrize("kernel", STREAM_KERNELS)
def test_streaming_emulation_passes_every_shape(kernel, dtype):
    for B, T, C in E.STREAM_SHAPES + (E.WIDE_SHAPE[dtype],):
        img, ref, tol = _emul_streaming(kernel, B, T, C, dtype)
        r, pads = check_rows(img, ref, tol, B, T)
        assert r <= 1.0 and pads, (kernel, dtype, (B, T, C), r, pads)


@pytest.mark.parametrize("mutant,kernel,shape", [
    ("pad_once_per_step", "bn_gelu_forward", (7, 5, 64)), ("pad_once_per_step", "gelu_backward", (7, 5, 64)),
    ("drop_last_row", "glu_forward", (3, 77, 320)), ("drop_last_row", "bn_gelu_forward", (1, 1, 64)),
    ("drop_batch_remainder", "bn_gelu_forward", (5, 33, 128)), ("drop_batch_remainder", "glu_forward", (5, 33, 128)),
    ("drop_second_pass", "bn_gelu_forward", "wide"), ("drop_second_pass", "glu_backward", "wide")])
def test_row_walk_mutants_of_the_streaming_kernels(mutant, kernel, shape):
    for dtype in E.DTYPES:
        B, T, C = E.WIDE_SHAPE[dtype] if shape == "wide" else shape
        img, ref, tol = _emul_streaming(kernel, B, T, C, dtype, mutant)
        r, _ = check_rows(img, ref, tol, B, T)
        caught(mutant, f"{kernel} {(B, T, C)} {dtype}", r)


# ---------------------------------------------------------------------------------------------------------------
# 3b. row walk: reducers
# ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", E.DTYPES, ids=str)
def test_colsum_emulation_is_exact_on_integers_and_within_the_bound_on_reals(dtype):
    for B, T, C in E.REDUCE_SHAPES:
        xi = E.integer_operands(B * T, C)["d"]
        assert torch.equal(E.emul_colsum(E.to_rl(xi, B, T), B, T, dtype), xi.double().sum(0).float()), (B, T, C)
        xr = E.real_operands(B * T, C, dtype)["x"]
        tol = E.sum_tol(xr, torch.zeros(()), E.reduce_n_acc(B, T, C, dtype))
        assert E.ratio(E.emul_colsum(E.to_rl(xr, B, T), B, T, dtype), xr.double().sum(0), tol) <= 1.0, (B, T, C)


@pytest.mark.parametrize("mutant,shape", [("pad_once_per_step", (7, 5, 128)), ("drop_last_row", (3, 77, 320)), ("drop_last_row", (1, 1, 64))])
def test_row_walk_mutants_of_the_reducers(mutant, shape):
    B, T, C = shape
    for dtype in E.DTYPES:
        xi = E.integer_operands(B * T, C)["d"] + 4.0                   # 1 .. 7: a dropped row always shows
        assert not torch.equal(E.emul_colsum(E.to_rl(xi, B, T), B, T, dtype, mutant), xi.double().sum(0).float())
        xr = E.real_operands(B * T, C, dtype)["x"] + 8.0
        tol = E.sum_tol(xr, torch.zeros(()), E.reduce_n_acc(B, T, C, dtype))
        caught(mutant, f"colsum {shape} {dtype}", E.ratio(E.emul_colsum(E.to_rl(xr, B, T), B, T, dtype, mutant), xr.double().sum(0), tol))


def test_integer_operands_make_the_fused_column_sums_exact():
    """GELU' = 1 / 0 at +-32 exactly in both device forms whatever the 1-ulp instructions return; sigmoid = 1 / 0 at +-100 given
    rcp(1) = 1 and rcp(inf) = 0"""
    o = E.integer_operands(64, 64)
    for dtype in E.DTYPES:
        for hw in E.HW_VARIANTS:
            gg = E.ggrad_emul(o["x"], dtype, hw)
            assert torch.equal(gg, (o["x"] > 0).float())
        assert torch.equal(E.sigmoid_emul(o["gate"]), (o["gate"] > 0).float())
        d = E.emul_glu_backward(o["val"], o["gate"], o["d"])
        assert torch.equal(d, d.round()) and torch.equal(d[:, 64:], torch.zeros(64, 64))


# ---------------------------------------------------------------------------------------------------------------
# 3c. value sweeps
# ---------------------------------------------------------------------------------------------------------------
def _sweep(kernel, x, dtype, hw=(0, 0), mutant=None):
    one = torch.ones_like(x)
    if kernel == "bn_gelu_forward":
        got = E.emul_bn_gelu_forward(x, torch.ones(64), torch.zeros(64), dtype, hw, mutant)
        ref, tol = E.ref_bn_gelu_forward(x, torch.ones(64), torch.zeros(64), dtype)
    elif kernel == "gelu_backward":
        got = E.emul_gelu_backward(x, one, dtype, hw, mutant)
        ref, tol = E.ref_gelu_backward(x, one, dtype)
    elif kernel == "glu_forward":
        got = E.emul_glu_forward(one, x, hw)
        ref, tol = E.ref_glu_forward(one, x, dtype)
    elif kernel == "glu_backward":
        got = E.emul_glu_backward(one, x, one, hw, mutant)
        ref, tol = E.ref_glu_backward(one, x, one, dtype)
    else:
        out = E.q(E.sig64(x).float(), dtype)
        got = E.emul_glu_backward_og(out, x, one, hw, mutant, val=one)
        ref, tol = E.ref_glu_backward_og(out, x, one, dtype)
    return E.q(got, dtype), ref, tol


@pytest.mark.parametrize("dtype", E.DTYPES, ids=str)
@pytest.mark.parametrize("kernel", STREAM_KERNELS)
def test_sweep_emulation_is_finite_and_within_tolerance_everywhere(kernel, dtype):
    for name, x in E.sweep_sets(dtype).items():
        for hw in E.HW_VARIANTS:
            got, ref, tol = _sweep(kernel, x, dtype, hw)
            assert E.ratio(got, ref, tol) <= 1.0, (kernel, dtype, name, hw, E.ratio(got, ref, tol))
        if kernel == "bn_gelu_forward":
            tiny = x.abs() < E.TINY[dtype]
            assert bool((got[tiny].abs() <= x[tiny].abs()).all())


@pytest.mark.parametrize("mutant,kernel", [("tanh_gelu", "bn_gelu_forward"), ("tail_without_e", "bn_gelu_forward"),
                                           ("tail_without_e", "gelu_backward"), ("ggrad_sign", "gelu_backward"),
                                           ("sig_grad_squared", "glu_backward"), ("og_uses_value", "glu_backward_og")])
def test_formula_mutants_miss_the_sweep_tolerance(mutant, kernel):
    for dtype in E.DTYPES:
        if mutant == "tail_without_e" and dtype == F32:
            continue                                                   # the fp32 form has no Abramowitz-Stegun tail
        worst = max(E.ratio(*_sweep(kernel, x, dtype, mutant=mutant)) for x in E.sweep_sets(dtype).values())
        caught(mutant, f"sweep {kernel} {dtype}", worst)


# ---------------------------------------------------------------------------------------------------------------
# 3d. partial sums and bn_finalize
# ---------------------------------------------------------------------------------------------------------------
def test_final_reduction_exactness_catches_fp32_and_a_short_stride():
    for Cp in (64, 320):
        for n in E.NTILES:
            part = E.exact_partials(n, Cp)
            want = part.double().sum(0).float()
            assert torch.equal(E.final_reduce(part.reshape(n, 2 * Cp)), want.reshape(-1))
            if n >= 127:
                assert not torch.equal(E.final_reduce(part.reshape(n, 2 * Cp), "fp32_final"), want.reshape(-1)), n
            if n > 128:
                assert not torch.equal(E.final_reduce(part.reshape(n, 2 * Cp), "first_128_rows"), want.reshape(-1)), n
    CAUGHT["fp32_final"] = ("exact partials, ntiles >= 127: not equal", math.inf)
    CAUGHT["first_128_rows"] = ("exact partials, ntiles 129 / 300 / 1024: not equal", math.inf)


def test_bn_finalize_channels_are_what_they_are_named():
    for n in E.NTILES:
        part = E.bn_partials(n, 60, 64)
        N = n * E.ROWS_PER_TILE
        r = E.ref_bn_finalize(part, N, E.bn_params(60), 60, 64, True)
        s = part.double().sum(0)
        raw = s[1] / N - (s[0] / N) ** 2
        assert raw[2] == 0.0 and raw[3] < 0.0 and raw[1] > 0.0
        assert abs(float(s[0, 1] / N)) > 500 * math.sqrt(float(raw[1]))
        assert float(r["rstd"][2]) == float(r["rstd"][3]) == 1.0 / math.sqrt(float(torch.tensor(1e-5, dtype=F32)))
        assert bool(torch.isfinite(r["rstd"]).all()) and bool((r["mean"][60:] == 0).all())


@pytest.mark.parametrize("mutant", ["no_clamp", "unbiased_norm"])
def test_bn_finalize_mutants_miss_one_ulp(mutant):
    worst, where = 0.0, None
    for n in E.NTILES:
        part, p = E.bn_partials(n, 60, 64), E.bn_params(60)
        N = n * E.ROWS_PER_TILE
        ref, bad = E.ref_bn_finalize(part, N, p, 60, 64, True), E.ref_bn_finalize(part, N, p, 60, 64, True, mutant=mutant)
        r = E.ratio(bad["rstd"].float(), ref["rstd"], E.ulp(ref["rstd"], F32))
        if r > worst:
            worst, where = r, n
        assert not E.within_one_ulp(bad["rstd"].float(), ref["rstd"])
    caught(mutant, f"bn_finalize rstd, ntiles {where}", worst)


# ---------------------------------------------------------------------------------------------------------------
# 3e. BatchNorm backward
# ---------------------------------------------------------------------------------------------------------------
def _bn_emul(dtype, dg_form, mutant=None, hw=(0, 0)):
    case = E.bn_backward_case(4, 40, 64, dtype, designed=True)
    r = E.ref_bn_backward(case, dtype, dg_form)
    got = E.emul_bn_backward_apply(case, r["mean"].float(), r["rstd"].float(), r["dgamma"].float(), r["dbeta"].float(), dtype, dg_form,
                                   dg=r["dg"], hw=hw, mutant=mutant)
    return E.ratio(E.q(got, dtype), r["dx"], r["tol"])


@pytest.mark.parametrize("dtype", E.DTYPES, ids=str)
@pytest.mark.parametrize("dg_form", [False, True])
def test_bn_backward_emulation_stays_inside_the_running_error_bound(dtype, dg_form):
    for hw in E.HW_VARIANTS:
        assert _bn_emul(dtype, dg_form, hw=hw) <= 1.0


@pytest.mark.parametrize("mutant", ["p_without_q_mean", "swap_dgamma_dbeta"])
def test_bn_backward_mutants_miss_the_bound(mutant):
    for dtype in E.DTYPES:
        for dg_form in (False, True):
            caught(mutant, f"bn backward (4, 40, 64) {dtype} dg={dg_form}", _bn_emul(dtype, dg_form, mutant))


# ---------------------------------------------------------------------------------------------------------------
# 3f. weight-gradient tail
# ---------------------------------------------------------------------------------------------------------------
def test_vec_reduce_unpack_emulation_and_its_mutants():
    for KS in E.WGRAD_KS:
        for Cout, Cin, half, half_p in ((48, 40, 0, 0), (70, 64, 0, 0), (40, 64, 20, 64)):
            slabs = E.wgrad_case(7, KS, Cout, Cin, half, half_p)
            ref = E.ref_reduce_unpack(slabs, Cout, Cin, KS, half, half_p)
            assert torch.equal(E.emul_reduce_unpack_vec(slabs, Cout, Cin, KS, half, half_p), ref)
            if KS == 3:
                assert not torch.equal(E.emul_reduce_unpack_vec(slabs, Cout, Cin, KS, half, half_p, "o1_for_oKS"), ref)
            if half:
                assert not torch.equal(E.ref_reduce_unpack(slabs, Cout, Cin, KS, half, half_p, "half_for_half_p"), ref)
    CAUGHT["o1_for_oKS"] = ("reduce_unpack KS = 3: not equal", math.inf)
    CAUGHT["half_for_half_p"] = ("reduce_unpack GLU pair half < half_p: not equal", math.inf)


# ---------------------------------------------------------------------------------------------------------------
# 3g. Adam
# ---------------------------------------------------------------------------------------------------------------
def _adam_ratio(n, mutant, steps=2, mag=1.0, step0=0):
    g = torch.Generator().manual_seed(29)
    p0 = torch.randn(n, generator=g)
    grads = [torch.randn(n, generator=g) * mag for _ in range(steps)]
    z = torch.zeros(n)
    tols = E.adam_tolerances(grads, p0, z, z, step0)
    pr = torch.nn.Parameter(p0.double())
    opt = torch.optim.Adam([pr], lr=1e-3)
    p, m, v, worst = p0.clone(), z.clone(), z.clone(), 0.0
    for k, gk in enumerate(grads, 1):
        p, m, v = E.emul_adam(p, gk, m, v, k, mutant=mutant)
        pr.grad = gk.double()
        opt.step()
        ref = (pr.detach(), opt.state[pr]["exp_avg"], opt.state[pr]["exp_avg_sq"])
        worst = max(worst, max(E.ratio(t, ref[i], tols[k - 1][i]) for i, t in enumerate((p, m, v))))
    return worst


def test_adam_emulation_passes_and_its_mutants_do_not():
    assert _adam_ratio(E.ADAM_BIG, None, steps=7) <= 1.0
    assert _adam_ratio(3, None, mag=1e-12) <= 1.0 and _adam_ratio(70, None, mag=1e12) <= 1.0
    caught("skip_second_trip", f"adam {E.ADAM_BIG} elements", _adam_ratio(E.ADAM_BIG, "skip_second_trip"))
    caught("skip_tail", f"adam {E.ADAM_BIG} elements (n % 4 = 1)", _adam_ratio(E.ADAM_BIG, "skip_tail"))
    caught("skip_tail", "adam 3 elements", _adam_ratio(3, "skip_tail"))
    caught("bias_step_minus_1", "adam step 1, 2", _adam_ratio(64, "bias_step_minus_1"))
    caught("eps_in_sqrt", "adam |g| = 1e-6", _adam_ratio(64, "eps_in_sqrt", mag=1e-6))


def _params(test):
    return [m.args[1] for m in test.pytestmark if m.name == "parametrize"][0]


def test_every_mutant_of_the_issue_is_recorded():
    """21 planted bugs, each caught at least once above (run on its own, this test runs the mutant tests first)"""
    want = {"pad_once_per_step", "drop_last_row", "drop_batch_remainder", "drop_second_pass", "tanh_gelu", "tail_without_e", "ggrad_sign",
            "sig_grad_squared", "og_uses_value", "fp32_final", "first_128_rows", "no_clamp", "unbiased_norm", "p_without_q_mean",
            "swap_dgamma_dbeta", "o1_for_oKS", "half_for_half_p", "skip_second_trip", "skip_tail", "bias_step_minus_1", "eps_in_sqrt"}
    if not want <= set(CAUGHT):
        for test in (test_row_walk_mutants_of_the_streaming_kernels, test_row_walk_mutants_of_the_reducers, test_formula_mutants_miss_the_sweep_tolerance,
                     test_bn_finalize_mutants_miss_one_ulp, test_bn_backward_mutants_miss_the_bound):
            for args in _params(test):
                test(*args) if isinstance(args, tuple) else test(args)
        test_final_reduction_exactness_catches_fp32_and_a_short_stride()
        test_vec_reduce_unpack_emulation_and_its_mutants()
        test_adam_emulation_passes_and_its_mutants_do_not()
    assert len(want) == 21 and want <= set(CAUGHT), want - set(CAUGHT)


# ---------------------------------------------------------------------------------------------------------------
# 4. host-side refusals
# ---------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def host():
    from speech_decoding_amd import lib
    Lb = lib.load()
    buf = (ctypes.c_char * (1 << 16))()                               # host memory that no kernel may ever see
    p = (ctypes.cast(buf, ctypes.c_void_p).value + 15) // 16 * 16
    return lib, Lb, p, buf


def _refused(Lb, rc, msg, what):
    assert rc == -1, what
    assert msg in Lb.sda_last_error(), (what, Lb.sda_last_error())


def test_reducers_refuse_widths_they_cannot_hold_without_launch(host):
    lib, Lb, p, _ = host
    for dt in (lib.F32, lib.BF16, lib.F16):
        for W in (1088, 96, 2048):
            _refused(Lb, Lb.sda_colsum(p, p, p, 2, 5, W, dt, None), b"colsum: bad arguments", W)
            _refused(Lb, Lb.sda_bn_gelu_backward_reduce(p, p, p, p, p, p, 64, p, p, p, 2, 5, W, dt, None),
                     b"bn_gelu_backward_reduce: bad arguments", W)
            _refused(Lb, Lb.sda_gelu_backward_colsum(p, p, p, p, p, 2, 5, W, dt, None), b"gelu_backward_colsum: bad arguments", W)
            _refused(Lb, Lb.sda_glu_backward_colsum(p, p, p, p, p, 2, 5, W, dt, None), b"glu_backward_colsum: bad arguments", W)
            _refused(Lb, Lb.sda_glu_backward_colsum_og(p, p, p, p, p, p, 2, 5, W, dt, None), b"glu_backward_colsum_og: bad arguments", W)
            _refused(Lb, Lb.sda_glu_backward_colsum_og(p, p, p, p, None, p, 2, 5, W, dt, None), b"glu_backward_colsum_og: bad arguments", W)


def test_streaming_kernels_refuse_a_width_that_is_no_multiple_of_64_without_launch(host):
    lib, Lb, p, _ = host
    for dt in (lib.F32, lib.BF16, lib.F16):
        for W in (96, 1000, 8):
            _refused(Lb, Lb.sda_bn_gelu_forward(p, p, p, p, 2, 5, W, dt, None), b"bn_gelu_forward: bad arguments", W)
            _refused(Lb, Lb.sda_bn_gelu_backward_apply(p, p, p, p, p, p, 8, p, p, 10.0, p, p, 2, 5, W, dt, None),
                     b"bn_gelu_backward_apply: bad arguments", W)
            _refused(Lb, Lb.sda_bn_gelu_backward_apply_dg(p, p, p, p, p, p, 8, p, p, 10.0, p, p, 2, 5, W, dt, None),
                     b"bn_gelu_backward_apply: bad arguments", W)
            _refused(Lb, Lb.sda_bn_gelu_backward_from_stats(p, 1, p, p, p, p, p, p, 8, 10.0, p, p, p, p, 2, 5, W, dt, None),
                     b"bn_gelu_backward_from_stats: bad arguments", W)
            _refused(Lb, Lb.sda_bn_gelu_backward_from_stats_dg(p, 1, p, p, p, p, p, p, 8, 10.0, p, p, p, p, 2, 5, W, dt, None),
                     b"bn_gelu_backward_from_stats: bad arguments", W)
            _refused(Lb, Lb.sda_glu_forward(p, p, 2, 5, W, dt, None), b"glu_forward: bad arguments", W)
            _refused(Lb, Lb.sda_glu_backward(p, p, p, 2, 5, W, dt, None), b"glu_backward: bad arguments", W)
            _refused(Lb, Lb.sda_gelu_backward(p, p, p, 2, 5, W, dt, None), b"gelu_backward: bad arguments", W)


def test_rows_sumsq_refuses_rows_that_are_no_whole_16_byte_loads(host):
    lib, Lb, p, _ = host
    for row_elems, pitch in ((6, 8), (255, 256), (8, 10)):
        _refused(Lb, Lb.sda_rows_sumsq(p, p, p, 2, row_elems, pitch, lib.F32, None), b"rows_sumsq: bad arguments", (row_elems, pitch))
    _refused(Lb, Lb.sda_rows_sumsq(p, p, p, 0, 8, 8, lib.F32, None), b"rows_sumsq: bad arguments", "B")
    _refused(Lb, Lb.sda_reduce_stats(p, 0, p, p, 64, None), b"reduce_stats: bad arguments", "nrows")
