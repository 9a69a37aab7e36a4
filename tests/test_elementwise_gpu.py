"""Kernel-level tests of csrc/elementwise.hip on a real MI355X: BatchNorm finalize / apply (+GELU), GLU, GELU backward, the
column sums and the per-sample norms; and of csrc/param_ops.hip: the vector maps, the slab reduce / unpack of the weight
gradients and the fused Adam; each launched directly in
fp32, bf16 and fp16 and held to float64 on the operands as the kernel reads them.  Inputs, references and tolerances (each with
its derivation) are in tests/elementwise_cases.py; tests/test_elementwise_cpu.py shows that these cases catch 21 planted bugs.

Edge -> test that launches it:
  RowCursor / RowWalk: one row, RG > T, batch remainders, idle threads, RG = 1, a second chunk pass   test_streaming_row_walk, test_bn_backward_row_walk
  stream_blocks' cap of 2048, red_blocks' cap of 1024                                               test_streaming_past_the_grid_cap, test_reducers (cap shape)
  every reducer width 64 .. 1024 (LDS image, bwd_colsum_pad)                                        test_reducers
  every finite 16-bit input of GELU, GELU', sigmoid; 1e-30 .. 1e30 in fp32                          test_value_sweep
  block_partial_sums' 128-row stride, bn_finalize's clamp / N = 1 / eval mode / padding channels    test_partial_sums_are_exact, test_bn_finalize
  a x + b cancellation of the BatchNorm backward                                                    test_bn_backward_away_from_mean_zero
  reduce_unpack_wgrad's 16-byte and element paths, GLU row map                                      test_reduce_unpack_wgrad, test_vector_maps
  rows_sumsq below / at / above one chunk per block, B > 64                                         test_rows_sumsq*
  Adam's second grid-stride trip, tail, element path, per-step-count launches, late bias correction test_adam*"""
import math

import pytest
import torch

from tests import elementwise_cases as E

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
DTYPES = E.DTYPES
F32 = torch.float32
WORST = {}                   # (kernel, dtype) -> max error / tolerance, printed when the module is done


@pytest.fixture(scope="module")
def ops():
    from speech_decoding_amd import ops as _ops
    from speech_decoding_amd import lib
    lib.load()
    assert torch.cuda.is_available(), "these tests need the MI355X"
    yield _ops
    print("\nworst error / tolerance per kernel and dtype:")
    for (kern, dt), r in sorted(WORST.items(), key=lambda kv: (kv[0][0], str(kv[0][1]))):
        print(f"  {kern:34s} {str(dt):16s} {r:.3f}")


def note(kern, dtype, what, r):
    """the figure is recorded and printed before anything is asserted on it"""
    WORST[(kern, dtype)] = max(WORST.get((kern, dtype), 0.0), r)
    print(f"{kern} {dtype} {what}: error / tolerance {r:.3f}")
    return r


def dev_ratio(got, ref, tol):
    got = got.double()
    if not bool(torch.isfinite(got).all()):
        return float("inf")
    return float(((got - ref.to(got.device)).abs() / tol.to(got.device)).max())


def up(valid, B, T, dtype, ridx=None):
    """(rows, W) fp32 valid-row values (rows of a pattern that ridx tiles over the batch) -> row-layout buffer on the device"""
    v = valid.to(dtype).to(DEV)
    if ridx is not None:
        v = v[ridx]
    buf = torch.zeros((E.L.rows_alloc(B, T), valid.shape[1]), dtype=dtype, device=DEV)
    buf[E.mem_rows(B, T).to(DEV)] = v
    return buf


def out_buf(B, T, W, dtype):
    return torch.full((E.L.rows_alloc(B, T), W), E.SENT, dtype=dtype, device=DEV)


def check_rows(kern, dtype, what, got_rl, ref, tol, B, T, ridx=None):
    """valid rows within tol of ref; every pad row and every row past the last sample still holds the sentinel bit for bit"""
    torch.cuda.synchronize()
    idx = E.mem_rows(B, T).to(DEV)
    ref, tol = ref.to(DEV), tol.to(DEV)
    if ridx is not None:
        ref, tol = ref[ridx], tol[ridx]
    r = note(kern, dtype, what, dev_ratio(got_rl[idx], ref, tol))
    other = torch.ones(got_rl.shape[0], dtype=torch.bool, device=DEV)
    other[idx] = False
    assert bool((got_rl[other] == E.SENT).all()), (kern, dtype, what, "wrote outside the valid rows")
    assert r <= 1.0, (kern, dtype, what, r)


def check_vec(kern, dtype, what, got, ref, tol):
    torch.cuda.synchronize()
    r = note(kern, dtype, what, dev_ratio(got, ref, tol))
    assert r <= 1.0, (kern, dtype, what, r)


# ---------------------------------------------------------------------------------------------------------------
# 1. row walk of the streaming kernels
# ---------------------------------------------------------------------------------------------------------------
def run_streaming(ops, kernel, B, T, C, dtype, o, ridx=None, what=""):
    u = lambda v: up(v, B, T, dtype, ridx)
    if kernel == "bn_gelu_forward":
        y = ops.bn_gelu_forward(u(o["x"]), out_buf(B, T, C, dtype), o["scale"].to(DEV), o["shift"].to(DEV), B, T)
        ref, tol = E.ref_bn_gelu_forward(o["x"], o["scale"], o["shift"], dtype)
    elif kernel == "glu_forward":
        y = ops.glu_forward(u(torch.cat([o["val"], o["gate"]], 1)), out_buf(B, T, C, dtype), B, T)
        ref, tol = E.ref_glu_forward(o["val"], o["gate"], dtype)
    elif kernel == "gelu_backward":
        y = ops.gelu_backward(u(o["x"]), u(o["d"]), out_buf(B, T, C, dtype), B, T)
        ref, tol = E.ref_gelu_backward(o["x"], o["d"], dtype)
    elif kernel == "glu_backward":
        y = ops.glu_backward(u(torch.cat([o["val"], o["gate"]], 1)), u(o["d"]), out_buf(B, T, 2 * C, dtype), B, T)
        ref, tol = E.ref_glu_backward(o["val"], o["gate"], o["d"], dtype)
    else:
        raise KeyError(kernel)
    check_rows(kernel, dtype, what or str((B, T, C)), y, ref, tol, B, T, ridx)
    return y


STREAMING = ("bn_gelu_forward", "glu_forward", "gelu_backward", "glu_backward")


@pytest.mark.parametrize("dtype", DTYPES, ids=str)
@pytest.mark.parametrize("kernel", STREAMING)
def test_streaming_row_walk(ops, kernel, dtype):
    for B, T, C in E.STREAM_SHAPES + (E.WIDE_SHAPE[dtype],):
        run_streaming(ops, kernel, B, T, C, dtype, E.real_operands(B * T, C, dtype))


@pytest.mark.parametrize("dtype", DTYPES, ids=str)
@pytest.mark.parametrize("kernel", STREAMING)
def test_streaming_past_the_grid_cap(ops, kernel, dtype):
    """more than 2048 x 8 x RG rows: every workgroup's range is longer than one batch of its row groups.  The batch tiles a
    251-row pattern, so the float64 reference is computed for 251 rows and gathered on the device."""
    B, T, C = E.stream_cap_shape(dtype)
    ridx = (torch.arange(B * T) % 251).to(DEV)
    run_streaming(ops, kernel, B, T, C, dtype, E.real_operands(251, C, dtype), ridx, what=f"cap {(B, T, C)}")


def bn_inputs(case, r, B, T, dtype, ridx=None):
    x, dy = up(case["x"], B, T, dtype, ridx), up(case["dy"], B, T, dtype, ridx)
    dg = up(r["dg"].float(), B, T, dtype, ridx)
    f = lambda v: v.float().to(DEV)
    return x, dy, dg, f(r["mean"]), f(r["rstd"]), f(case["gamma"]), f(case["beta"])


def tile_stats_of(r, C):
    """three statistics rows (sum dg, sum dg xhat) that add up to the batch sums (to fp32 rounding)"""
    tot = torch.stack([r["dbeta"], r["dgamma"]])
    return torch.stack([tot * 0.5, tot * 0.25, tot * 0.25]).float().to(DEV)


def run_bn_backward(ops, B, T, C, dtype, case, what, ridx=None, weight=None):
    """all three entry points of bn_gelu_backward against float64"""
    scratch = ops.reduce_scratch(C, DEV) if C <= 1024 else None
    n_acc = E.reduce_n_acc(B, T, C, dtype) if C <= 1024 else 4          # the stand-alone pass; three statistics rows otherwise
    for entry in ("sums", "tile_stats", "dy_is_dg"):
        if entry == "sums" and C > 1024:
            continue                                                     # the reducers stop at 1024 channels
        dg_form = entry == "dy_is_dg"
        r = E.ref_bn_backward(case, dtype, dg_form, weight, n_acc)
        x, dy, dg, mean, rstd, gamma, beta = bn_inputs(case, r, B, T, dtype, ridx)
        dx = out_buf(B, T, C, dtype)
        kw = {} if entry == "sums" else dict(tile_stats=tile_stats_of(r, C), dy_is_dg=dg_form)
        dgamma, dbeta = ops.bn_gelu_backward(dg if dg_form else dy, x, mean, rstd, gamma, beta, dx, B, T, scratch, **kw)
        check_rows(f"bn_gelu_backward[{entry}]", dtype, what, dx, r["dx"], r["tol"], B, T, ridx)
        check_vec(f"bn_gelu_backward[{entry}] dgamma", dtype, what, dgamma, r["dgamma"], r["tol_dgamma"])
        check_vec(f"bn_gelu_backward[{entry}] dbeta", dtype, what, dbeta, r["dbeta"], r["tol_dbeta"])


@pytest.mark.parametrize("dtype", DTYPES, ids=str)
def test_bn_backward_row_walk(ops, dtype):
    for B, T, C in E.STREAM_SHAPES + (E.WIDE_SHAPE[dtype],):
        run_bn_backward(ops, B, T, C, dtype, E.bn_backward_case(B, T, C, dtype, designed=False), str((B, T, C)))


@pytest.mark.parametrize("dtype", DTYPES, ids=str)
def test_bn_backward_past_the_grid_cap(ops, dtype):
    B, T, C = E.stream_cap_shape(dtype)
    rows = B * T
    ridx = torch.arange(rows) % 251
    weight = torch.bincount(ridx, minlength=251)
    case = E.bn_backward_case(1, 251, C, dtype, designed=False)
    run_bn_backward(ops, B, T, C, dtype, case, f"cap {(B, T, C)}", ridx.to(DEV), weight)


@pytest.mark.parametrize("dtype", DTYPES, ids=str)
def test_bn_backward_away_from_mean_zero(ops, dtype):
    """section 4: mean / std of 0, 1, 30, 300 per channel, gamma of both signs and one gamma = 0; float64 autograd"""
    B, T, C = 4, 40, 64
    case = E.bn_backward_case(B, T, C, dtype, designed=True)
    assert float(case["gamma"].min()) < 0 < float(case["gamma"].max()) and float(case["gamma"][5]) == 0.0
    run_bn_backward(ops, B, T, C, dtype, case, "designed (4, 40, 64)")


# ---------------------------------------------------------------------------------------------------------------
# 1. reducers
# ---------------------------------------------------------------------------------------------------------------
def run_reducers(ops, B, T, C, dtype, o, exact):
    """colsum, gelu_backward_colsum, glu_backward_colsum, glu_backward_colsum_og, glu_backward_og and the BatchNorm sums pass on one
    set of operands.  exact: integer operands — the sums owe torch.equal; else the running-error bound."""
    what = f"{'integer' if exact else 'real'} {(B, T, C)}"
    scratch = ops.reduce_scratch(C, DEV)
    u = lambda v: up(v, B, T, dtype)
    n_acc = E.reduce_n_acc(B, T, C, dtype)
    zero = torch.zeros(())

    def sums(kern, got, terms, term_tol):
        torch.cuda.synchronize()
        want = (terms.double().round() if exact else terms.double()).sum(0)     # exact: every term is an integer (or 1e-40 off one)
        if exact:
            assert torch.equal(got.cpu(), want.float()), (kern, dtype, what)
        else:
            check_vec(kern + " sums", dtype, what, got, want, E.sum_tol(terms, term_tol, n_acc))

    sums("colsum", ops.colsum(u(o["d"]), B, T, scratch), o["d"], zero)

    # GELU backward: the fused kernel's du is the plain kernel's, bit for bit
    du = ops.gelu_backward(u(o["x"]), u(o["d"]), out_buf(B, T, C, dtype), B, T)
    du2 = out_buf(B, T, C, dtype)
    cs = ops.gelu_backward_colsum(u(o["x"]), u(o["d"]), du2, B, T, scratch)
    ref, tol = E.ref_gelu_backward(o["x"], o["d"], dtype)
    check_rows("gelu_backward_colsum", dtype, what, du2, ref, tol, B, T)
    assert torch.equal(du, du2), ("gelu_backward_colsum", dtype, what)
    sums("gelu_backward_colsum", cs, ref, tol - E.ulp(ref, dtype))

    # GLU backward on [value | gate]
    xg = u(torch.cat([o["val"], o["gate"]], 1))
    dx = ops.glu_backward(xg, u(o["d"]), out_buf(B, T, 2 * C, dtype), B, T)
    dx2 = out_buf(B, T, 2 * C, dtype)
    cs = ops.glu_backward_colsum(xg, u(o["d"]), dx2, B, T, scratch)
    ref, tol = E.ref_glu_backward(o["val"], o["gate"], o["d"], dtype)
    check_rows("glu_backward_colsum", dtype, what, dx2, ref, tol, B, T)
    assert torch.equal(dx, dx2), ("glu_backward_colsum", dtype, what)
    sums("glu_backward_colsum", cs, *E.ref_glu_backward(o["val"], o["gate"], o["d"], dtype, unstored=True))

    # GLU backward after a fused forward: out = value * sigmoid(gate) as stored
    out = o["val"] * (o["gate"] > 0) if exact else E.q((o["val"].double() * E.sig64(o["gate"])).float(), dtype)
    dx = ops.glu_backward_og(u(out), u(o["gate"]), u(o["d"]), out_buf(B, T, 2 * C, dtype), B, T)
    dx2 = out_buf(B, T, 2 * C, dtype)
    cs = ops.glu_backward_colsum_og(u(out), u(o["gate"]), u(o["d"]), dx2, B, T, scratch)
    ref, tol = E.ref_glu_backward_og(out, o["gate"], o["d"], dtype)
    check_rows("glu_backward_colsum_og", dtype, what, dx2, ref, tol, B, T)
    check_rows("glu_backward_og", dtype, what, dx, ref, tol, B, T)
    assert torch.equal(dx, dx2), ("glu_backward_og", dtype, what)
    sums("glu_backward_colsum_og", cs, *E.ref_glu_backward_og(out, o["gate"], o["d"], dtype, unstored=True))

    if exact:
        # BatchNorm sums pass with mean 0, rstd 1, gamma 1, beta 0 on x = +-32: dg = dy or 0, dg xhat = 32 dy or 0
        one, nul = torch.ones(C, device=DEV), torch.zeros(C, device=DEV)
        dgamma, dbeta = ops.bn_gelu_backward(u(o["d"]), u(o["x"]), nul, one, one, nul, out_buf(B, T, C, dtype), B, T, scratch)
        torch.cuda.synchronize()
        dgv = o["d"].double() * (o["x"] > 0)
        assert torch.equal(dbeta.cpu(), dgv.sum(0).float()) and torch.equal(dgamma.cpu(), (dgv * 32.0).sum(0).float()), ("bn sums", dtype, what)


@pytest.mark.parametrize("dtype", DTYPES, ids=str)
@pytest.mark.parametrize("exact", [True, False], ids=["integer", "real"])
def test_reducers(ops, dtype, exact):
    """the row-walk shapes, every width 64 .. 1024 at (3, 11, width), and one shape past red_blocks' cap of 1024"""
    for B, T, C in E.REDUCE_SHAPES + (E.REDUCE_CAP_SHAPE,):
        o = E.integer_operands(B * T, C) if exact else E.real_operands(B * T, C, dtype)
        run_reducers(ops, B, T, C, dtype, o, exact)


# ---------------------------------------------------------------------------------------------------------------
# 2. exhaustive value sweeps
# ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES, ids=str)
def test_value_sweep(ops, dtype):
    """every finite bf16 / fp16 bit pattern (fp32 storage: both sets widened, and 65 536 log-uniform values of either sign
    between 1e-30 and 1e30) as the GELU, GELU' and gate input: finite outputs, within tolerance of float64, and a zero or
    subnormal input gives a GELU no larger than itself"""
    B, T, C = 1, 1024, 64
    for name, x in E.sweep_sets(dtype).items():
        assert torch.equal(E.q(x, dtype), x)
        one = torch.ones_like(x)
        u = lambda v: up(v, B, T, dtype)
        what = f"sweep {name}"
        y = ops.bn_gelu_forward(u(x), out_buf(B, T, C, dtype), torch.ones(C, device=DEV), torch.zeros(C, device=DEV), B, T)
        check_rows("bn_gelu_forward", dtype, what, y, *E.ref_bn_gelu_forward(x, torch.ones(C), torch.zeros(C), dtype), B, T)
        got = y[E.mem_rows(B, T).to(DEV)].float().cpu()
        tiny = x.abs() < E.TINY[dtype]
        assert name == "loguniform" or int(tiny.sum()) > 2                     # +-0 and the storage type's subnormals
        assert bool((got[tiny].abs() <= x[tiny].abs()).all()), (dtype, name, "zero-sized inputs")
        y = ops.gelu_backward(u(x), u(one), out_buf(B, T, C, dtype), B, T)
        check_rows("gelu_backward", dtype, what, y, *E.ref_gelu_backward(x, one, dtype), B, T)
        xg = u(torch.cat([one, x], 1))
        y = ops.glu_forward(xg, out_buf(B, T, C, dtype), B, T)
        check_rows("glu_forward", dtype, what, y, *E.ref_glu_forward(one, x, dtype), B, T)
        y = ops.glu_backward(xg, u(one), out_buf(B, T, 2 * C, dtype), B, T)
        check_rows("glu_backward", dtype, what, y, *E.ref_glu_backward(one, x, one, dtype), B, T)
        out = E.q(E.sig64(x).float(), dtype)
        y = ops.glu_backward_og(u(out), u(x), u(one), out_buf(B, T, 2 * C, dtype), B, T)
        check_rows("glu_backward_og", dtype, what, y, *E.ref_glu_backward_og(out, x, one, dtype), B, T)


# ---------------------------------------------------------------------------------------------------------------
# 3. block_partial_sums and bn_finalize on given partials
# ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("Cp", [64, 320])
def test_partial_sums_are_exact(ops, Cp):
    """multiples of 2^-20 below 2^10: the fp64 sum over up to 1024 rows is exact, so reduce_stats and the sums inside
    bn_gelu_backward(tile_stats=...) owe torch.equal to it"""
    B, T = 1, 2
    x, dx = torch.zeros((E.L.rows_alloc(B, T), Cp), device=DEV), out_buf(B, T, Cp, F32)
    vec = torch.ones(Cp - 3, device=DEV)                                       # C < Cp
    mean = torch.zeros(Cp, device=DEV)
    for n in E.NTILES:
        part = E.exact_partials(n, Cp)
        want = part.double().sum(0).float()
        got = ops.reduce_stats(part.to(DEV))
        dgamma, dbeta = ops.bn_gelu_backward(x, x, mean, mean, vec, vec, dx, B, T, None, tile_stats=part.to(DEV))
        torch.cuda.synchronize()
        assert torch.equal(got.cpu(), want.reshape(-1)), ("reduce_stats", n, Cp)
        assert torch.equal(dbeta.cpu(), want[0]) and torch.equal(dgamma.cpu(), want[1]), ("bn_gelu_backward(tile_stats)", n, Cp)


@pytest.mark.parametrize("Cp,C", [(64, 60), (320, 270)])
def test_bn_finalize(ops, Cp, C):
    """mean, rstd, scale, shift, the running statistics, the coefficient table and the batch counter against float64 formulas on
    the same fp32 partials, within one fp32 ulp (the kernel works in double and rounds once)"""
    p = E.bn_params(C)
    d = lambda v: v.clone().to(DEV)
    for n in E.NTILES:
        part = E.bn_partials(n, C, Cp)
        N = n * E.ROWS_PER_TILE
        rm, rv, cnt = d(p["running_mean"]), d(p["running_var"]), torch.tensor(41, dtype=torch.int64, device=DEV)
        mean, rstd, scale, shift, coef = ops.bn_finalize(part.to(DEV), n, N, d(p["gamma"]), d(p["beta"]), rm, rv, Cp, True,
                                                         want_bwd_coef=True, batches_tracked=cnt)
        torch.cuda.synchronize()
        ref = E.ref_bn_finalize(part, N, p, C, Cp, True)
        for name, got in (("mean", mean), ("rstd", rstd), ("scale", scale), ("shift", shift), ("running_mean", rm), ("running_var", rv),
                          ("coef", coef)):
            assert E.within_one_ulp(got, ref[name]), (name, n, Cp, got.cpu(), ref[name])
        assert bool((torch.stack([mean, rstd, scale, shift])[:, C:] == 0).all()) and bool((coef[:, C:] == 0).all())
        assert int(cnt) == 42
        assert float(rstd[2]) == float(rstd[3]) == float(torch.tensor(1.0 / math.sqrt(float(torch.tensor(1e-5, dtype=F32))), dtype=F32))
    # N = 1: the unbiased variance is the variance itself
    xs = torch.randint(-20, 21, (Cp,), generator=torch.Generator().manual_seed(53)).float() / 4.0      # x^2 is exact: var = 0
    one = torch.stack([xs, xs * xs]).unsqueeze(0)
    rm, rv = d(p["running_mean"]), d(p["running_var"])
    outs = ops.bn_finalize(one.to(DEV), 1, 1, d(p["gamma"]), d(p["beta"]), rm, rv, Cp, True)
    torch.cuda.synchronize()
    ref = E.ref_bn_finalize(one, 1, p, C, Cp, True)
    for name, got in zip(("mean", "rstd", "scale", "shift", "running_mean", "running_var"), tuple(outs) + (rm, rv)):
        assert E.within_one_ulp(got, ref[name]), ("N = 1", name)
    # eval mode: from the running statistics, which stay as they are, and the counter does not move
    rm, rv, cnt = d(p["running_mean"]), d(p["running_var"]), torch.tensor(41, dtype=torch.int64, device=DEV)
    outs = ops.bn_finalize(None, 0, 1, d(p["gamma"]), d(p["beta"]), rm, rv, Cp, False, want_bwd_coef=True, batches_tracked=cnt)
    torch.cuda.synchronize()
    ref = E.ref_bn_finalize(None, 1, p, C, Cp, False)
    for name, got in zip(("mean", "rstd", "scale", "shift", "coef"), outs):
        assert E.within_one_ulp(got, ref[name]), ("eval", name)
    assert torch.equal(rm.cpu(), p["running_mean"]) and torch.equal(rv.cpu(), p["running_var"]) and int(cnt) == 41


# ---------------------------------------------------------------------------------------------------------------
# 5. weight-gradient reduce / unpack, vector maps
# ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("Cout,Cin,half,half_p", E.WGRAD_SHAPES)
def test_reduce_unpack_wgrad(ops, Cout, Cin, half, half_p):
    """integer slabs: both kernels, and reduce_slabs + unpack_conv_wgrad, owe torch.equal to the index-loop reference; slabs
    viewed 4 bytes into their allocation take the element path and give the same bits"""
    for KS in E.WGRAD_KS:
        for nslabs in E.WGRAD_NSLABS:
            slabs = E.wgrad_case(nslabs, KS, Cout, Cin, half, half_p)
            ref = E.ref_reduce_unpack(slabs, Cout, Cin, KS, half, half_p)
            dev = slabs.to(DEV)
            assert dev.data_ptr() % 16 == 0
            got = ops.reduce_unpack_wgrad(dev, Cout, Cin, KS, half, half_p)
            shifted = torch.empty(slabs.numel() + 1, device=DEV)[1:].view(slabs.shape)
            shifted.copy_(dev)
            assert shifted.data_ptr() % 16 == 4
            got_elem = ops.reduce_unpack_wgrad(shifted, Cout, Cin, KS, half, half_p)
            two = ops.unpack_conv_wgrad(ops.reduce_slabs(dev), 1, Cout, Cin, KS, slabs.shape[2], slabs.shape[3], half, half_p)[0]
            torch.cuda.synchronize()
            assert torch.equal(got.cpu(), ref), ("reduce_unpack_wgrad", nslabs, KS)
            assert torch.equal(got_elem.cpu(), ref), ("reduce_unpack_wgrad, element path", nslabs, KS)
            assert torch.equal(two.cpu(), ref), ("reduce_slabs + unpack_conv_wgrad", nslabs, KS)


def test_vector_maps(ops):
    """pack_vector / unpack_vector round trip with and without GLU halves; pad slots are zero"""
    g = torch.Generator().manual_seed(31)
    for Cc, Cp, half, half_p in ((40, 64, 0, 0), (270, 320, 0, 0), (64, 64, 0, 0), (600, 640, 300, 320), (70, 128, 35, 64)):
        v = torch.randn(Cc, generator=g)
        packed = ops.pack_vector(v.to(DEV), Cp, half, half_p)
        back = ops.unpack_vector(packed, Cc, half, half_p)
        torch.cuda.synchronize()
        want = torch.zeros(Cp)
        for c in range(Cc):
            want[E.glu_map(c, half, half_p)] = v[c]
        assert torch.equal(packed.cpu(), want) and torch.equal(back.cpu(), v), (Cc, Cp, half, half_p)


# ---------------------------------------------------------------------------------------------------------------
# 6. per-sample norms
# ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES, ids=str)
@pytest.mark.parametrize("B", E.SUMSQ_B)
def test_rows_sumsq(ops, dtype, B):
    g = torch.Generator().manual_seed(37)
    for row_elems in E.SUMSQ_ROW_ELEMS:
        pitch = row_elems + 8
        for exact in (True, False):
            x = torch.full((B, pitch), 100.0)                                  # the gap between rows must not be read
            x[:, :row_elems] = (torch.randint(-3, 4, (B, row_elems), generator=g).float() if exact
                                else E.q(torch.randn(B, row_elems, generator=g) * 2.0, dtype))
            got = ops.rows_sumsq(x.to(dtype).to(DEV), B, row_elems, pitch)
            torch.cuda.synchronize()
            sq = x[:, :row_elems].double() ** 2
            if exact:
                assert torch.equal(got.cpu(), sq.sum(1).float()), (dtype, B, row_elems)
            else:
                check_vec("rows_sumsq", dtype, f"B {B} row_elems {row_elems}", got, sq.sum(1),
                          E.sum_tol(sq, torch.zeros(()), E.sumsq_n_acc(row_elems), dim=1))


@pytest.mark.parametrize("B", E.SUMSQ_B)
def test_rows_sumsq_from_stats_and_row_parts(ops, B):
    """both sum in fp64 in a fixed order: integers owe torch.equal, reals one fp32 ulp"""
    g = torch.Generator().manual_seed(41)
    for exact in (True, False):
        gen = (lambda *s: torch.randint(0, 50, s, generator=g).float()) if exact else (lambda *s: torch.rand(*s, generator=g) * 9.0)
        for tiles, Cp in ((1, 64), (3, 320), (5, 1024)):
            stats = gen(B * tiles, 2, Cp)
            got = ops.rows_sumsq_from_stats(stats.to(DEV), B)
            torch.cuda.synchronize()
            want = stats[:, 1].double().reshape(B, -1).sum(1)
            assert torch.equal(got.cpu(), want.float()) if exact else E.within_one_ulp(got, want), ("from_stats", B, tiles, Cp, exact)
        for T, n_parts in ((1, 1), (77, 5), (300, 2)):
            parts = torch.full((E.L.rows_alloc(B, T), n_parts), 1000.0)        # pad rows hold junk the kernel must skip
            valid = gen(B * T, n_parts)
            parts[E.mem_rows(B, T)] = valid
            got = ops.rows_sumsq_from_row_parts(parts.to(DEV), B, T)
            torch.cuda.synchronize()
            want = valid.double().reshape(B, -1).sum(1)
            assert torch.equal(got.cpu(), want.float()) if exact else E.within_one_ulp(got, want), ("from_row_parts", B, T, n_parts, exact)


# ---------------------------------------------------------------------------------------------------------------
# 7. Adam
# ---------------------------------------------------------------------------------------------------------------
def _real(t):
    return torch.view_as_real(t) if t.is_complex() else t


def test_adam_against_float64_adam():
    """FusedAdam against torch.optim.Adam on float64 copies after 1, 2 and 7 steps: parameters, exp_avg and exp_avg_sq.  big: a
    second grid-stride trip and a tail that is no multiple of 4; offset: data_ptr() % 16 == 4, the element path; late: first
    gradient at step 3 (its own step count, a second launch in one step()); never: no gradient, stays bit-identical; zero: an
    all-zero gradient moves nothing."""
    from speech_decoding_amd.optim import FusedAdam
    names = ("big", "three", "cplx", "offset", "late", "never", "zero")
    grads, shapes = E.adam_grads(names, max(E.ADAM_STEPS))
    g = torch.Generator().manual_seed(43)
    init = {n: torch.randn(shapes[n], generator=g) for n in names}
    base = torch.zeros(1002, device=DEV)
    assert base.data_ptr() % 16 == 0
    base[1:] = init["offset"].to(DEV)

    def make(n, dev, dt):
        t = init[n].to(dt)
        t = torch.view_as_complex(t.contiguous()) if n == "cplx" else t
        if dev == DEV and n == "offset":
            return torch.nn.Parameter(base[1:])
        return torch.nn.Parameter(t.to(dev))
    P = {n: make(n, DEV, torch.float32) for n in names}
    R = {n: make(n, "cpu", torch.float64) for n in names}
    assert P["offset"].data_ptr() % 16 == 4 and P["big"].numel() > 256 * 1024 and P["big"].numel() % 4 == 1
    opt, ref = FusedAdam(P.values(), lr=1e-3), torch.optim.Adam(R.values(), lr=1e-3)
    tols = {n: E.adam_tolerances(grads[n], init[n], torch.zeros(shapes[n]), torch.zeros(shapes[n]), 0) for n in names}
    for k in range(1, max(E.ADAM_STEPS) + 1):
        for n in names:
            gk = grads[n][k - 1]
            P[n].grad = None if gk is None else (torch.view_as_complex(gk.contiguous()) if n == "cplx" else gk).to(DEV)
            R[n].grad = None if gk is None else (torch.view_as_complex(gk.double().contiguous()) if n == "cplx" else gk.double())
        opt.step()
        ref.step()
        torch.cuda.synchronize()
        if k not in E.ADAM_STEPS:
            continue
        for n in names:
            if tols[n][k - 1] is None:
                assert torch.equal(_real(P[n].detach()).cpu(), init[n]), (n, k, "a parameter without a gradient moved")
                continue
            tp, tm, tv = tols[n][k - 1]
            for what, got, want, tol in (("param", P[n].detach(), R[n].detach(), tp), ("exp_avg", opt.state[P[n]]["exp_avg"], ref.state[R[n]]["exp_avg"], tm),
                                         ("exp_avg_sq", opt.state[P[n]]["exp_avg_sq"], ref.state[R[n]]["exp_avg_sq"], tv)):
                r = note(f"adam {n} {what}", F32, f"step {k}", dev_ratio(_real(got), _real(want), tol))
                assert r <= 1.0, (n, what, k, r)
        assert torch.equal(P["zero"].detach().cpu(), init["zero"]), "an all-zero gradient moved its parameter"
        assert int(opt.state[P["late"]].get("step", 0)) == max(0, k - 2) and int(opt.state[P["big"]]["step"]) == k
    assert P["never"] not in opt.state or not opt.state[P["never"]]


def test_adam_late_bias_correction():
    """state["step"] preset to 9 999 with exp_avg / exp_avg_sq in place: one more step against float64 Adam"""
    from speech_decoding_amd.optim import FusedAdam
    g = torch.Generator().manual_seed(47)
    n = 4099
    p0, m0, v0, grad = torch.randn(n, generator=g), torch.randn(n, generator=g) * 0.1, torch.rand(n, generator=g) * 0.01, torch.randn(n, generator=g)
    p, r = torch.nn.Parameter(p0.to(DEV)), torch.nn.Parameter(p0.double())
    opt, ref = FusedAdam([p], lr=1e-3), torch.optim.Adam([r], lr=1e-3)
    opt.state[p].update(step=9999, exp_avg=m0.to(DEV), exp_avg_sq=v0.to(DEV))
    ref.state[r].update(step=torch.tensor(9999.0), exp_avg=m0.double(), exp_avg_sq=v0.double())
    p.grad, r.grad = grad.to(DEV), grad.double()
    opt.step()
    ref.step()
    torch.cuda.synchronize()
    assert int(opt.state[p]["step"]) == 10000 and float(ref.state[r]["step"]) == 10000.0
    tp, tm, tv = E.adam_tolerances([grad], p0, m0, v0, 9999)[0]
    for what, got, want, tol in (("param", p.detach(), r.detach(), tp), ("exp_avg", opt.state[p]["exp_avg"], ref.state[r]["exp_avg"], tm),
                                 ("exp_avg_sq", opt.state[p]["exp_avg_sq"], ref.state[r]["exp_avg_sq"], tv)):
        rr = note(f"adam step 10000 {what}", F32, "", dev_ratio(got, want, tol))
        assert rr <= 1.0, (what, rr)
