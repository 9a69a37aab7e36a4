"""Exact-arithmetic tests of the matrix-core kernels on a real MI355X: small-integer operands (tests/exact_cases.py), int64-exact
references, and torch.equal on the unpacked stored values — no tolerance.  Every product and every fp32 partial sum is an
integer below 2^24, so the accumulator is the same in every summation order, tiling and split-K plan; the stored value is
its round-to-nearest-even rounding.  tests/test_exact_cpu.py proves on the CPU that the cases imported here exercise the
rounding (ties included) and that a truncating store, a 16-bit accumulator, a double rounding or a defect on one tile edge
each fail them."""
import numpy as np
import pytest
import torch
import torch.nn.functional as TF

pytestmark = pytest.mark.gpu

from tests import exact_cases as X   # noqa: E402

DEV = "cuda:0"
NAN = float("nan")


@pytest.fixture(scope="module")
def ops():
    from speech_decoding_amd import ops as _ops
    from speech_decoding_amd import lib
    lib.load()
    assert torch.cuda.is_available(), "these tests need the MI355X"
    return _ops


def name(dtype):
    return str(dtype).replace("torch.", "")


def rows(ops, t, dtype, Cp=None):
    """float64 integers (B, C, T) -> row-layout buffer of `dtype` (lossless cast asserted)"""
    from speech_decoding_amd import lib as L
    B, C, T = t.shape
    buf = ops.new_rows(B, T, Cp or L.pad_channels(C), dtype, DEV)
    return ops.pack_rows(X.operand(t, dtype).to(DEV), buf)


def unrows(ops, buf, B, C, T):
    return ops.unpack_rows(buf, B, C, T).cpu().double()


def weight(ops, w, Cout_p, Cin_p, dtype, **kw):
    X.operand(w, dtype)
    return ops.pack_conv_weight(w.float().to(DEV), Cout_p, Cin_p, dtype, **kw)


def padding_is_zero(buf, B, C, T):
    """pad rows (in front of every sample, behind the last) and pad channels of a row-layout buffer hold exact zeros"""
    from speech_decoding_amd import lib as L
    full = buf.float().cpu()
    Tp = L.rows_tp(T)
    valid = torch.zeros(full.shape[0], dtype=torch.bool)
    for b in range(B):
        valid[b * Tp + L.ROW_PAD: b * Tp + L.ROW_PAD + T] = True
    ok = bool((full[~valid] == 0).all())
    return ok and (full.shape[1] == C or bool((full[:, C:] == 0).all()))


# ---------------------------------------------------------------------------------------------------------------
# kernel size 3, forward
# ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", X.DTYPES, ids=name)
@pytest.mark.parametrize("regime", X.REGIMES)
@pytest.mark.parametrize("i", range(len(X.CONV3_SHAPES)), ids=lambda i: "x".join(map(str, X.CONV3_SHAPES[i])))
def test_conv3_forward_every_tiling_and_epilogue(ops, i, regime, dtype):
    """one tile / two tiles per workgroup, the flat kernel (two workgroups or one per CU; widths without a flat tiling take the
    tile kernel again), each bare, with bias, with bias + residual: the stored values are the rounded exact ones, padding stays
    zero, and in the exact regime the statistics' sum plane holds the exact column sums.
    With no CU limit these shapes (at most 3 units x 2 channel tiles against 512 workgroup slots) give the flat kernel a plan of
    one unit per workgroup: it runs its 128-row tiles only.  Its 256-row tile, and runs of several tiles per workgroup, meet the
    same references in tests/test_persistent_runs_gpu.py."""
    from speech_decoding_amd import lib as L
    case = X.conv3_case(i, regime, dtype)
    s = case.shape
    B = s.B
    Cin_p, Cout_p = L.pad_channels(s.cin), L.pad_channels(s.cout)
    xb = rows(ops, case.x, dtype)
    wp = weight(ops, case.w, Cout_p, Cin_p, dtype)
    bias = ops.pack_vector(case.bias.float().to(DEV), Cout_p)
    for tiling in (L.CONV_SINGLE_TILE, L.CONV_PAIR_TILES, L.CONV_FLAT_TILES, L.CONV_FLAT_TILES | L.CONV_ONE_PER_CU):
        for epi in X.EPILOGUES:
            if epi == "bias_res" and case.res is None:
                continue
            what = f"conv3 {tuple(s)} {regime} {name(dtype)} flags {tiling} {epi}"
            want = X.store(X.conv_expected(case, epi), dtype)
            yb = ops.new_rows(B, s.T, Cout_p, dtype, DEV)
            stats = None if epi == "bare" else torch.full((ops.conv_stats_rows(B, s.T, 3, Cout_p, tiling), 2, Cout_p), NAN, device=DEV)
            ops.conv_gemm(xb, wp, yb, B=B, T=s.T, KS=3, dil=s.dil, bias=None if epi == "bare" else bias,
                          res=xb if epi == "bias_res" else None, stats=stats, flags=tiling)
            X.assert_same(unrows(ops, yb, B, s.cout, s.T), want, what)
            assert padding_is_zero(yb, B, s.cout, s.T), what
            if stats is not None and regime == "exact":
                assert float(want.abs().sum(dim=(0, 2)).max()) < 2 ** 24
                X.assert_same(stats[:, 0, :s.cout].double().sum(0).cpu(), want.sum(dim=(0, 2)), what + " stats sums", axes="c")


@pytest.mark.parametrize("dtype", X.DTYPES, ids=name)
@pytest.mark.parametrize("regime", X.REGIMES)
def test_conv3_flat_glu_epilogue_keeps_the_exact_gate(ops, regime, dtype):
    check_glu_gate(ops, regime, dtype)


def check_glu_gate(ops, regime, dtype):
    """SDA_EPI_GLU (weights and bias packed 80 values + 80 gates per tile): the gate written to y_pre is the conv's gate half"""
    from speech_decoding_amd import lib as L
    case = X.glu_case(regime, dtype)
    s, half = case.shape, X.GLU_HALF
    Cin_p, Hp = L.pad_channels(s.cin), L.pad_channels(half)
    assert Hp % 80 == 0
    X.operand(case.w, dtype)
    w_d, b_d = case.w.float().to(DEV), case.bias.float().to(DEV)
    plan = ops.PackPlan(dtype, DEV)
    plan.add_weight("w", w_d, 2 * Hp, Cin_p, glu_half=half, glu_half_p=Hp, glu_tile=80)
    plan.add_vector("b", b_d, 2 * Hp, glu_half=half, glu_half_p=Hp, glu_tile=80)
    pk = plan.run({"w": w_d, "b": b_d})
    xb = rows(ops, case.x, dtype)
    out, gate = ops.new_rows(s.B, s.T, Hp, dtype, DEV), ops.new_rows(s.B, s.T, Hp, dtype, DEV)
    ops.conv_gemm(xb, pk["w"], out, B=s.B, T=s.T, KS=3, dil=s.dil, bias=pk["b"], y_pre=gate, flags=L.CONV_FLAT_TILES | L.EPI_GLU)
    X.assert_same(unrows(ops, gate, s.B, half, s.T), X.store(case.ref[:, half:], dtype), f"glu gate {regime} {name(dtype)}")
    assert padding_is_zero(gate, s.B, half, s.T)


@pytest.mark.parametrize("B,T,dtype", [(136, 345, torch.bfloat16), (136, 345, torch.float16), (227, 345, torch.bfloat16),
                                       (227, 345, torch.float16), (136, 345, torch.float32)],
                         ids=lambda v: name(v) if isinstance(v, torch.dtype) else str(v))
def test_conv3_flat_staggered_tile_order_gives_the_same_bits(ops, B, T, dtype):
    """SDA_CONV_FLAT_STAGGER (the forward path's order: the second workgroup of a CU takes its 128-row tile(s) first) against
    SDA_CONV_FLAT_TILES alone on the same operands, 320 -> 320 channels (two channel tiles), dilation 2, bias + residual +
    statistics: the stored buffers are equal bit for bit.  On 256 CUs (136, 345) is 384 units, 2 per workgroup — every second
    workgroup of a CU turns one 256-row tile into 128 + 128 — and (227, 345) is 641 units, 3 per workgroup — 128 + 256 instead of
    256 + 128; fp32 storage runs 128-row tiles in either order.
    The statistics: a 256-row tile writes its sums into its first unit's row and zeros into the second, so the two orders
    spread the same sums over a run's rows differently by design (and the same for fp32, where the rows themselves must be
    equal).  What both orders share is the sum over a workgroup's run of units, and the operands are integers small enough that
    every partial sum (and sum of squares) of a tile is exact in fp32, whatever the order: the per-run sums, taken in float64,
    are compared with torch.equal, and so are the raw rows for fp32.
    Both orders could be wrong alike, so the plain order's output must also equal a reference that uses no project kernel: the
    operands are integers in [-1, 1] (bias in [-3, 3]), so three shifted float64 matmuls plus bias and residual are exact, and
    the stored value is their one rounding to the storage type."""
    from speech_decoding_amd import lib as L
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    if cus != 256:
        pytest.skip(f"the shapes are taken from conv3_flat's tile plan for 256 CUs; this device has {cus}")
    C, dil = 320, 2
    n_units = ops.conv_stats_rows(B, T, 3, C, L.CONV_FLAT_TILES)
    per_wg = -(-n_units * (C // 160) // (2 * cus))
    assert (n_units, per_wg) == {136: (384, 2), 227: (641, 3)}[B]
    g = torch.Generator(device=DEV)
    g.manual_seed(B)
    x = torch.randint(-1, 2, (B, C, T), device=DEV, generator=g).to(dtype)
    w = torch.randint(-1, 2, (C, C, 3), device=DEV, generator=g).float()
    xb = ops.pack_rows(x, ops.new_rows(B, T, C, dtype, DEV))
    wp = ops.pack_conv_weight(w, C, C, dtype)
    bias_v = torch.randint(-3, 4, (C,), device=DEV, generator=g)
    bias = ops.pack_vector(bias_v.float(), C)
    got = []
    for flags in (L.CONV_FLAT_TILES, L.CONV_FLAT_TILES | L.CONV_FLAT_STAGGER):
        yb = ops.new_rows(B, T, C, dtype, DEV)
        stats = torch.full((n_units, 2, C), NAN, device=DEV)
        ops.conv_gemm(xb, wp, yb, B=B, T=T, KS=3, dil=dil, bias=bias, res=xb, stats=stats, flags=flags)
        got.append((yb, stats))
    (y0, s0), (y1, s1) = got
    # the reference, in plain torch on the device: three shifted float64 matmuls (integers: exact), bias and residual, one rounding
    xd = TF.pad(x.double(), (dil, dil))
    want = sum(torch.matmul(w[:, :, k].double(), xd[:, :, k * dil: k * dil + T]) for k in range(3))
    want = (want + bias_v.double()[None, :, None] + x.double()).float().to(dtype)
    if not torch.equal(ops.unpack_rows(y0, B, C, T), want.float()):         # (the failing index names the tile or run boundary)
        X.assert_same(ops.unpack_rows(y0, B, C, T), want, f"conv3_flat {B} x {C} x {T} {name(dtype)} against three shifted matmuls")
    assert torch.equal(ops.unpack_rows(y0, B, C, T), ops.unpack_rows(y1, B, C, T))
    assert torch.equal(y0, y1)                                           # padding included
    assert float(y0.float().abs().max()) ** 2 * 256 < 2 ** 24            # a tile's sums are exact in fp32
    run = torch.arange(n_units, device=DEV) // per_wg
    sums = [torch.zeros((int(run[-1]) + 1, 2, C), dtype=torch.float64, device=DEV).index_add_(0, run, s.double()) for s in (s0, s1)]
    assert not bool(torch.isnan(sums[0]).any())
    assert torch.equal(sums[0], sums[1])
    if dtype == torch.float32:
        assert torch.equal(s0, s1)
    else:
        assert not torch.equal(s0, s1), "the staggered order was not taken"


# ---------------------------------------------------------------------------------------------------------------
# kernel size 1
# ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("regime", X.REGIMES)
@pytest.mark.parametrize("shape,dtype", [(n, d) for n in sorted(X.CONV1_SHAPES) for d in X.DTYPES
                                         if not (n.startswith("wide") and d == torch.float32)],       # conv1_wide has no fp32 form
                         ids=lambda v: v if isinstance(v, str) else name(v))
def test_conv1_tile_flat_and_wide_kernels(ops, shape, regime, dtype):
    """conv + bias as stored, and as the pre-activation kept under SDA_EPI_GELU, from the tile kernel (per-sample weights through
    widx), conv1_flat and conv1_wide (256- and 320-channel tilings, 16-bit only); SDA_EPI_ROW_SUMSQ in the exact regime."""
    from speech_decoding_amd import lib as L
    wide = shape.startswith("wide")
    case = X.conv1_case(shape, regime, dtype)
    s = case.shape
    Cin_p, Cout_p = L.pad_channels(s.cin), L.pad_channels(s.cout)
    xb = rows(ops, case.x, dtype)
    wp = weight(ops, case.w, Cout_p, Cin_p, dtype)
    bias = ops.pack_vector(case.bias.float().to(DEV), Cout_p)
    want = X.store(case.ref, dtype)
    kw = dict(B=s.B, T=s.T, KS=1, dil=0, bias=bias)
    if case.widx is not None:
        yb = ops.conv_gemm(xb, wp, ops.new_rows(s.B, s.T, Cout_p, dtype, DEV), widx=case.widx.to(DEV), **kw)
        X.assert_same(unrows(ops, yb, s.B, s.cout, s.T), want, f"conv1 {shape} widx")
        assert padding_is_zero(yb, s.B, s.cout, s.T)
        return
    kernels = [("tile", 0)]
    if ops.conv_kernel(1, Cout_p, L.CONV_FLAT_TILES, dtype) == L.CONV_KERNEL_FLAT1:
        kernels.append(("flat", L.CONV_FLAT_TILES))
    if wide:
        kernels.append(("wide", L.CONV_WIDE_TILES))
    assert len(kernels) == (3 if wide else 2)
    for label, flags in kernels:
        what = f"conv1 {shape} {regime} {name(dtype)} {label}"
        yb = ops.conv_gemm(xb, wp, ops.new_rows(s.B, s.T, Cout_p, dtype, DEV), flags=flags, **kw)
        X.assert_same(unrows(ops, yb, s.B, s.cout, s.T), want, what)
        assert padding_is_zero(yb, s.B, s.cout, s.T), what
        post, pre = ops.new_rows(s.B, s.T, Cout_p, dtype, DEV), ops.new_rows(s.B, s.T, Cout_p, dtype, DEV)
        ops.conv_gemm(xb, wp, post, y_pre=pre, gelu=True, flags=flags, **kw)
        X.assert_same(unrows(ops, pre, s.B, s.cout, s.T), want, what + " y_pre under GELU")
        assert padding_is_zero(pre, s.B, s.cout, s.T), what
        if regime == "exact" and label != "tile" and s.cout == Cout_p and Cout_p % (256 if label == "wide" else 128) == 0:
            parts = torch.full((L.rows_alloc(s.B, s.T), Cout_p // 128), NAN, device=DEV)
            yb = ops.conv_gemm(xb, wp, ops.new_rows(s.B, s.T, Cout_p, dtype, DEV), flags=flags, row_sumsq=parts, **kw)
            X.assert_same(unrows(ops, yb, s.B, s.cout, s.T), want, what + " with row sums of squares")
            ref = X.row_sumsq_ref(want)
            assert float(ref.max()) < 2 ** 24
            Tp = L.rows_tp(s.T)
            got = torch.stack([parts[b * Tp + L.ROW_PAD: b * Tp + L.ROW_PAD + s.T] for b in range(s.B)]).cpu()
            X.assert_same(got, ref, what + " row sums of squares", axes="btj")


# ---------------------------------------------------------------------------------------------------------------
# data gradient
# ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", X.DTYPES, ids=name)
@pytest.mark.parametrize("regime", X.REGIMES)
@pytest.mark.parametrize("i", range(len(X.DGRAD_SHAPES)), ids=lambda i: "x".join(map(str, X.DGRAD_SHAPES[i])))
def test_data_gradient_on_mode1_weights(ops, i, regime, dtype):
    from speech_decoding_amd import lib as L
    check_data_gradient(ops, i, regime, dtype, (0, L.CONV_SINGLE_TILE, L.CONV_PAIR_TILES, L.CONV_FLAT_TILES))


def check_data_gradient(ops, i, regime, dtype, tilings):
    """dx through conv_gemm on weights packed with mode 1, plain and in the GLU channel layout (the halves split at half_p)"""
    from speech_decoding_amd import lib as L
    case = X.dgrad_case(i, regime, dtype)
    s = case.shape
    half = s.cout // 2 if s.glu else 0
    half_p = L.pad_channels(half) if s.glu else 0
    Cin_p = L.pad_channels(s.cin)
    Cout_p = 2 * half_p if s.glu else L.pad_channels(s.cout)
    dy = case.dy
    if s.glu:
        dy = torch.zeros(s.B, Cout_p, s.T, dtype=torch.float64)
        dy[:, :half] = case.dy[:, :half]
        dy[:, half_p: half_p + s.cout - half] = case.dy[:, half:]
    dyb = rows(ops, dy, dtype, Cp=Cout_p)
    wt = weight(ops, case.w, Cout_p, Cin_p, dtype, mode=1, glu_half=half, glu_half_p=half_p)
    for flags in tilings:
        dxb = ops.conv_gemm(dyb, wt, ops.new_rows(s.B, s.T, Cin_p, dtype, DEV), B=s.B, T=s.T, KS=s.KS, dil=s.dil, flags=flags)
        what = f"dgrad {tuple(s)} {regime} {name(dtype)} flags {flags}"
        X.assert_same(unrows(ops, dxb, s.B, s.cin, s.T), X.store(case.ref, dtype), what)
        assert padding_is_zero(dxb, s.B, s.cin, s.T), what


# ---------------------------------------------------------------------------------------------------------------
# weight gradient
# ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", X.DTYPES, ids=name)
@pytest.mark.parametrize("i", range(len(X.WGRAD_SHAPES)), ids=lambda i: "x".join(map(str, X.WGRAD_SHAPES[i][:6])))
def test_wgrad_slabs_equal_the_integer_gradient(ops, i, dtype):
    """sda_wgrad_gemm + sda_reduce_slabs + unpack_conv_wgrad: one segment, per-subject segments through perm / seg_start, and
    SDA_WGRAD_FLAT_ROWS with and without perm — the fp32 slabs ARE the integer gradient in every summation order."""
    from speech_decoding_amd import lib as L
    case = X.wgrad_case(i)
    s = case.shape
    Cin_p, Cout_p = L.pad_channels(s.cin), L.pad_channels(s.cout)
    dyb, xb = rows(ops, case.dy, dtype), rows(ops, case.x, dtype)
    kw = dict(B=s.B, T=s.T, KS=s.KS, dil=s.dil)
    what = f"wgrad {tuple(s)[:6]} {name(dtype)}"

    def unpack(slabs, n):
        return ops.unpack_conv_wgrad(slabs, n, s.cout, s.cin, s.KS, Cout_p, Cin_p).cpu().double()

    total = X.wgrad_ref(case.dy, case.x, s.KS, s.dil)
    X.assert_same(unpack(ops.wgrad_gemm(dyb, xb, **kw), 1), total, what + " one segment", axes="sock")
    # per-subject segments (a subject absent from the batch gets an all-zero slab)
    sidx = np.array(s.subjects)
    order = np.argsort(sidx, kind="stable").astype(np.int32)
    seg = np.searchsorted(sidx[order], np.arange(X.WGRAD_NSUBJ + 1)).astype(np.int32)
    per_subject = X.wgrad_ref(case.dy, case.x, s.KS, s.dil, s.subjects, X.WGRAD_NSUBJ)
    pk = dict(kw, perm=torch.from_numpy(order).to(DEV), seg_start=torch.from_numpy(seg).to(DEV), nseg=X.WGRAD_NSUBJ)
    for flat in (False, True):
        slabs = ops.wgrad_gemm(dyb, xb, flat_rows=flat, **pk)
        X.assert_same(unpack(slabs, X.WGRAD_NSUBJ), per_subject, what + f" per subject, flat_rows={flat}", axes="sock")
        X.assert_same(unpack(ops.reduce_slabs(slabs)[None], 1), total, what + f" per subject reduced, flat_rows={flat}", axes="sock")
    # runs of consecutive samples, contracted per sample and as one run of rows
    edges = np.floor(np.linspace(0, s.B, 3)).astype(np.int32)
    run_of = np.searchsorted(edges, np.arange(s.B), side="right") - 1
    runs = X.wgrad_ref(case.dy, case.x, s.KS, s.dil, run_of, 2)
    for flat in (False, True):
        slabs = ops.wgrad_gemm(dyb, xb, seg_start=torch.from_numpy(edges).to(DEV), nseg=2, flat_rows=flat, **kw)
        X.assert_same(unpack(slabs, 2), runs, what + f" two runs, flat_rows={flat}", axes="sock")


@pytest.mark.parametrize("dtype", X.DTYPES, ids=name)
@pytest.mark.parametrize("regime", X.REGIMES)
@pytest.mark.parametrize("i", range(len(X.TYPED_SHAPES)))
def test_wgrad_typed_output_rounds_once(ops, i, regime, dtype):
    """out_e = out_scale * (acc_scale * acc - rscale * sub), everything into the fp32 accumulator, one rounding at the store"""
    from speech_decoding_amd import lib as L
    case = X.typed_case(i, regime, dtype)
    s = case.shape
    G = torch.zeros((s.M + 1, L.pad_channels(s.N)), dtype=dtype, device=DEV)
    G[:s.M, :s.N] = X.operand(case.G, dtype).to(DEV)
    Y, sub = X.operand(case.Y, dtype).to(DEV), X.operand(case.sub, dtype).to(DEV)
    out = torch.full((s.N, s.K), NAN, dtype=dtype, device=DEV)
    ops.matmul_tn_typed(G, Y, out, sub, case.rscale.float().to(DEV), M_rows=s.M, N_valid=s.N, K_cols=s.K, pitch=s.K,
                        out_scale=torch.tensor([case.out_scale], device=DEV), acc_scale=case.acc_scale.float().to(DEV))
    X.assert_same(out.cpu().double(), X.store(case.ref, dtype), f"typed wgrad {tuple(s)} {regime} {name(dtype)}", axes="jk")


# ---------------------------------------------------------------------------------------------------------------
# split-K and similarity GEMMs
# ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", X.DTYPES, ids=name)
@pytest.mark.parametrize("i", range(len(X.SIM_SHAPES)), ids=lambda i: "x".join(map(str, X.SIM_SHAPES[i])))
def test_splitk_and_sim_gemm_equal_the_integer_product(ops, i, dtype):
    """matmul_nt_splitk_into on conv_gemm's split-K matrix mode and on sim_gemm's 256 x 256 tiles (16-bit): M and N no multiples of
    a tile, a row pitch above K (the columns behind K hold sevens), one K slice and several."""
    from speech_decoding_amd import lib as L
    s = X.SIM_SHAPES[i]
    A, Bm, ref = X.sim_case(i)
    Np = L.pad_channels(s.N)
    xm = torch.full((s.M, s.pitch), 7.0, dtype=dtype, device=DEV)
    wm = torch.full((s.N, s.pitch), 7.0, dtype=dtype, device=DEV)
    xm[:, :s.K], wm[:, :s.K] = X.operand(A, dtype).to(DEV), X.operand(Bm, dtype).to(DEV)
    routes = [False] if dtype == torch.float32 else [False, True]
    for tiles256 in routes:
        if tiles256:
            assert L.load().sda_sim_gemm_ksplit(s.M, s.N, s.K, ops.dt_code(dtype)) > 0
        slab = 32 if (tiles256 or dtype == torch.float32) else 64
        for ks in X.SIM_KSPLITS:
            ks = min(ks, s.K // slab)
            partial = torch.full((ks, s.M, Np), NAN, device=DEV)
            out = torch.full((s.M, Np), NAN, device=DEV)
            ops.matmul_nt_splitk_into(xm, wm, s.M, s.N, s.K, s.pitch, tiles256, ks, partial, out)
            X.assert_same(out[:, :s.N].cpu().double(), ref, f"splitk {tuple(s)} {name(dtype)} tiles256={tiles256} ksplit={ks}", axes="ij")


# ---------------------------------------------------------------------------------------------------------------
# the loss's embedding gradient
# ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", X.DTYPES16, ids=name)
@pytest.mark.parametrize("regime", X.REGIMES)
@pytest.mark.parametrize("i", range(len(X.CLIP_SHAPES)), ids=lambda i: "x".join(map(str, X.CLIP_SHAPES[i])))
def test_clip_dz_and_typed_wgrad_agree_with_the_reference(ops, i, regime, dtype):
    """sda_clip_dz (coefficients in registers for Bm <= 256, 256 x 256 tiles above) and the same product through matmul_tn_typed:
    both equal the single-rounding reference, hence each other."""
    from speech_decoding_amd import lib as L
    case = X.clip_case(i, regime, dtype)
    s = case.shape
    Yt, Zt = rows(ops, case.Y, dtype), rows(ops, case.Z, dtype)
    Fp = Yt.shape[1]
    re = L.rows_tp(s.T) * Fp
    assert L.load().sda_clip_dz_supported(s.Bm, s.Bn, re, ops.dt_code(dtype))
    assert (s.Bm <= 256 and re % 64 == 0) or (s.Bm >= 256 and re % 256 == 0)
    G = torch.zeros((s.Bm + 1, L.pad_channels(s.Bn)), dtype=dtype, device=DEV)
    G[:s.Bm, :s.Bn] = X.operand(case.G, dtype).to(DEV)
    cs, rs = case.cscale.float().to(DEV), case.rscale.float().to(DEV)
    scale = torch.tensor([case.out_scale], device=DEV)
    want = X.store(case.ref, dtype)
    what = f"clip_dz {tuple(s)} {regime} {name(dtype)}"
    out = ops.new_rows_uninit(s.Bn, s.T, Fp, dtype, DEV)
    ops.clip_dz(G, Yt, Zt, out, rs, cs, Bm=s.Bm, Bn=s.Bn, row_elems=re, out_scale=scale)
    X.assert_same(ops.rows_view(out, s.Bn, s.F, s.T).cpu().double(), want, what + " streaming kernel")
    full, Tp = out.float().cpu(), L.rows_tp(s.T)
    for b in range(s.Bn):
        assert bool((full[b * Tp: b * Tp + L.ROW_PAD] == 0).all()), what
    old = ops.new_rows_uninit(s.Bn, s.T, Fp, dtype, DEV)
    ops.matmul_tn_typed(G, Yt, old, Zt, rs, M_rows=s.Bm, N_valid=s.Bn, K_cols=re, pitch=re, out_scale=scale, acc_scale=cs)
    X.assert_same(ops.rows_view(old, s.Bn, s.F, s.T).cpu().double(), want, what + " typed wgrad")


# ---------------------------------------------------------------------------------------------------------------
# the encoder's input gradient, the parameter GEMM
# ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("out_dtype", X.DTYPES, ids=lambda d: "out_" + name(d))
@pytest.mark.parametrize("dtype", X.DTYPES, ids=name)
@pytest.mark.parametrize("regime", X.REGIMES)
@pytest.mark.parametrize("i", range(len(X.IG_SHAPES)), ids=lambda i: "x".join(map(str, X.IG_SHAPES[i])))
def test_input_grad_per_sample_matrices(ops, i, regime, dtype, out_dtype):
    """sda_input_grad with nW > 1 through widx, C < Cp, Kp = 32 and Kp = 96 (three K chunks), every out_dtype"""
    from speech_decoding_amd import lib as L
    case = X.ig_case(i, regime, out_dtype)
    s = case.shape
    Gb = rows(ops, case.G, dtype)
    assert Gb.shape[1] >= s.Kp and s.C < s.Cp
    W = X.operand(case.W, dtype).to(DEV)
    widx = torch.tensor(X.IG_WIDX[i], dtype=torch.int32, device=DEV)
    got = ops.input_grad(Gb, W, widx, s.B, s.C, s.T, out_dtype)
    assert got.dtype == out_dtype and tuple(got.shape) == (s.B, s.C, s.T)
    X.assert_same(got.cpu().double(), X.store(case.ref, out_dtype), f"input_grad {tuple(s)} {regime} {name(dtype)} -> {name(out_dtype)}")


@pytest.mark.parametrize("form", X.PGEMM_FORMS)
def test_param_gemm_on_strided_views_of_integers(ops, form):
    A, B = X.pgemm_operands(form)
    Ad, Bd = A.float().to(DEV), B.float().to(DEV)
    out = buf = None
    if form == "a_transposed":
        Ad, A = Ad.t(), A.t()
    elif form == "batched_both_sliced":
        Ad, A = Ad[:, :270].transpose(1, 2), A[:, :270].transpose(1, 2)
        Bd, B = Bd[:, :270, :209], B[:, :270, :209]
    else:
        buf = torch.zeros((4, 1, 320, 256), dtype=torch.bfloat16, device=DEV)
        out = buf[:, 0, :270, :209]
    got = ops.param_gemm(Ad, Bd, out=out)
    ref = torch.matmul(A, B)
    assert float(ref.abs().max()) < 2 ** 24
    if out is None:
        assert got.dtype == torch.float32
        X.assert_same(got.cpu().double(), ref, f"param_gemm {form}", axes="bij"[-ref.dim():])
    else:
        X.assert_same(got.float().cpu().double(), X.store(ref, torch.bfloat16), f"param_gemm {form}", axes="bij")
        mask = torch.ones_like(buf, dtype=torch.bool)
        mask[:, 0, :270, :209] = False
        assert bool((buf[mask].float() == 0).all())
