"""The row-layout buffer contract, kernel by kernel, with reused (dirty) buffers.

The encoder hands the same workspace buffers to every step (EncoderEngine._rows), rotates three ping-pong buffers per padded
width in no-grad forwards (layers of different valid widths share one: D1 = 270 and D2 = 320 both pad to 320), and leaves the
valid rows of Z, dZ and gathered batches uninitialised (ops.new_rows_uninit).  Every consumer relies on three things:

  * a producer writes every valid row of its output, pad channels included: what a dirty buffer held before never shows;
  * the pad channels it writes are exactly 0 (the next layer of another valid width reads them as zero inputs);
  * it never writes a pad row (the 16 rows in front of each sample) or the slack behind the last sample: the k = 3 convs'
    halo and wgrad_gemm(flat_rows=True) contract across those rows as zeros.

Each entry point below runs twice on identical inputs: once into zero-filled outputs (as in test_kernels_gpu.py) and once into
outputs whose valid rows hold NaN across the full padded width (pad rows and slack zero, as new_rows_uninit leaves them).  The
two results must be bit-identical and the second must satisfy the three points above.  Scratch, statistics and split-K partial
buffers are filled with NaN in the second run as well: a kernel that reads a scratch word it did not write first fails."""
import math

import pytest
import torch

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
DTYPES = [torch.float32, torch.bfloat16, torch.float16]
NAN = float("nan")
# (Cin, Cout, T, B): channel counts that are not multiples of 64 (pad channels exist), T not a multiple of 128
SHAPES = [(270, 320, 129, 3), (40, 48, 130, 1), (300, 300, 360, 3)]


@pytest.fixture(scope="module")
def ops():
    from speech_decoding_amd import lib
    from speech_decoding_amd import ops as _ops
    lib.load()
    assert torch.cuda.is_available(), "these tests need the MI355X"
    return _ops


def _L():
    from speech_decoding_amd import lib as L
    return L


def q(x, dtype):
    return x.to(dtype).float()


def rows_of(ops, x, dtype, Cp=None):
    """(B, C, T) fp32 -> a zero-initialised row-layout buffer (the kernels' inputs are always clean here)."""
    B, C, T = x.shape
    buf = ops.new_rows(B, T, Cp or _L().pad_channels(C), dtype, DEV)
    ops.pack_rows(x.to(DEV), buf)
    return buf


def out_rows(ops, B, T, Cp, dtype, dirty):
    buf = ops.new_rows(B, T, Cp, dtype, DEV)
    if dirty:                                          # every valid row NaN across all Cp channels; pad rows + slack zero
        ops.rows_view(buf, B, Cp, T).fill_(NAN)
    return buf


def _bits(t):
    return t.view({4: torch.int32, 2: torch.int16, 1: torch.uint8}[t.element_size()])


def assert_same_bits(got, want, what):
    a, b = _bits(got), _bits(want)
    if not torch.equal(a, b):
        idx = tuple(int(i) for i in (a != b).nonzero()[0])
        raise AssertionError(f"{what}: dirty-buffer run differs from the clean run; first at index {idx}: "
                             f"{float(got[idx])} vs {float(want[idx])}")


def assert_rows_contract(buf, B, T, valid, what):
    """valid: list of (lo, hi) channel ranges that carry data; every other channel of a valid row, every pad row and the
    slack behind the last sample must be exactly 0."""
    L = _L()
    Tp, Cp = L.rows_tp(T), buf.shape[1]
    rowmask = torch.zeros(buf.shape[0], dtype=torch.bool, device=buf.device)
    for b in range(B):
        rowmask[b * Tp + L.ROW_PAD: b * Tp + L.ROW_PAD + T] = True
    chmask = torch.zeros(Cp, dtype=torch.bool, device=buf.device)
    for lo, hi in valid:
        chmask[lo:hi] = True
    full = buf.float()
    bad = (full != 0) & ~rowmask[:, None]
    if bool(bad.any()):
        r, c = (int(i) for i in bad.nonzero()[0])
        kind = "slack behind the last sample" if r >= B * Tp else f"pad row {r % Tp} of sample {r // Tp}"
        raise AssertionError(f"{what}: {kind} (row {r}, channel {c}) holds {float(full[r, c])}, not 0")
    bad = (full != 0) & rowmask[:, None] & ~chmask[None, :]
    if bool(bad.any()):
        r, c = (int(i) for i in bad.nonzero()[0])
        raise AssertionError(f"{what}: pad channel {c} of valid row {r} holds {float(full[r, c])}, not 0")


def run_both(ops, B, T, outs, scratch, launch):
    """outs: [(name, Cp, dtype, valid ranges)] row-layout outputs; scratch: [(name, shape, compared)] fp32 buffers (statistics /
    partials / scratch: `compared` = the launch writes all of it and its content is a result).  launch(o, s) -> dict of further
    results.  Runs clean then dirty and checks the contract."""
    res = {}
    for dirty in (False, True):
        o = {n: out_rows(ops, B, T, Cp, dt, dirty) for n, Cp, dt, _ in outs}
        s = {n: torch.full(shape, NAN if dirty else 0.0, dtype=torch.float32, device=DEV) for n, shape, _ in scratch}
        extra = launch(o, s) or {}
        res[dirty] = (o, s, extra)
    (oc, sc, ec), (od, sd, ed) = res[False], res[True]
    for n, Cp, dt, valid in outs:
        assert_same_bits(od[n], oc[n], n)
        assert_rows_contract(od[n], B, T, valid, n)
    for n, _, compared in scratch:
        if compared:
            assert_same_bits(sd[n], sc[n], n)
    for n in ec:
        assert_same_bits(ed[n], ec[n], n)
    return od, sd, ed


# ------------------------------------------------------------------------------------------------------------- conv_gemm
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("tiling", [4096, 8192, 16384])
@pytest.mark.parametrize("cin,cout,T,B", SHAPES)
def test_conv3_bias_residual_stats(ops, dtype, tiling, cin, cout, T, B):
    L = _L()
    g = torch.Generator().manual_seed(cin + T)
    Cip, Cop = L.pad_channels(cin), L.pad_channels(cout)
    xb = rows_of(ops, q(torch.randn(B, cin, T, generator=g), dtype), dtype)
    wp = ops.pack_conv_weight(q(torch.randn(cout, cin, 3, generator=g) / math.sqrt(3 * cin), dtype).to(DEV), Cop, Cip, dtype)
    bias = ops.pack_vector(torch.randn(cout, generator=g).to(DEV), Cop)
    res = xb if cin == cout else None
    nst = ops.conv_stats_rows(B, T, 3, Cop, tiling)

    def launch(o, s):
        ops.conv_gemm(xb, wp, o["y"], B=B, T=T, KS=3, dil=2, bias=bias, res=res, stats=s["stats"], flags=tiling)
    run_both(ops, B, T, [("y", Cop, dtype, [(0, cout)])], [("stats", (nst, 2, Cop), True)], launch)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("cin,half,T,B", [(270, 300, 129, 3), (320, 320, 360, 1)])
def test_conv3_glu_epilogue(ops, dtype, cin, half, T, B):
    L = _L()
    g = torch.Generator().manual_seed(half + T)
    Cip, Hp = L.pad_channels(cin), L.pad_channels(half)
    xb = rows_of(ops, q(torch.randn(B, cin, T, generator=g), dtype), dtype)
    w = q(torch.randn(2 * half, cin, 3, generator=g) / math.sqrt(3 * cin), dtype).to(DEV)
    b = torch.randn(2 * half, generator=g).to(DEV)
    plan = ops.PackPlan(dtype, DEV)
    plan.add_weight("w", w, 2 * Hp, Cip, glu_half=half, glu_half_p=Hp, glu_tile=80)
    plan.add_vector("b", b, 2 * Hp, glu_half=half, glu_half_p=Hp, glu_tile=80)
    pk = dict(plan.run({"w": w, "b": b}))

    def launch(o, s):
        ops.conv_gemm(xb, pk["w"], o["out"], B=B, T=T, KS=3, dil=4, bias=pk["b"], y_pre=o["gate"],
                      flags=L.CONV_FLAT_TILES | L.EPI_GLU)
    run_both(ops, B, T, [("out", Hp, dtype, [(0, half)]), ("gate", Hp, dtype, [(0, half)])], [], launch)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("KS,cin,H,T,B", [(3, 270, 300, 129, 3), (1, 600, 300, 130, 1), (3, 40, 48, 360, 3)])
def test_conv_glu_backward_epilogue(ops, dtype, KS, cin, H, T, B):
    L = _L()
    g = torch.Generator().manual_seed(KS + H + T)
    Cip, Hp = L.pad_channels(cin), L.pad_channels(H)
    xb = rows_of(ops, q(torch.randn(B, cin, T, generator=g), dtype), dtype)
    wp = ops.pack_conv_weight(q(torch.randn(H, cin, KS, generator=g) / math.sqrt(KS * cin), dtype).to(DEV), Hp, Cip, dtype)
    resb, outb, gateb = (rows_of(ops, q(torch.randn(B, H, T, generator=g), dtype), dtype) for _ in range(3))
    nst = ops.conv_stats_rows(B, T, KS, Hp, 0)

    def launch(o, s):
        ops.conv_gemm(xb, wp, o["dx"], B=B, T=T, KS=KS, dil=2 if KS == 3 else 0, res=resb, stats=s["stats"], glu_bwd=(outb, gateb))
    run_both(ops, B, T, [("dx", 2 * Hp, dtype, [(0, H), (Hp, Hp + H)])], [("stats", (nst, 2, Hp), True)], launch)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("store_dg", [False, True])
@pytest.mark.parametrize("tiling", [4096, 8192, 16384])
@pytest.mark.parametrize("cin,cout,T,B", SHAPES)
def test_conv3_bn_backward_statistics_epilogue(ops, dtype, store_dg, tiling, cin, cout, T, B):
    L = _L()
    g = torch.Generator().manual_seed(cin + cout + T)
    Cip, Cop = L.pad_channels(cin), L.pad_channels(cout)
    dyb = rows_of(ops, q(torch.randn(B, cin, T, generator=g), dtype), dtype)
    wp = ops.pack_conv_weight(q(torch.randn(cout, cin, 3, generator=g) / math.sqrt(3 * cin), dtype).to(DEV), Cop, Cip, dtype)
    res = dyb if cin == cout else None                 # the model's data-gradient convs: the conv's own input, or none
    h = rows_of(ops, q(torch.randn(B, cout, T, generator=g) * 1.3 + 0.2, dtype), dtype)
    gamma, beta = (torch.rand(cout, generator=g) + 0.5).to(DEV), (torch.rand(cout, generator=g) - 0.5).to(DEV)
    hs = ops.unpack_rows(h, B, cout, T)
    part = torch.zeros((1, 2, Cop), device=DEV)
    part[0, 0, :cout], part[0, 1, :cout] = hs.sum(dim=(0, 2)), (hs ** 2).sum(dim=(0, 2))
    *_, coef = ops.bn_finalize(part, 1, B * T, gamma, beta, torch.zeros(cout, device=DEV), torch.ones(cout, device=DEV), Cop,
                               True, want_bwd_coef=True)
    flags = tiling | (L.EPI_BN_STORE_DG if store_dg else 0)
    nst = ops.conv_stats_rows(B, T, 3, Cop, flags)

    def launch(o, s):
        ops.conv_gemm(dyb, wp, o["dg"], B=B, T=T, KS=3, dil=2, res=res, stats=s["stats"], bn_x=h, bn_coef=coef, flags=flags)
    run_both(ops, B, T, [("dg", Cop, dtype, [(0, cout)])], [("stats", (nst, 2, Cop), True)], launch)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("cin,cout,T,B", SHAPES)
def test_conv1_gelu_and_per_sample_weights(ops, dtype, cin, cout, T, B):
    L = _L()
    g = torch.Generator().manual_seed(cout + T)
    Cip, Cop = L.pad_channels(cin), L.pad_channels(cout)
    xb = rows_of(ops, q(torch.randn(B, cin, T, generator=g), dtype), dtype)
    w = q(torch.randn(3, cout, cin, 1, generator=g) / math.sqrt(cin), dtype).to(DEV)
    wp1, wps = ops.pack_conv_weight(w[0], Cop, Cip, dtype), ops.pack_conv_weight(w, Cop, Cip, dtype)
    bias = ops.pack_vector(torch.randn(cout, generator=g).to(DEV), Cop)
    widx = torch.tensor([2, 0, 1][:B], dtype=torch.int32, device=DEV)

    def launch(o, s):
        ops.conv_gemm(xb, wp1, o["g"], B=B, T=T, KS=1, dil=0, bias=bias, y_pre=o["u"], gelu=True)
        ops.conv_gemm(xb, wps, o["y"], B=B, T=T, KS=1, dil=0, widx=widx)
    valid = [(0, cout)]
    run_both(ops, B, T, [("g", Cop, dtype, valid), ("u", Cop, dtype, valid), ("y", Cop, dtype, valid)], [], launch)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("cin,cout,T,B", [(270, 300, 129, 3), (1000, 600, 130, 1), (300, 240, 360, 3)])
def test_conv1_flat_gelu_backward_epilogue(ops, dtype, cin, cout, T, B):
    L = _L()
    g = torch.Generator().manual_seed(cin + T)
    Cip, Cop = L.pad_channels(cin), L.pad_channels(cout)
    assert ops.conv_kernel(1, Cop, L.CONV_FLAT_TILES | L.EPI_GELU_BWD, dtype) == L.CONV_KERNEL_FLAT1
    xb = rows_of(ops, q(torch.randn(B, cin, T, generator=g), dtype), dtype)
    wp = ops.pack_conv_weight(q(torch.randn(cout, cin, 1, generator=g) / math.sqrt(cin), dtype).to(DEV), Cop, Cip, dtype)
    ub = rows_of(ops, q(torch.randn(B, cout, T, generator=g), dtype), dtype)
    flags = L.CONV_FLAT_TILES
    nst = ops.conv_stats_rows(B, T, 1, Cop, flags | L.EPI_GELU_BWD)

    def launch(o, s):
        ops.conv_gemm(xb, wp, o["du"], B=B, T=T, KS=1, dil=0, flags=flags, gelu_bwd_u=ub, stats=s["stats"])
    run_both(ops, B, T, [("du", Cop, dtype, [(0, cout)])], [("stats", (nst, 2, Cop), True)], launch)


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16])
@pytest.mark.parametrize("cin,cout,T,B", [(600, 1000, 129, 3), (300, 500, 360, 1)])
def test_conv1_wide_tiles_row_sumsq(ops, dtype, cin, cout, T, B):
    L = _L()
    g = torch.Generator().manual_seed(cout + T)
    Cip, Cop = L.pad_channels(cin), L.pad_channels(cout)
    assert ops.conv_kernel(1, Cop, L.CONV_WIDE_TILES | L.EPI_ROW_SUMSQ, dtype) == L.CONV_KERNEL_WIDE
    xb = rows_of(ops, q(torch.randn(B, cin, T, generator=g), dtype), dtype)
    wp = ops.pack_conv_weight(q(torch.randn(cout, cin, 1, generator=g) / math.sqrt(cin), dtype).to(DEV), Cop, Cip, dtype)
    bias = ops.pack_vector(torch.randn(cout, generator=g).to(DEV), Cop)

    def launch(o, s):
        ops.conv_gemm(xb, wp, o["z"], B=B, T=T, KS=1, dil=0, bias=bias, y_pre=o["u"], gelu=True, row_sumsq=s["parts"],
                      flags=L.CONV_WIDE_TILES)
        return {"norms": ops.rows_sumsq_from_row_parts(s["parts"], B, T)}
    valid = [(0, cout)]
    run_both(ops, B, T, [("z", Cop, dtype, valid), ("u", Cop, dtype, valid)],
             [("parts", (L.rows_alloc(B, T), Cop // 128), False)], launch)


# ------------------------------------------------------------------------------------------------- element-wise producers
def _bn_setup(ops, dtype, C, T, B, seed):
    L = _L()
    g = torch.Generator().manual_seed(seed)
    Cp = L.pad_channels(C)
    xb = rows_of(ops, q(torch.randn(B, C, T, generator=g) * 1.5 + 0.3, dtype), dtype)
    gamma, beta = (torch.rand(C, generator=g) + 0.5).to(DEV), (torch.rand(C, generator=g) - 0.5).to(DEV)
    xs = ops.unpack_rows(xb, B, C, T)
    part = torch.zeros((1, 2, Cp), device=DEV)
    part[0, 0, :C], part[0, 1, :C] = xs.sum(dim=(0, 2)), (xs ** 2).sum(dim=(0, 2))
    mean, rstd, scale, shift, coef = ops.bn_finalize(part, 1, B * T, gamma, beta, torch.zeros(C, device=DEV),
                                                     torch.ones(C, device=DEV), Cp, True, want_bwd_coef=True)
    return g, Cp, xb, gamma, beta, mean, rstd, scale, shift, coef


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("C,T,B", [(300, 129, 3), (48, 130, 1), (270, 360, 3)])
def test_bn_gelu_forward(ops, dtype, C, T, B):
    _, Cp, xb, _, _, _, _, scale, shift, _ = _bn_setup(ops, dtype, C, T, B, C)

    def launch(o, s):
        ops.bn_gelu_forward(xb, o["y"], scale, shift, B, T)
    run_both(ops, B, T, [("y", Cp, dtype, [(0, C)])], [], launch)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("mode", ["apply", "tile_stats", "dy_is_dg"])
@pytest.mark.parametrize("cin,C,T,B", [(270, 300, 129, 3), (40, 48, 130, 1), (320, 270, 360, 3)])
def test_bn_gelu_backward(ops, dtype, mode, cin, C, T, B):
    """apply: the stand-alone sums pass + the apply pass (reduce scratch poisoned too); tile_stats / dy_is_dg: the sums from the
    statistics rows of the data-gradient conv that wrote dy (with and without SDA_EPI_BN_STORE_DG)."""
    L = _L()
    g, Cp, hb, gamma, beta, mean, rstd, _, _, coef = _bn_setup(ops, dtype, C, T, B, C + 7)
    Cip = L.pad_channels(cin)
    xin = rows_of(ops, q(torch.randn(B, cin, T, generator=g), dtype), dtype)
    wp = ops.pack_conv_weight(q(torch.randn(C, cin, 3, generator=g) / math.sqrt(3 * cin), dtype).to(DEV), Cp, Cip, dtype)
    flags = L.CONV_PAIR_TILES | (L.EPI_BN_STORE_DG if mode == "dy_is_dg" else 0)
    st = torch.empty((ops.conv_stats_rows(B, T, 3, Cp, flags), 2, Cp), dtype=torch.float32, device=DEV)
    dy = ops.conv_gemm(xin, wp, ops.new_rows(B, T, Cp, dtype, DEV), B=B, T=T, KS=3, dil=1, stats=st, bn_x=hb, bn_coef=coef,
                       flags=flags)

    def launch(o, s):
        dgam, dbet = ops.bn_gelu_backward(dy, hb, mean, rstd, gamma, beta, o["dx"], B, T, s["scratch"],
                                          tile_stats=None if mode == "apply" else st, dy_is_dg=mode == "dy_is_dg")
        return {"dgamma": dgam, "dbeta": dbet}
    run_both(ops, B, T, [("dx", Cp, dtype, [(0, C)])], [("scratch", (_L().load().sda_reduce_scratch_floats(Cp),), False)], launch)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("H,T,B", [(300, 129, 3), (48, 130, 1), (320, 360, 3)])
def test_glu_and_gelu_passes(ops, dtype, H, T, B):
    """glu_forward, glu_backward, gelu_backward and the column-sum forms (glu_backward_colsum, glu_backward_colsum_og,
    gelu_backward_colsum, colsum) whose reduce scratch is poisoned as well."""
    L = _L()
    g = torch.Generator().manual_seed(H + T)
    Hp = L.pad_channels(H)
    packed = torch.zeros(B, 2 * Hp, T)
    packed[:, :H], packed[:, Hp: Hp + H] = torch.randn(B, H, T, generator=g), torch.randn(B, H, T, generator=g)
    x2 = rows_of(ops, q(packed, dtype), dtype, Cp=2 * Hp)                     # [value | gate] as the conv writes it
    dy, u, outb, gateb = (rows_of(ops, q(torch.randn(B, H, T, generator=g), dtype), dtype) for _ in range(4))
    nscr = L.load().sda_reduce_scratch_floats(2 * Hp)
    glu2 = [(0, H), (Hp, Hp + H)]

    def launch(o, s):
        ops.glu_forward(x2, o["glu_y"], B, T)
        ops.glu_backward(x2, dy, o["glu_dx"], B, T)
        ops.gelu_backward(u, dy, o["gelu_du"], B, T)
        return {"cs_glu": ops.glu_backward_colsum(x2, dy, o["glu_dx_cs"], B, T, s["s0"]),
                "cs_og": ops.glu_backward_colsum_og(outb, gateb, dy, o["og_dx"], B, T, s["s1"]),
                "cs_gelu": ops.gelu_backward_colsum(u, dy, o["gelu_du_cs"], B, T, s["s2"]),
                "colsum": ops.colsum(dy, B, T, s["s3"])}
    outs = [("glu_y", Hp, dtype, [(0, H)]), ("glu_dx", 2 * Hp, dtype, glu2), ("gelu_du", Hp, dtype, [(0, H)]),
            ("glu_dx_cs", 2 * Hp, dtype, glu2), ("og_dx", 2 * Hp, dtype, glu2), ("gelu_du_cs", Hp, dtype, [(0, H)])]
    run_both(ops, B, T, outs, [(f"s{i}", (nscr,), False) for i in range(4)], launch)


# ------------------------------------------------------------------------------------------- layout changes and the loss
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("C,T,B", [(270, 129, 3), (40, 130, 1), (300, 360, 3)])
def test_pack_rows_and_gather_samples(ops, dtype, C, T, B):
    L = _L()
    g = torch.Generator().manual_seed(C + T)
    Cp, Tp = L.pad_channels(C), L.rows_tp(T)
    x = torch.randn(B, C, T, generator=g).to(DEV)
    N = 5
    table = torch.zeros((N * Tp + L.rows_alloc(1, T) - Tp, Cp), dtype=dtype, device=DEV)
    ops.pack_rows(torch.randn(N, C, T, generator=g).to(DEV), table)
    idx = torch.tensor([4, 0, 4][:B], dtype=torch.int64, device=DEV)

    def launch(o, s):
        ops.pack_rows(x, o["packed"])
        ops.pack_rows(x, o["packed_ones"], ones_channel=C)
        L.check(L.load().sda_gather_samples(table.data_ptr(), idx.data_ptr(), o["gathered"].data_ptr(), B,
                                            Tp * Cp * table.element_size(), ops._st()), "gather_samples")
    run_both(ops, B, T, [("packed", Cp, dtype, [(0, C)]), ("packed_ones", Cp, dtype, [(0, C + 1)]),
                         ("gathered", Cp, dtype, [(0, C)])], [], launch)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("B,F,T", [(6, 48, 130), (3, 300, 129), (12, 1000, 40)])
def test_clip_dz_rows(ops, dtype, B, F, T):
    """The loss's embedding gradient dZ (CLIPLoss.backward writes it into new_rows_uninit)."""
    from speech_decoding_amd import clip
    L = _L()
    g = torch.Generator().manual_seed(B + F)
    Fp = L.pad_channels(F)
    Y = q(torch.randn(B, F, T, generator=g), dtype)
    Yt, Zt = rows_of(ops, Y, dtype), rows_of(ops, q(0.3 * Y + torch.randn(B, F, T, generator=g), dtype), dtype)
    _, _, _, ctx = clip.clip_forward(Yt, Zt, torch.tensor([2.0], device=DEV), Bm=B, Bn=B, T=T)

    def launch(o, s):
        clip.clip_backward(ctx, o["dZ"])
    run_both(ops, B, T, [("dZ", Fp, dtype, [(0, F)])], [], launch)


# ---------------------------------------------------------------------------------------------- scratch and partial buffers
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("B,C,T", [(6, 300, 129), (1, 48, 130), (13, 1000, 40)])
def test_rows_sumsq_scratch(ops, dtype, B, C, T):
    L = _L()
    g = torch.Generator().manual_seed(B + C)
    xb = rows_of(ops, q(torch.randn(B, C, T, generator=g), dtype), dtype)
    row_elems = L.rows_tp(T) * xb.shape[1]

    def launch(o, s):
        out = torch.empty(B, dtype=torch.float32, device=DEV)
        L.check(L.load().sda_rows_sumsq(xb.data_ptr(), out.data_ptr(), s["scratch"].data_ptr(), B, row_elems, row_elems,
                                        ops.dt_code(dtype), ops._st()), "rows_sumsq")
        return {"sumsq": out}
    _, _, e = run_both(ops, B, T, [], [("scratch", (B * 64,), False)], launch)
    ref = ops.unpack_rows(xb, B, C, T).double().pow(2).sum(dim=(1, 2))
    torch.testing.assert_close(e["sumsq"].double(), ref, rtol=1e-5, atol=0)


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16])
@pytest.mark.parametrize("M,N,K,pitch", [(300, 200, 4096, 4096 + 64), (64, 24, 2048, 2048), (256, 256, 16384, 16384)])
def test_sim_gemm_partials(ops, dtype, M, N, K, pitch):
    L = _L()
    g = torch.Generator().manual_seed(M + N)
    xm = torch.randn(M, pitch, generator=g).to(dtype).to(DEV)
    wm = torch.randn(N, pitch, generator=g).to(dtype).to(DEV)
    Np = L.pad_channels(N)
    ks = L.load().sda_sim_gemm_ksplit(M, N, K, ops.dt_code(dtype))
    assert ks > 0

    def launch(o, s):
        L.check(L.load().sda_sim_gemm(xm.data_ptr(), wm.data_ptr(), s["partial"].data_ptr(), M, N, Np, K, pitch, ks,
                                      ops.dt_code(dtype), ops._st()), "sim_gemm")
        red = ops.reduce_slabs(s["partial"]) if ks > 1 else s["partial"][0]
        return {"S": red[:, :N].contiguous()}                # columns [N, Np) are documented don't-care
    _, _, e = run_both(ops, 1, 1, [], [("partial", (ks, M, Np), False)], launch)
    ref = xm[:, :K].double() @ wm[:, :K].double().t()
    torch.testing.assert_close(e["S"].double(), ref, rtol=1e-4, atol=1e-3 * math.sqrt(K))


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("cin,cout,T", [(300, 320, 129), (1000, 600, 130)])
def test_split_k_partials(ops, dtype, cin, cout, T):
    """linear_rows: conv_gemm's split-K slabs + the epilogue kernel that sums them (bias, GELU, residual), one sample."""
    L = _L()
    g = torch.Generator().manual_seed(cin + cout)
    Cip, Cop = L.pad_channels(cin), L.pad_channels(cout)
    xb = rows_of(ops, q(torch.randn(1, cin, T, generator=g), dtype), dtype)
    wp = ops.pack_conv_weight(q(torch.randn(cout, cin, 1, generator=g) / math.sqrt(cin), dtype).to(DEV), Cop, Cip, dtype)
    bias = ops.pack_vector(torch.randn(cout, generator=g).to(DEV), Cop)
    res = rows_of(ops, q(torch.randn(1, cout, T, generator=g), dtype), dtype)
    ksplit = ops.linear_rows_ksplit(T, Cop, Cip, dtype)
    assert ksplit >= 2

    def launch(o, s):
        ops.linear_rows(xb, wp, o["y"], T, bias=bias, res=res, gelu=True, scratch=s["partial"])
    run_both(ops, 1, T, [("y", Cop, dtype, [(0, cout)])], [("partial", (ksplit * T * Cop,), False)], launch)
