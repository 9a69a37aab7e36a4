"""inf / NaN propagation and containment of every kernel that moves a gradient in backward, on a real MI355X, through the ops
wrappers and in the compute dtypes each kernel serves.  A swallowed overflow does not crash: it feeds Adam a wrong, finite
gradient, and fp16's overflow guard (tests/test_overflow_guard_gpu.py) only works if the inf or NaN of an overflowed activation
gradient reaches a parameter gradient.  Poison values, named positions, the two checks and the restatements are in
tests/nonfinite_cases.py; tests/test_nonfinite_cpu.py shows that the checks catch a NaN-skipping soft-max, a saturating store, a
mask applied by multiplication and a column sum that skips non-finite terms.

The reference of every case is the restatement the kernel's own accuracy test uses (tests/elementwise_cases.py,
tests/exact_cases.py, tests/sa_loss_cases.py), evaluated on the poisoned operands as the kernel reads them; only its isfinite
mask is compared.  The incoming gradient is poisoned at every named position, a saved activation once per operand.

Kernel -> test:
  colsum, gelu_backward(_colsum), glu_backward(_colsum, _colsum_og)               test_elementwise_backward_passes, test_glu_backward_og_product_...
  bn_gelu_backward: apply, from_stats, _dg, and the first two in eval mode        test_bn_gelu_backward
  mse_backward                                                                    test_mse_backward
  reduce_slabs, reduce_unpack_wgrad (16-byte and element paths)                   test_slab_reduce_and_unpack, test_wgrad_gemm_and_its_reductions
  conv_gemm as data gradient on mode-1 weights: plain, every tiling               test_conv3_data_gradient_on_mode1_weights
    + GELU backward (tile, flat, wide), GLU backward, BatchNorm statistics        test_conv1_..._gelu_backward_epilogue, test_conv3_..._epilogue
  wgrad_gemm: one segment, flat rows, per-sample segments, typed output           test_wgrad_gemm_and_its_reductions, test_wgrad_typed_output
  input_grad (nW 2, Kp 96), param_gemm                                            test_input_grad_per_sample_matrices, test_param_gemm
  clip_logits_stats, clip_grad, clip_grad_y + clip_grad_y_finish, clip_dz         test_clip_*
  sa_softmax_backward, sa_weights_backward                                        test_sa_softmax_backward_and_weights_backward
  (forward, same file's maxima) sa_weights_forward, clip_merge_rows               test_sa_weights_forward, test_clip_merge_rows
  eval-mode BrainEncoder (Z and dX), retrieve                                     test_eval_mode_encoder_..., test_retrieve_...
and in tests/test_nonfinite_losses_gpu.py (the losses with labels, the sigmoid loss, extra negatives):
  clip_logits_stats_masked (rows and columns kernels), clip_grad_labels,          test_labelled_clip_kernels
    clip_grad_y_labels: positive and mask mode, fp32 / bf16 / fp16 G and Gy
  sigmoid_grad_y (labels, both modes), sigmoid_pairs + sigmoid_finish (mask)      test_sigmoid_loss_kernels
    (positive mode of the pair: tests/test_sigmoid_loss_gpu.py::test_nonfinite_inputs_propagate)
  clip_neg_stats, clip_neg_grad (with clip_neg_dtemp behind it)                   test_negatives_scalar_kernels
  clip_dz_windows                                                                 test_clip_dz_windows
  sim_gemm_windows, sim_gemm (256 x 256 tiles; kernel's K split and one slice)    test_sim_gemm_windows_and_sim_gemm"""
import pytest
import torch

from tests import builders as TB
from tests import elementwise_cases as E
from tests import exact_cases as X
from tests import nonfinite_cases as N
from tests import sa_loss_cases as S

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
F32 = torch.float32
DTYPES = E.DTYPES
DTYPES16 = X.DTYPES16


@pytest.fixture(scope="module")
def ops():
    from speech_decoding_amd import ops as _ops
    from speech_decoding_amd import lib
    lib.load()
    assert torch.cuda.is_available(), "these tests need the MI355X"
    return _ops


def name(dtype):
    return str(dtype).replace("torch.", "")


def host(t):
    torch.cuda.synchronize()
    return t.detach().cpu()


def run_cases(kernel, run, ref, operands, sites, dtype, typed=(), values=None):
    """run(o) -> {output: tensor}, ref(o) -> {output: tensor as stored}; sites: (what, operand, index) to poison, one at a time, with
    every poison value.  `typed` operands live in `dtype` on the device: the reference sees them as rounded (a 1e5 handed to an
    fp16 operand IS an inf)."""
    seen = lambda o: {k: (E.q(v, dtype) if k in typed else v) for k, v in o.items()}
    return N.run_cases(kernel, run, ref, operands, sites, N.poisons(dtype) if values is None else values, name(dtype), seen=seen)


def sites_of(key, pos, index_of):
    return [(what, key, index_of(*btc)) for what, btc in pos.items()]


# ---------------------------------------------------------------------------------------------------------------
# elementwise passes and column sums (csrc/elementwise.hip): independent per element, sums per channel
# ---------------------------------------------------------------------------------------------------------------
EW = (3, 11, 64)            # the reducers' smallest shape: 33 rows = two 17-row blocks of the column sums (valid row 17 = sample 1, t = 6)


def up(valid, B, T, dtype):
    buf = torch.zeros((E.L.rows_alloc(B, T), valid.shape[1]), dtype=dtype, device=DEV)
    buf[E.mem_rows(B, T).to(DEV)] = valid.to(dtype).to(DEV)
    return buf


def out_buf(B, T, W, dtype):
    return torch.full((E.L.rows_alloc(B, T), W), E.SENT, dtype=dtype, device=DEV)


def valid_rows(buf, B, T):
    return host(buf)[E.mem_rows(B, T)]


def ew_positions():
    B, T, C = EW
    return N.positions(B, T, C, t_edges=(6,))


ELEMENTWISE = ("colsum", "gelu_backward", "gelu_backward_colsum", "glu_backward", "glu_backward_colsum", "glu_backward_colsum_og")


@pytest.mark.parametrize("dtype", DTYPES, ids=name)
@pytest.mark.parametrize("kernel", ELEMENTWISE)
def test_elementwise_backward_passes(ops, kernel, dtype):
    B, T, C = EW
    o = E.real_operands(B * T, C, dtype)
    o = dict(x=o["x"], d=o["d"], val=o["val"], gate=o["gate"], out=E.q((o["val"].double() * E.sig64(o["gate"])).float(), dtype))
    scratch = ops.reduce_scratch(2 * C, DEV)
    u = lambda v: up(v, B, T, dtype)
    st = lambda r: N.stored(r, dtype)

    def run(o):
        if kernel == "colsum":
            return {"colsum": host(ops.colsum(u(o["d"]), B, T, scratch))}
        if kernel == "gelu_backward":
            return {"du": valid_rows(ops.gelu_backward(u(o["x"]), u(o["d"]), out_buf(B, T, C, dtype), B, T), B, T)}
        if kernel == "gelu_backward_colsum":
            du = out_buf(B, T, C, dtype)
            cs = ops.gelu_backward_colsum(u(o["x"]), u(o["d"]), du, B, T, scratch)
            return {"du": valid_rows(du, B, T), "colsum": host(cs)}
        dx = out_buf(B, T, 2 * C, dtype)
        xg = u(torch.cat([o["val"], o["gate"]], 1))
        if kernel == "glu_backward":
            return {"dx": valid_rows(ops.glu_backward(xg, u(o["d"]), dx, B, T), B, T)}
        if kernel == "glu_backward_colsum":
            cs = ops.glu_backward_colsum(xg, u(o["d"]), dx, B, T, scratch)
        else:
            cs = ops.glu_backward_colsum_og(u(o["out"]), u(o["gate"]), u(o["d"]), dx, B, T, scratch)
        return {"dx": valid_rows(dx, B, T), "colsum": host(cs)}

    def ref(o):
        if kernel == "colsum":
            return {"colsum": N.stored(o["d"].double().sum(0), None)}
        if kernel.startswith("gelu"):
            r = E.ref_gelu_backward(o["x"], o["d"], dtype)[0]
        elif kernel.endswith("_og"):
            r = E.ref_glu_backward_og(o["out"], o["gate"], o["d"], dtype)[0]
        else:
            r = E.ref_glu_backward(o["val"], o["gate"], o["d"], dtype)[0]
        out = {"du" if kernel.startswith("gelu") else "dx": st(r)}
        if "colsum" in kernel:
            out["colsum"] = N.stored(r.sum(0), None)           # the fused sums add the fp32 values before the store
        return out

    row = lambda b, t, c: (b * T + t, c)
    sites = sites_of("d", ew_positions(), row)
    first = (0, 0)
    if kernel.startswith("gelu"):
        sites.append(("the saved pre-activation, first row, channel 0", "x", first))
    elif kernel.endswith("_og"):
        sites += [("the saved output, first row, channel 0 (out half)", "out", first),
                  ("the saved gate, last row, channel C - 1 (gate half)", "gate", (B * T - 1, C - 1))]
    elif kernel.startswith("glu"):
        sites += [("the saved value, first row, channel 0 (out half)", "val", first),
                  ("the saved gate, last row, channel C - 1 (gate half)", "gate", (B * T - 1, C - 1))]
    assert run_cases(kernel, run, ref, o, sites, dtype, typed=("x", "d", "val", "gate", "out")) >= 12


def test_glu_backward_og_product_that_overflows_fp16(ops):
    """dy = 1000, out = 100, gate = -100 (1 - sigmoid = 1 exactly): d gate = 1e5 in the fp32 registers, inf as stored, and 1e5
    in the fused fp32 column sum"""
    B, T, C = EW
    dtype = torch.float16
    o = E.integer_operands(B * T, C)
    o = dict(out=o["val"], gate=o["gate"], d=o["d"])
    for k, v in (("gate", -100.0), ("out", 1.0), ("d", 1.0)):          # (positive, so that the zero of d value keeps its sign)
        o[k][B * T - 1, C - 1] = v
    scratch = ops.reduce_scratch(2 * C, DEV)

    def run(o):
        dx = out_buf(B, T, 2 * C, dtype)
        cs = ops.glu_backward_colsum_og(up(o["out"], B, T, dtype), up(o["gate"], B, T, dtype), up(o["d"], B, T, dtype), dx, B, T, scratch)
        return {"dx": valid_rows(dx, B, T), "colsum": host(cs)}

    def ref(o):
        r = E.ref_glu_backward_og(o["out"], o["gate"], o["d"], dtype)[0]
        return {"dx": N.stored(r, dtype), "colsum": N.stored(r.sum(0), None)}

    big = dict(o, out=N.poisoned(o["out"], (B * T - 1, C - 1), 100.0), d=N.poisoned(o["d"], (B * T - 1, C - 1), 1000.0))
    r = ref(big)
    assert float(E.ref_glu_backward_og(big["out"], big["gate"], big["d"], dtype)[0][B * T - 1, 2 * C - 1]) == pytest.approx(1e5, rel=1e-12)
    assert int((~torch.isfinite(r["dx"])).sum()) == 1 and bool(torch.isfinite(r["colsum"]).all())
    N.check_all("glu_backward_colsum_og", r, run(big), run(o), ref(o), "fp16, dy * out = 1e5")


# ---------------------------------------------------------------------------------------------------------------
# BatchNorm + GELU backward (C 24 of 64 padded channels, T 40): training mode couples a channel, nothing else
# ---------------------------------------------------------------------------------------------------------------
BN = (3, 40, 24)


def bn_restatement(o, dtype, form):
    """E.ref_bn_backward's closed form on given mean / rstd (the kernels are handed them), without its autograd cross-check (NaN
    fails any comparison).  form "apply": the sums come from dy and x; "from_stats" / "dg": from the statistics rows the conv
    that wrote dy left (dg: dy already holds dg = dy GELU'(z))."""
    x, dy, gamma, beta, mean, rstd = (o[k].double() for k in ("x", "dy", "gamma", "beta", "mean", "rstd"))
    n = x.shape[0]
    xhat = (x - mean) * rstd
    eval_mode, form = form.endswith(", eval mode"), form.replace(", eval mode", "")
    dg = dy if form == "dg" else dy * E.ggrad64(gamma * xhat + beta)
    if form == "apply":
        dbeta, dgamma = dg.sum(0), (dg * xhat).sum(0)
    else:
        dbeta, dgamma = o["stats"][:, 0].double().sum(0), o["stats"][:, 1].double().sum(0)
    # eval mode (running statistics): no batch-statistics terms, every element on its own; dgamma and dbeta stay the plain sums
    dx = gamma * rstd * (dg if eval_mode else dg - dbeta / n - xhat * dgamma / n)
    return {"dx": N.stored(dx, dtype), "dgamma": N.stored(dgamma, None), "dbeta": N.stored(dbeta, None)}


@pytest.mark.parametrize("dtype", DTYPES, ids=name)
@pytest.mark.parametrize("form", ["apply", "from_stats", "dg", "apply, eval mode", "from_stats, eval mode"])
def test_bn_gelu_backward(ops, form, dtype):
    """training mode couples a channel through its two sums and nothing else; eval mode (count = inf: the engine's way of
    dropping the batch-statistics terms) couples nothing: a poisoned element reaches dx at its own place and its channel's
    dgamma / dbeta"""
    eval_mode, form = form.endswith(", eval mode"), form.replace(", eval mode", "")
    tag = form + (", eval mode" if eval_mode else "")
    B, T, C = BN
    Cp = E.L.pad_channels(C)
    case = E.bn_backward_case(B, T, C, dtype, designed=False)
    r = E.ref_bn_backward(case, dtype, form == "dg")
    o = dict(x=case["x"], dy=E.q(r["dg"].float(), dtype) if form == "dg" else case["dy"], gamma=case["gamma"], beta=case["beta"],
             mean=r["mean"].float(), rstd=r["rstd"].float())
    tot = torch.stack([r["dbeta"], r["dgamma"]]).float()
    o["stats"] = torch.stack([tot * 0.5, tot * 0.25, tot * 0.25])            # three statistics rows that add up to the batch sums
    padc = lambda v: torch.cat([v, torch.zeros(v.shape[:-1] + (Cp - C,))], -1)
    scratch = ops.reduce_scratch(Cp, DEV)

    def run(o):
        dx = out_buf(B, T, Cp, dtype)
        f = lambda v: v.float().to(DEV)
        kw = {} if form == "apply" else dict(tile_stats=f(padc(o["stats"])), dy_is_dg=form == "dg")
        if eval_mode:
            kw["count"] = float("inf")
        dgamma, dbeta = ops.bn_gelu_backward(up(padc(o["dy"]), B, T, dtype), up(padc(o["x"]), B, T, dtype), f(padc(o["mean"])), f(padc(o["rstd"])),
                                             f(o["gamma"]), f(o["beta"]), dx, B, T, scratch, **kw)
        return {"dx": valid_rows(dx, B, T)[:, :C], "dgamma": host(dgamma)[:C], "dbeta": host(dbeta)[:C]}

    row = lambda b, t, c: (b * T + t, c)
    sites = sites_of("dy", N.positions(B, T, C, t_edges=(20,)), row)
    sites.append(("the saved BatchNorm input, first row, channel C - 1", "x", (0, C - 1)))
    if form != "apply":
        sites += [("the statistics rows: sum dg, last row, channel 0", "stats", (2, 0, 0)),
                  ("the statistics rows: sum dg xhat, first row, channel C - 1", "stats", (0, 1, C - 1))]
    run_cases(f"bn_gelu_backward[{tag}]", run, lambda o: bn_restatement(o, dtype, tag), o, sites, dtype, typed=("x", "dy"))


# ---------------------------------------------------------------------------------------------------------------
# MSE backward (csrc/mse_loss.hip): elementwise in z and y, everything scaled by dloss
# ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("ydtype", DTYPES, ids=lambda d: "y_" + name(d))
@pytest.mark.parametrize("zdtype", DTYPES, ids=lambda d: "z_" + name(d))
def test_mse_backward(ops, zdtype, ydtype):
    """z in the row layout (what the encoder hands out), y a plain (B, F, T) tensor, dz and dy each in its operand's type: a
    fp32 z of 1e5 overflows the fp16 dy and leaves the fp32 dz finite"""
    B, F, T = 3, 80, 40
    Fp = E.L.pad_channels(F)
    g = torch.Generator().manual_seed(B + F + T)
    y = torch.randn(B, F, T, generator=g)
    o = dict(y=E.q(y, ydtype), z=E.q(torch.randn(B, F, T, generator=g) * 0.7 + 0.2 * y, zdtype), dloss=torch.tensor([3.0]))

    def run(o):
        zb = ops.pack_rows(o["z"].to(zdtype).to(DEV), ops.new_rows(B, T, Fp, zdtype, DEV))
        yd = o["y"].to(ydtype).to(DEV)
        dz, dy = ops.new_rows(B, T, Fp, zdtype, DEV), torch.full_like(yd, E.SENT)
        ops.mse_backward(zb, yd, B, F, T, B, o["dloss"].to(DEV), dz, dy)
        return {"dz": host(ops.rows_view(dz, B, F, T)), "dy": host(dy)}

    def ref(o):
        d = 2.0 * (o["dloss"].double() / B) * (E.q(o["z"], zdtype).double() - E.q(o["y"], ydtype).double())
        return {"dz": N.stored(d, zdtype), "dy": N.stored(-d, ydtype)}

    pos = N.positions(B, T, F)
    at = lambda b, t, c: (b, c, t)
    sites = [("the incoming gradient", "dloss", (0,))] + sites_of("z", pos, at) + [("the target, last row, channel 0", "y", (B - 1, 0, T - 1))]
    values = dict(N.POISONS)
    if zdtype == F32:
        values.update({k: v for d in (ydtype,) for k, v in N.poisons(d).items()})
    run_cases("mse_backward", run, ref, o, sites, zdtype, values=values)


# ---------------------------------------------------------------------------------------------------------------
# weight-gradient slabs: reduce_slabs, reduce_unpack_wgrad (16-byte and element paths)
# ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("Cout,Cin,half,half_p", [(48, 40, 0, 0), (70, 64, 35, 64)])
@pytest.mark.parametrize("KS", E.WGRAD_KS)
def test_slab_reduce_and_unpack(ops, KS, Cout, Cin, half, half_p):
    """9 slabs (one more than a thread's unrolled 8): a poison in one slab element reaches exactly that element of the gradient;
    Cin 40 with KS 3 takes the 16-byte kernel, the same slabs 4 bytes into their allocation the element path"""
    nslabs = 9
    slabs = E.wgrad_case(nslabs, KS, Cout, Cin, half, half_p)
    Cout_p, Cin_p = slabs.shape[2], slabs.shape[3]

    def run(o):
        dev = o["slabs"].to(DEV)
        shifted = torch.empty(dev.numel() + 1, device=DEV)[1:].view(dev.shape)
        shifted.copy_(dev)
        assert dev.data_ptr() % 16 == 0 and shifted.data_ptr() % 16 == 4
        return {"reduce_unpack_wgrad": host(ops.reduce_unpack_wgrad(dev, Cout, Cin, KS, half, half_p)),
                "reduce_unpack_wgrad, element path": host(ops.reduce_unpack_wgrad(shifted, Cout, Cin, KS, half, half_p)),
                "reduce_slabs": host(ops.reduce_slabs(dev))}

    def ref(o):
        s = o["slabs"]
        g = torch.stack([torch.stack([s[:, tap, E.glu_map(co, half, half_p), :Cin].double().sum(0) for tap in range(KS)], -1)
                         for co in range(Cout)])
        g = N.stored(g, None)
        return {"reduce_unpack_wgrad": g, "reduce_unpack_wgrad, element path": g, "reduce_slabs": N.stored(s.double().sum(0), None)}

    last_row = E.glu_map(Cout - 1, half, half_p)
    sites = [("first slab, first tap, row 0, column 0", "slabs", (0, 0, 0, 0)),
             ("last slab, last tap, the last real row and column", "slabs", (nslabs - 1, KS - 1, last_row, Cin - 1)),
             ("the ninth slab (past the unrolled eight), row 1, column 5", "slabs", (8, 0, 1, 5))]
    if half:
        sites.append(("the last row of the out half, next to the pad rows between the halves", "slabs", (3, 0, half - 1, 2)))
    run_cases("reduce_slabs / reduce_unpack_wgrad", run, ref, dict(slabs=slabs), sites, F32)


# ---------------------------------------------------------------------------------------------------------------
# the matrix-core kernels on the integer operands of tests/exact_cases.py: the reference is exact, and so is its mask
# ---------------------------------------------------------------------------------------------------------------
def rows(ops, t, dtype, Cp=None):
    """(B, C, T) values -> row-layout buffer of `dtype`"""
    B, C, T = t.shape
    buf = ops.new_rows(B, T, Cp or E.L.pad_channels(C), dtype, DEV)
    return ops.pack_rows(t.to(dtype).to(DEV), buf)


def unrows(ops, buf, B, C, T):
    """the stored values, in the buffer's own type"""
    return host(ops.unpack_rows(buf, B, C, T, buf.dtype))


def bct(b, t, c):
    return (b, c, t)


@pytest.mark.parametrize("dtype", DTYPES, ids=name)
def test_conv3_data_gradient_on_mode1_weights(ops, dtype):
    """(cin 40, cout 48, dil 2, T 70, B 3): every tiling of the tile kernel and the flat kernel, whose 256-row tiles put a
    boundary at memory row 256 (sample 2, t = 68).  A poisoned dy[b, co, t] reaches dx[b, :, t - 2], [.., t], [.., t + 2] and no
    other sample or frame; the pad channels of those frames are the exception recorded in tests/nonfinite_cases.py."""
    from speech_decoding_amd import lib as L
    case = X.dgrad_case(0, "exact", dtype)
    s = case.shape
    assert tuple(s)[:6] == (40, 48, 3, 2, 70, 3) and not s.glu
    Cin_p, Cout_p = L.pad_channels(s.cin), L.pad_channels(s.cout)
    wt = ops.pack_conv_weight(case.w.float().to(DEV), Cout_p, Cin_p, dtype, mode=1)
    tilings = {"default": 0, "single tile": L.CONV_SINGLE_TILE, "tile pairs": L.CONV_PAIR_TILES, "flat tiles": L.CONV_FLAT_TILES}

    def run(o):
        dyb = rows(ops, o["dy"], dtype)
        out = {}
        for label, flags in tilings.items():
            dxb = ops.conv_gemm(dyb, wt, ops.new_rows(s.B, s.T, Cin_p, dtype, DEV), B=s.B, T=s.T, KS=s.KS, dil=s.dil, flags=flags)
            out.update(N.split_pad(label, unrows(ops, dxb, s.B, Cin_p, s.T), s.cin))
        return out

    def ref(o):
        r = torch.zeros(s.B, Cin_p, s.T, dtype=torch.float64)
        r[:, :s.cin] = X.dgrad_ref(o["dy"].double(), case.w, s.dil)
        return {k: v for label in tilings for k, v in N.split_pad(label, N.stored(r, dtype), s.cin).items()}

    pos = N.positions(s.B, s.T, s.cout, flat_edges=(128, 256))
    assert {(1, 25), (1, 26), (2, 67), (2, 68)} <= {(b, t) for b, t, _ in pos.values()}          # memory rows 127 | 128 and 255 | 256
    run_cases("conv_gemm (data gradient)", run, ref, dict(dy=case.dy.float()), sites_of("dy", pos, bct), dtype, typed=("dy",))


@pytest.mark.parametrize("dtype", DTYPES, ids=name)
def test_wgrad_gemm_and_its_reductions(ops, dtype):
    """(cin 64, cout 160, KS 3, dil 1, T 50, B 5, five per-sample segments): one segment, per-subject segments through perm /
    seg_start, flat rows; then reduce_slabs and reduce_unpack_wgrad.  A poisoned dy[b, co, t] reaches row co of the slab of b's
    segment (every tap, every input channel) and no other output channel or segment; a poisoned x[b, ci, t] column ci."""
    from speech_decoding_amd import lib as L
    cin, cout, KS, dil, T, B, nseg = 64, 160, 3, 1, 50, 5, 5
    Cin_p, Cout_p = L.pad_channels(cin), L.pad_channels(cout)
    o = dict(dy=X.ints((B, cout, T), 3, 4100).float(), x=X.ints((B, cin, T), 3, 4101).float())
    order = [3, 0, 4, 1, 2]                                        # segment j holds sample order[j]
    perm = torch.tensor(order, dtype=torch.int32, device=DEV)
    seg = torch.arange(nseg + 1, dtype=torch.int32, device=DEV)
    kw = dict(B=B, T=T, KS=KS, dil=dil)

    def unpack(slabs, n):
        return host(ops.unpack_conv_wgrad(slabs, n, cout, cin, KS, Cout_p, Cin_p))

    def run(o):
        dyb, xb = rows(ops, o["dy"], dtype), rows(ops, o["x"], dtype)
        out = {"one segment": unpack(ops.wgrad_gemm(dyb, xb, **kw), 1)}
        for flat in (False, True):
            slabs = ops.wgrad_gemm(dyb, xb, flat_rows=flat, perm=perm, seg_start=seg, nseg=nseg, **kw)
            tag = ", flat rows" if flat else ""
            out["per sample" + tag] = unpack(slabs, nseg)
            out["per sample, reduce_slabs" + tag] = unpack(ops.reduce_slabs(slabs)[None], 1)
            out["per sample, reduce_unpack_wgrad" + tag] = host(ops.reduce_unpack_wgrad(slabs, cout, cin, KS))
        out["one segment, flat rows"] = unpack(ops.wgrad_gemm(dyb, xb, flat_rows=True, **kw), 1)
        return out

    def ref(o):
        dy, x = o["dy"].double(), o["x"].double()
        sample_seg = [order.index(b) for b in range(B)]
        per = N.stored(X.wgrad_ref(dy, x, KS, dil, sample_seg, nseg), None)
        tot = N.stored(X.wgrad_ref(dy, x, KS, dil), None)
        out = {"one segment": tot, "one segment, flat rows": tot}
        for tag in ("", ", flat rows"):
            out.update({"per sample" + tag: per, "per sample, reduce_slabs" + tag: tot, "per sample, reduce_unpack_wgrad" + tag: tot[0]})
        return out

    pos = N.positions(B, T, cout, t_edges=(32,))                   # the contraction runs in chunks of 32 / 64 rows
    sites = sites_of("dy", pos, bct) + [("the saved input, last row of the last sample, channel C - 1", "x", (B - 1, cin - 1, T - 1)),
                                        ("the saved input, first row of the first sample, channel 0", "x", (0, 0, 0)),
                                        ("the saved input, last row of sample 0 (next to sample 1's pad rows)", "x", (0, 1, T - 1)),
                                        ("the saved input, first row of sample 1", "x", (1, 1, 0))]
    run_cases("wgrad_gemm", run, ref, o, sites, dtype, typed=("dy", "x"))


@pytest.mark.parametrize("dtype", DTYPES16, ids=name)
def test_wgrad_typed_output(ops, dtype):
    """out (N, K) = out_scale (acc_scale[j] G^T Y - rscale[j] sub) rounded once into 16-bit storage, (M 33, N 70, K 192): a
    poisoned G[i, j] reaches row j alone, a poisoned Y[i, k] column k, sub[j, k] one element, the fp32 scales their row — also
    with the finite fp32 value that overflows the storage type"""
    from speech_decoding_amd import lib as L
    c = X.typed_case(0, "exact", dtype)
    s = c.shape
    o = dict(G=c.G.float(), Y=c.Y.float(), sub=c.sub.float(), rscale=c.rscale.float(), acc_scale=c.acc_scale.float(),
             out_scale=torch.tensor([c.out_scale]))
    o["rscale"][o["rscale"] == 0] = 1.0                           # (0 * inf is a NaN either way; keep every row's sub term alive)

    def run(o):
        G = torch.zeros((s.M + 1, L.pad_channels(s.N)), dtype=dtype, device=DEV)
        G[:s.M, :s.N] = o["G"].to(dtype).to(DEV)
        out = torch.full((s.N, s.K), float("nan"), dtype=dtype, device=DEV)
        ops.matmul_tn_typed(G, o["Y"].to(dtype).to(DEV), out, o["sub"].to(dtype).to(DEV), o["rscale"].to(DEV), M_rows=s.M, N_valid=s.N,
                            K_cols=s.K, pitch=s.K, out_scale=o["out_scale"].to(DEV), acc_scale=o["acc_scale"].to(DEV))
        return {"out": host(out)}

    def ref(o):
        d = lambda k: o[k].double()
        r = d("out_scale") * (d("acc_scale")[:, None] * (d("G").t() @ d("Y")) - d("rscale")[:, None] * d("sub"))
        return {"out": N.stored(r, dtype)}

    inf3 = dict(N.POISONS)
    n = run_cases("wgrad_gemm (typed output)", run, ref, o,
                  [("first row, first column", "G", (0, 0)), ("last row, last real column", "G", (s.M - 1, s.N - 1)),
                   ("row 31, below the chunk boundary at 32", "G", (31, 1)), ("row 32, above the chunk boundary at 32", "G", (32, 1)),
                   ("the other operand, last row, last column", "Y", (s.M - 1, s.K - 1)), ("the subtracted operand", "sub", (s.N - 1, 0))],
                  dtype, typed=("G", "Y", "sub"), values=inf3)
    n += run_cases("wgrad_gemm (typed output)", run, ref, o, [("row 0", "rscale", (0,)), ("the last row", "acc_scale", (s.N - 1,)),
                                                             ("the scalar", "out_scale", (0,))], dtype, typed=("G", "Y", "sub"))
    assert n == 18 + 12


@pytest.mark.parametrize("out_dtype", DTYPES, ids=lambda d: "out_" + name(d))
@pytest.mark.parametrize("dtype", DTYPES, ids=name)
def test_input_grad_per_sample_matrices(ops, dtype, out_dtype):
    """the Kp = 96 case (nW 2, C 70 of 128, B 3, T 130: two 128-row tiles): a poisoned G[b, d, t] reaches dX[b, :, t] and no other
    sample or frame; fp32 operands also carry the finite value that overflows a 16-bit dX"""
    case = X.ig_case(1, "exact", out_dtype)
    s = case.shape
    assert s.Kp == 96 and s.nW > 1
    widx = torch.tensor(X.IG_WIDX[1], dtype=torch.int32, device=DEV)
    o = dict(G=case.G.float(), W=case.W.float())
    # every column of every matrix holds a non-zero weight in row 0 and row Kp - 1 (the poisoned rows), so that a finite
    # overflow value reaches every channel of its frame
    o["W"][:, 0][o["W"][:, 0] == 0] = 1.0
    o["W"][:, s.Kp - 1][o["W"][:, s.Kp - 1] == 0] = 1.0

    def run(o):
        got = ops.input_grad(rows(ops, o["G"], dtype), o["W"].to(dtype).to(DEV), widx, s.B, s.C, s.T, out_dtype)
        return {"dX": host(got)}

    def ref(o):
        idx = torch.tensor(X.IG_WIDX[1])
        return {"dX": N.stored(torch.einsum("bdc,bdt->bct", o["W"].double()[idx][:, :, :s.C], o["G"].double()), out_dtype)}

    pos = N.positions(s.B, s.T, s.Kp, t_edges=(128,))
    values = N.poisons(out_dtype) if dtype == F32 else dict(N.POISONS)
    run_cases("input_grad", run, ref, o, sites_of("G", pos, bct), dtype, typed=("G", "W"), values=values)


@pytest.mark.parametrize("out_dtype", DTYPES, ids=lambda d: "out_" + name(d))
def test_param_gemm(ops, out_dtype):
    """fp32 operands of any strides, the product rounded into the output's type: batched (7, 270, 300)^T-sliced @ (7, 270, 209)
    views.  A poisoned A[b, i, k] reaches row i of batch member b, a poisoned B[b, k, j] column j; the finite value that
    overflows a 16-bit output is stored as inf"""
    A, Bm = X.pgemm_operands("batched_both_sliced")
    o = dict(A=A.float(), B=Bm.float())
    o["B"][o["B"] == 0] = 1.0                                      # every product of a poisoned A element is non-zero
    o["A"][o["A"] == 0] = 1.0

    def run(o):
        Ad, Bd = o["A"].to(DEV)[:, :270].transpose(1, 2), o["B"].to(DEV)[:, :270, :209]
        return {"out": host(ops.param_gemm(Ad, Bd, out_dtype=out_dtype))}

    def ref(o):
        return {"out": N.stored(torch.matmul(o["A"].double()[:, :270].transpose(1, 2), o["B"].double()[:, :270, :209]), out_dtype)}

    sites = [("first batch member, first row, first k", "A", (0, 0, 0)), ("last batch member, last row, last k", "A", (6, 269, 269)),
             ("k 127 of row 128", "A", (3, 127, 128)), ("k 128 of row 127", "A", (3, 128, 127)),
             ("the other operand, first column", "B", (0, 0, 0)), ("the other operand, last column", "B", (6, 269, 208))]
    run_cases("param_gemm", run, ref, o, sites, F32, values=N.poisons(out_dtype))


# ---------------------------------------------------------------------------------------------------------------
# the loss's embedding gradient (csrc/loss_gemm.hip)
# ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES16, ids=name)
@pytest.mark.parametrize("Bm,F,T", [(6, 32, 40), (130, 64, 20)], ids=["B6", "B130"])
def test_clip_dz_with_out_scale(ops, Bm, F, T, dtype):
    """out[j] = out_scale (cscale[j] sum_i G[i][j] Y[i] - rscale[j] Z[j]) on the streaming kernel; B 130 crosses its 128-row tile.
    A poisoned G[i][j] reaches sample j alone, a poisoned Y[i] element its (t, f) in every sample, a poisoned Z[j] element itself."""
    from speech_decoding_amd import lib as L
    Bn = Bm
    t = X._typed_build(X.TypedShape(Bm, Bn, F * T), 7100 + Bm, 1, (0.5, 1.0))
    sh = lambda v, n: v.reshape(n, T, F).permute(0, 2, 1).contiguous().float()
    o = dict(G=t.G.float(), Y=sh(t.Y, Bm), Z=sh(t.sub, Bn), cscale=t.acc_scale.float(), rscale=t.rscale.float(), out_scale=torch.tensor([2.0]))
    o["rscale"][o["rscale"] == 0] = 1.0
    Fp = L.pad_channels(F)
    re = L.rows_tp(T) * Fp
    assert L.load().sda_clip_dz_supported(Bm, Bn, re, ops.dt_code(dtype))

    def run(o):
        G = torch.zeros((Bm + 1, L.pad_channels(Bn)), dtype=dtype, device=DEV)
        G[:Bm, :Bn] = o["G"].to(dtype).to(DEV)
        out = ops.new_rows_uninit(Bn, T, Fp, dtype, DEV)
        ops.clip_dz(G, rows(ops, o["Y"], dtype), rows(ops, o["Z"], dtype), out, o["rscale"].to(DEV), o["cscale"].to(DEV), Bm=Bm, Bn=Bn,
                    row_elems=re, out_scale=o["out_scale"].to(DEV))
        return {"dZ": host(ops.rows_view(out, Bn, F, T))}

    def ref(o):
        d = lambda k: o[k].double()
        acc = torch.einsum("ij,ift->jft", d("G"), d("Y"))
        r = d("out_scale") * (d("cscale")[:, None, None] * acc - d("rscale")[:, None, None] * d("Z"))
        return {"dZ": N.stored(r, dtype)}

    gsites = [("first row, first column", "G", (0, 0)), ("last row, last column", "G", (Bm - 1, Bn - 1))]
    if Bm > 128:
        gsites += [("row 127, column 128", "G", (127, 128)), ("row 128, column 127", "G", (128, 127))]
    pos = N.positions(Bm, T, F)
    run_cases("clip_dz", run, ref, o, gsites + sites_of("Y", pos, bct) + [("the brain embedding, last row, channel C - 1", "Z", (Bn - 1, F - 1, T - 1))],
              dtype, typed=("G", "Y", "Z"), values=dict(N.POISONS))
    run_cases("clip_dz", run, ref, o, [("row 0", "rscale", (0,)), ("the last row", "cscale", (Bn - 1,)), ("the scalar", "out_scale", (0,))],
              dtype, typed=("G", "Y", "Z"))


# ---------------------------------------------------------------------------------------------------------------
# the CLIP loss tail (csrc/sa_loss.hip): fp32 statistics that couple a row and a column, coefficient matrices in 16-bit storage.
# The restatements are the fp32 emulations of tests/sa_loss_cases.py: torch's amax and max propagate a NaN.
# ---------------------------------------------------------------------------------------------------------------
CLIP_B = [6, 130]                                                   # (B 6, F 32, T 40) and (B 130, F 64, T 20): one block, col0 = 0


def matrix_sites(key, Bm, Bn):
    out = [("first row, first column", key, (0, 0)), ("last row, last column", key, (Bm - 1, Bn - 1)), ("row 1, last column", key, (1, Bn - 1))]
    if Bm > 128:
        out += [("row 127, column 128", key, (127, 128)), ("row 128, column 127", key, (128, 127))]
    return out


def overflowing_norm(coef32, largest):
    """the squared norm of row / column 1 at which the fp32 coefficient [1][1] (coef32(norm): the restatement without the store) is
    +-1e5, the issue's fp16 overflow value; asserted: it is, and no other coefficient lies within a factor 2 of fp16's largest
    value, where the kernel's own rounding could decide between finite and inf"""
    first = largest * 1e-10
    norm = first * (float(coef32(first)[1, 1].abs()) / N.OVERFLOW[torch.float16]) ** 2
    g = coef32(norm).abs()
    assert abs(float(g[1, 1]) / 1e5 - 1.0) < 1e-3, float(g[1, 1])
    g[1, 1] = 0.0
    assert not bool(((g > 65504.0 / 2) & (g < 65504.0 * 2)).any()), float(g.max())
    return norm


def clip_operands(Bm):
    c = S.clip_case(Bm, Bm, 0, "trained")
    return {k: v for k, v in c.items() if k != "name"}


def dev(t):
    return t.to(DEV).contiguous()


@pytest.mark.parametrize("Bm", CLIP_B)
def test_clip_logits_stats(ops, Bm):
    """a poisoned S[i][j] reaches logit (i, j), row i's maximum, sum and log-sum-exp, column j's log-sum-exp and the positive's
    logit when i = j; a poisoned norm its row or column; the temperature everything"""
    c = clip_operands(Bm)
    names = ("logits", "row_max", "row_sum", "col_lse", "diag", "row_lse")

    def run(o):
        return dict(zip(names, map(host, ops.clip_logits_stats(dev(o["S"]), dev(o["ysq"]), dev(o["zsq"]), dev(o["temp"]), Bm, Bm, 0))))

    def ref(o):
        return dict(zip(names, S.emul_logits_stats(o)))

    sites = matrix_sites("S", Bm, Bm) + [("the speech norms, last row", "ysq", (Bm - 1,)), ("the brain norms, first column", "zsq", (0,)),
                                         ("the temperature", "temp", (0,))]
    run_cases("clip_logits_stats", run, ref, c, sites, F32)


@pytest.mark.parametrize("dtype", DTYPES, ids=name)
@pytest.mark.parametrize("Bm", CLIP_B)
def test_clip_grad(ops, Bm, dtype):
    """a poisoned logit (i, j) reaches G[i][j], rscale[j] and the temperature's gradient; a poisoned row_lse[i] row i of G and
    every rscale; a poisoned speech norm the range factor ymax, hence every G and cscale"""
    c = clip_operands(Bm)

    def run(o):
        ins = [dev(o[k]) for k in ("logits", "row_lse", "col_lse", "ysq", "zsq", "temp")]
        return dict(zip(("G", "rscale", "cscale", "scalars"), map(host, ops.clip_grad(*ins, o["inv_norm"], 0, dtype))))

    def ref(o):
        G, rscale, cscale, scal = S.emul_clip_grad(o, dtype)
        return {"G": G[:Bm + 1], "rscale": rscale, "cscale": cscale, "scalars": scal}

    sites = matrix_sites("logits", Bm, Bm) + [("row 1", "row_lse", (1,)), ("the last column", "col_lse", (Bm - 1,)),
                                              ("the speech norms, row 1", "ysq", (1,)), ("the brain norms, last column", "zsq", (Bm - 1,)),
                                              ("the temperature", "temp", (0,))]
    run_cases(f"clip_grad -> {name(dtype)}", run, ref, c, sites, F32)
    if dtype == torch.float16:
        # a finite value that overflows the store: row 1's norm so far below the largest that the positive's G[1][1] = D (ymax /
        # |Y_1|) is 1e5 in the fp32 registers: inf as stored, never 65504.  Nothing else of G comes near fp16's range, and
        # everything in fp32 (rscale, cscale, the scalars) stays finite.
        small = overflowing_norm(lambda v: S.emul_clip_grad(dict(c, ysq=N.poisoned(c["ysq"], (1,), v)), F32)[0][:Bm, :Bm], float(c["ysq"].max()))
        r = ref(dict(c, ysq=N.poisoned(c["ysq"], (1,), small)))
        assert int((~torch.isfinite(r["G"])).sum()) == 1 and bool(torch.isinf(r["G"][1, 1])) and all(bool(torch.isfinite(r[k]).all()) for k in r if k != "G")
        run_cases("clip_grad -> float16", run, ref, c, [("the speech norms, row 1", "ysq", (1,))], F32, values={"ymax^2 / 1e10": small})


@pytest.mark.parametrize("dtype", DTYPES, ids=name)
@pytest.mark.parametrize("Bm", CLIP_B)
def test_clip_grad_y_and_finish(ops, Bm, dtype):
    """the speech side: a poisoned logit (i, j) reaches Gy[j][i] and row i's partial of j's 64-column block; then the finisher,
    where a poisoned partial reaches its own row's rscale and nothing else"""
    c = clip_operands(Bm)

    def run(o):
        ins = [dev(o[k]) for k in ("logits", "row_lse", "col_lse", "zsq", "zsq_all")]
        return dict(zip(("Gy", "part"), map(host, ops.clip_grad_y(*ins, 0, dtype))))

    def ref(o):
        Gy, part = S.emul_clip_grad_y(o, dtype)
        return {"Gy": Gy[:Bm + 1], "part": part[:-1]}

    sites = matrix_sites("logits", Bm, Bm) + [("row 1", "row_lse", (1,)), ("the last column", "col_lse", (Bm - 1,)),
                                              ("the brain norms, column 1", "zsq", (1,)), ("every rank's brain norms, column 1", "zsq_all", (1,))]
    run_cases(f"clip_grad_y -> {name(dtype)}", run, ref, c, sites, F32)
    if dtype == torch.float16:
        # the same for Gy[j][i] = D (zmax / |Z_j|): column 1's norm 1e5 times below the largest
        small = overflowing_norm(lambda v: S.emul_clip_grad_y(dict(c, zsq=N.poisoned(c["zsq"], (1,), v)), F32)[0][:Bm, :Bm], float(c["zsq_all"].max()))
        r = ref(dict(c, zsq=N.poisoned(c["zsq"], (1,), small)))
        assert int((~torch.isfinite(r["Gy"])).sum()) == 1 and bool(torch.isinf(r["Gy"][1, 1])) and bool(torch.isfinite(r["part"]).all())
        run_cases("clip_grad_y -> float16", run, ref, c, [("the brain norms, column 1", "zsq", (1,))], F32, values={"zmax^2 / 1e10": small})

    part32, row0, nrows = S.finish_case(c)
    o = dict(c, part=part32)

    def run_f(o):
        r = ops.clip_grad_y_finish(dev(o["part"]), dev(o["ysq"]), dev(o["zsq_all"]), dev(o["temp"]), o["inv_norm"], row0, nrows)
        return dict(zip(("rscale_y", "cscale_y"), map(host, r)))

    def ref_f(o):
        return dict(zip(("rscale_y", "cscale_y"), S.emul_clip_grad_y_finish(o, o["part"], row0, nrows)))

    sites = [("first block, first asked row", "part", (0, row0)), ("last block, last row", "part", (part32.shape[0] - 1, Bm - 1)),
             ("the speech norms, last row", "ysq", (Bm - 1,)), ("every rank's brain norms, column 0", "zsq_all", (0,)), ("the temperature", "temp", (0,))]
    if dtype == F32:                                              # the finisher has no storage type of its own: once
        run_cases("clip_grad_y_finish", run_f, ref_f, o, sites, F32)


# ---------------------------------------------------------------------------------------------------------------
# SpatialAttention backward (D1 20, K2 36, C 70; a dropped sensor at channel 0): the soft-max backward couples a row
# ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mask_kind", ["none", "dropped"])
def test_sa_softmax_backward_and_weights_backward(ops, mask_kind):
    """a poisoned dWd[r][c] reaches all of da's row r through the row's dot product, hence dz[r], and no other row; so does a
    poisoned saved weight W[r][c]"""
    from speech_decoding_amd import lib
    case = S.sa_case(20, 36, 70, "o1", mask_kind)
    D1, K2, C = case["D1"], case["K2"], case["C"]
    Cq = S.pad64(C)
    o = dict(dWd=case["dWd"], W=S.sa_forward_ref(case, False)["W"].float())
    mask = None if case["mask"] is None else dev(case["mask"])
    cosT, sinT = dev(case["cos"].t()), dev(case["sin"].t())
    ptr = lambda t: None if t is None else t.data_ptr()

    def run(o):
        dWd, W = dev(S.dwd_padded(dict(case, dWd=o["dWd"]))), dev(o["W"])
        da = torch.full((D1 + 1, Cq), S.SENT, device=DEV)
        lib.check(lib.load().sda_sa_softmax_backward(ptr(dWd), dWd.shape[1], ptr(W), ptr(mask), ptr(da), Cq, D1, C, ops._st()), "sa_softmax_backward")
        dz = torch.view_as_real(ops.sa_weights_backward(dWd, W, mask, cosT, sinT, K2))
        return {"da": host(da), "dz": host(dz)}

    def ref(o):
        cs = dict(case, dWd=o["dWd"])
        return {"da": S.emul_sa_softmax_backward(cs, o["W"], Cq), "dz": S.emul_sa_backward(cs, o["W"])[:D1]}

    sites = [("first row, channel 0", "dWd", (0, 0)), ("last row, the last real channel", "dWd", (D1 - 1, C - 1)),
             ("row 7, below the workgroup boundary at 8", "dWd", (7, 1)), ("row 8, above the workgroup boundary at 8", "dWd", (8, C - 1)),
             ("the saved weights, row 8, channel 1", "W", (8, 1))]
    run_cases("sa_softmax_backward / sa_weights_backward", run, ref, o, sites, F32)


# ---------------------------------------------------------------------------------------------------------------
# the other two kernels of csrc/sa_loss.hip whose soft-max shift is a maximum: the SpatialAttention forward and the
# cross-rank merge of the loss's row statistics.  Neither moves a gradient, but a NaN they dropped would never get that far.
# ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES, ids=name)
def test_sa_weights_forward(ops, dtype):
    """(D1 20, K2 36, C 70, a dropped sensor): a poisoned z[r][m] reaches every score of row r, hence the whole row of W and of
    the packed operand, and no other row"""
    case = S.sa_case(20, 36, 70, "o1", "dropped")
    D1 = case["D1"]
    cos, sin, mask = dev(case["cos"]), dev(case["sin"]), dev(case["mask"])

    def run(o):
        W, Wp = ops.sa_weights_forward(torch.view_as_complex(dev(o["z"])), cos, sin, mask, case["D1p"], case["Cp"], dtype)
        return {"W": host(W), "Wp": host(Wp[0, 0])}

    def ref(o):
        W, Wp = S.emul_softmax_pack(S.emul_sa_scores(dict(case, z=o["z"])), case, dtype)
        return {"W": W[:D1], "Wp": Wp}

    sites = [("first row, first mode, real part", "z", (0, 0, 0)), ("last row, last mode, imaginary part", "z", (D1 - 1, 35, 1)),
             ("row 7, below the workgroup boundary at 8", "z", (7, 1, 0)), ("row 8, above the workgroup boundary at 8", "z", (8, 1, 1))]
    run_cases("sa_weights_forward", run, ref, dict(z=case["z"]), sites, F32)


def test_clip_merge_rows(ops):
    """[world 4][3][Bg 300] tables of (row max, row sum, positive's logit): a poisoned entry of one rank reaches its own row's
    log-sum-exp (or positive) and no other row"""
    allp = S.merge_cases()["random"]
    world, _, Bg = allp.shape

    def run(o):
        return dict(zip(("lse", "diag"), map(host, ops.clip_merge_rows(dev(o["all"])))))

    def ref(o):
        return dict(zip(("lse", "diag"), S.emul_merge(o["all"])))

    sites = [("rank 0's row maxima, first row", "all", (0, 0, 0)), ("the last rank's row maxima, last row", "all", (world - 1, 0, Bg - 1)),
             ("rank 1's row sums, row 255", "all", (1, 1, 255)), ("rank 2's row sums, row 256", "all", (2, 1, 256)),
             ("rank 1's positives, row 7", "all", (1, 2, 7))]
    run_cases("clip_merge_rows", run, ref, dict(all=allp), sites, F32)


# ---------------------------------------------------------------------------------------------------------------
# the data-gradient conv's epilogues: GELU backward (tile, flat and wide kernels), GLU backward, BatchNorm statistics
# ---------------------------------------------------------------------------------------------------------------
def dgrad_operands(B, c_dy, c_dx, KS, T, seed):
    """integer dy (B, c_dy, T) and forward weights (c_dy, c_dx, KS): the data gradient is exact in every summation order"""
    return X.ints((B, c_dy, T), 2, seed).float(), X.ints((c_dy, c_dx, KS), 2, seed + 1)


def split_sums(label, v, C, Cp):
    """[plane 0 | plane 1] per-channel sums of Cp channels each -> the real channels, and the pad channels as an output of their
    own (the exception of tests/nonfinite_cases.py covers exactly those)"""
    return N.split_pad(label, v.reshape(2, Cp), C)


def pad_to(r, Cp):
    out = torch.zeros(r.shape[0], Cp, r.shape[2], dtype=r.dtype)
    out[:, :r.shape[1]] = r
    return out


# (kernel, dy channels, dx channels, T, B): the tile kernel at conv1 (64, 160, T 40, B 7) as its data gradient; the flat kernel's
# 128-channel tiling and the wide kernel's 256-channel tiling at the smallest shapes of their own tests
GELU_BWD = [("tile", 160, 64, 40, 7), ("flat", 100, 128, 77, 2), ("wide", 64, 256, 50, 9)]


@pytest.mark.parametrize("kernel,c_dy,c_dx,T,B,dtype", [g + (d,) for g in GELU_BWD for d in DTYPES if not (g[0] == "wide" and d == F32)],
                         ids=lambda v: v if isinstance(v, str) else name(v) if isinstance(v, torch.dtype) else str(v))      # conv1_wide has no fp32 form
def test_conv1_data_gradient_with_gelu_backward_epilogue(ops, kernel, c_dy, c_dx, T, B, dtype):
    """du = round(dy W) GELU'(u) and the per-unit column sums of du (the bias gradient): a poisoned dy[b, :, t] reaches du[b, :, t]
    and every channel's sum, a poisoned pre-activation u[b, c, t] its own element and channel c's sum"""
    from speech_decoding_amd import lib as L
    flags = {"tile": 0, "flat": L.CONV_FLAT_TILES, "wide": L.CONV_WIDE_TILES}[kernel]
    Cy, Cx = L.pad_channels(c_dy), L.pad_channels(c_dx)
    dy, w = dgrad_operands(B, c_dy, c_dx, 1, T, 5100 + c_dx)
    g = torch.Generator().manual_seed(c_dx)
    o = dict(dy=dy, u=E.q(torch.randn(B, c_dx, T, generator=g), dtype))
    wt = ops.pack_conv_weight(w.float().to(DEV), Cy, Cx, dtype, mode=1)
    nst = ops.conv_stats_rows(B, T, 1, Cx, flags | L.EPI_GELU_BWD)

    def run(o):
        st = torch.full((nst, 2, Cx), float("nan"), device=DEV)
        du = ops.conv_gemm(rows(ops, o["dy"], dtype), wt, ops.new_rows(B, T, Cx, dtype, DEV), B=B, T=T, KS=1, dil=0, flags=flags,
                           gelu_bwd_u=rows(ops, o["u"], dtype), stats=st)
        return {"du": unrows(ops, du, B, Cx, T), "column sums": host(st[:, 0].double().sum(0)), "unused statistics plane": host(st[:, 1])}

    def ref(o):
        dg = N.stored(X.dgrad_ref(o["dy"].double(), w, 0), dtype).double()
        du = pad_to(dg * E.ggrad64(o["u"]), Cx)
        return {"du": N.stored(du, dtype), "column sums": du.sum(dim=(0, 2)), "unused statistics plane": torch.zeros(nst, Cx)}

    # conv1_flat works in 128-row units, conv1_wide on 256-row tiles; the tile kernel's 128-row tiles lie inside a sample (T 40)
    edge = {"tile": None, "flat": 128, "wide": 256}[kernel]
    pos = N.positions(B, T, c_dy, flat_edges=(edge,) if edge else ())
    if edge:
        sides = [k for k in pos if f"the boundary at {edge}" in k]
        assert len(sides) == 2 and edge < B * L.rows_tp(T), (kernel, sides)       # flat: memory rows 127 | 128 = sample 1, t 18 | 19
    sites = sites_of("dy", pos, bct)
    sites.append(("the saved pre-activation, last row of the last sample, channel C - 1", "u", (B - 1, c_dx - 1, T - 1)))
    # dx has no pad channels at these widths: no exception applies, every element of every output owes both checks
    assert Cx == c_dx and "conv_gemm (data gradient, GELU backward)" not in N.EXCEPTIONS
    run_cases("conv_gemm (data gradient, GELU backward)", run, ref, o, sites, dtype, typed=("dy", "u"))


@pytest.mark.parametrize("dtype", DTYPES, ids=name)
def test_conv3_data_gradient_with_glu_backward_epilogue(ops, dtype):
    """conv3 (cin 40, cout 48, dil 2, T 70, B 3) as the gradient entering an F.glu: [dy sig(g) | dy out (1 - sig(g))] and the
    column sums of both halves; the saved output is poisoned in the out half, the saved gate in the gate half"""
    from speech_decoding_amd import lib as L
    B, c_dy, H, KS, dil, T = 3, 48, 40, 3, 2, 70
    Cy, Hp = L.pad_channels(c_dy), L.pad_channels(H)
    dy, w = dgrad_operands(B, c_dy, H, KS, T, 5200)
    g = torch.Generator().manual_seed(52)
    o = dict(dy=dy, out=E.q(torch.randn(B, H, T, generator=g), dtype), gate=E.q(torch.randn(B, H, T, generator=g), dtype))
    wt = ops.pack_conv_weight(w.float().to(DEV), Cy, Hp, dtype, mode=1)
    nst = ops.conv_stats_rows(B, T, KS, Hp, 0)

    def split_halves(dx):
        """(B, 2 Hp, T) = [d value | d gate], each half H real + Hp - H pad channels -> the real channels of both, the pad of both"""
        v, g = N.split_pad("v", dx[:, :Hp], H), N.split_pad("g", dx[:, Hp:], H)
        return {"dx": torch.cat([v["v"], g["g"]], 1), "dx" + N.PAD: torch.cat([v["v" + N.PAD], g["g" + N.PAD]], 1)}

    def run(o):
        st = torch.full((nst, 2, Hp), float("nan"), device=DEV)
        got = ops.conv_gemm(rows(ops, o["dy"], dtype), wt, ops.new_rows(B, T, 2 * Hp, dtype, DEV), B=B, T=T, KS=KS, dil=dil, stats=st,
                            glu_bwd=(rows(ops, o["out"], dtype), rows(ops, o["gate"], dtype)))
        return dict(split_sums("column sums", host(ops.reduce_stats(st)), H, Hp), **split_halves(unrows(ops, got, B, 2 * Hp, T)))

    def ref(o):
        d = X.dgrad_ref(o["dy"].double(), w, dil).permute(0, 2, 1).reshape(B * T, H)
        rl = lambda v: v.permute(0, 2, 1).reshape(B * T, H)
        r = E.ref_glu_backward_og(rl(o["out"]), rl(o["gate"]), d, dtype)[0]
        both = torch.zeros(B * T, 2 * Hp, dtype=torch.float64)
        both[:, :H], both[:, Hp:Hp + H] = r[:, :H], r[:, H:]
        return dict(split_sums("column sums", N.stored(both.sum(0), None), H, Hp),
                    **split_halves(N.stored(both.reshape(B, T, 2 * Hp).permute(0, 2, 1), dtype)))

    sites = sites_of("dy", N.positions(B, T, c_dy), bct) + [("the saved output, first row, channel 0 (out half)", "out", (0, 0, 0)),
                                                           ("the saved gate, last row, channel H - 1 (gate half)", "gate", (B - 1, H - 1, T - 1))]
    run_cases("conv_gemm (data gradient)", run, ref, o, sites, dtype, typed=("dy", "out", "gate"))


@pytest.mark.parametrize("dtype", DTYPES, ids=name)
@pytest.mark.parametrize("store_dg", [False, True], ids=["dy", "dg"])
def test_conv3_data_gradient_with_bn_statistics_epilogue(ops, store_dg, dtype):
    """conv3 (cin 40, cout 48, dil 2, T 70, B 3) whose output is the gradient of a BatchNorm + GELU layer: the stored dy (or, with
    EPI_BN_STORE_DG, dg = dy GELU'(z)) and the per-tile statistics (sum dg, sum dg xhat) on the single-tile, tile-pair and flat
    kernels.  A poisoned gradient reaches every channel's statistics; a poisoned BatchNorm input h[b, c, t] channel c's alone."""
    from speech_decoding_amd import lib as L
    B, c_dy, c_dx, KS, dil, T = 3, 48, 40, 3, 2, 70
    Cy, Cx = L.pad_channels(c_dy), L.pad_channels(c_dx)
    dy, w = dgrad_operands(B, c_dy, c_dx, KS, T, 5300)
    g = torch.Generator().manual_seed(53)
    o = dict(dy=dy, h=E.q(torch.randn(B, c_dx, T, generator=g) * 1.3 + 0.2, dtype))
    gamma, beta = torch.rand(c_dx, generator=g) + 0.5, torch.rand(c_dx, generator=g) - 0.5
    mean = o["h"].double().mean(dim=(0, 2)).float()
    rstd = (1.0 / torch.sqrt(o["h"].double().var(dim=(0, 2), unbiased=False) + 1e-5)).float()
    coef = torch.zeros(4, Cx)
    coef[:, :c_dx] = torch.stack([gamma, beta, mean, rstd])
    wt = ops.pack_conv_weight(w.float().to(DEV), Cy, Cx, dtype, mode=1)
    tilings = {"single tile": L.CONV_SINGLE_TILE, "tile pairs": L.CONV_PAIR_TILES, "flat tiles": L.CONV_FLAT_TILES}

    def run(o):
        out = {}
        dyb, hb = rows(ops, o["dy"], dtype), rows(ops, o["h"], dtype)
        for label, flags in tilings.items():
            st = torch.full((ops.conv_stats_rows(B, T, KS, Cx, flags), 2, Cx), float("nan"), device=DEV)
            y = ops.conv_gemm(dyb, wt, ops.new_rows(B, T, Cx, dtype, DEV), B=B, T=T, KS=KS, dil=dil, stats=st, bn_x=hb, bn_coef=coef.to(DEV),
                              flags=flags | (L.EPI_BN_STORE_DG if store_dg else 0))
            out.update(N.split_pad(label, unrows(ops, y, B, Cx, T), c_dx))
            out.update(split_sums(label + " statistics", host(ops.reduce_stats(st)), c_dx, Cx))
        return out

    def ref(o):
        d = X.dgrad_ref(o["dy"].double(), w, dil)
        c = lambda v: v.double()[None, :, None]
        xhat = (o["h"].double() - c(mean)) * c(rstd)
        dg = d * E.ggrad64(c(gamma) * xhat + c(beta))
        y = N.stored(pad_to(dg if store_dg else d, Cx), dtype)
        st = N.stored(torch.cat([pad_to(dg, Cx).sum(dim=(0, 2)), pad_to(dg * xhat, Cx).sum(dim=(0, 2))]), None)
        return {k: v for label in tilings for k, v in dict(split_sums(label + " statistics", st, c_dx, Cx), **N.split_pad(label, y, c_dx)).items()}

    sites = sites_of("dy", N.positions(B, T, c_dy, flat_edges=(128, 256)), bct)
    sites.append(("the saved BatchNorm input, last row of the last sample, channel C - 1", "h", (B - 1, c_dx - 1, T - 1)))
    run_cases("conv_gemm (data gradient)", run, ref, o, sites, dtype, typed=("dy", "h"))


# ---------------------------------------------------------------------------------------------------------------
# whole-model containment: one bad sample must not reach another sample's result
# ---------------------------------------------------------------------------------------------------------------
TOY = dict(TB.TOY, B=6)          # the toy shape of tests/test_dp_gpu.py, six samples


@pytest.mark.parametrize("dtype", ["bf16", "fp16"])
def test_eval_mode_encoder_keeps_an_inf_inside_its_sample(dtype):
    """eval-mode BrainEncoder (BatchNorm on its running statistics: nothing couples the samples), forward and dX: sample 2's input
    holds one inf; every other sample's Z and dX carry the bits of the clean run, and sample 2's own are non-finite"""
    d = TOY
    loc, P, X, _, subj = TB.toy_problem(d, d["B"])
    enc = TB.build_encoder(P, TB.encoder_args(d, loc, dtype), DEV, training=False)
    dZ = torch.randn(d["B"], d["F"], d["T"], generator=torch.Generator().manual_seed(11))
    bad = 2

    def run(Xin):
        Xl = Xin.to(DEV).requires_grad_(True)
        Z = enc(Xl, subj)
        Z.backward(dZ.to(DEV).to(Z.dtype))
        return host(Z.detach().clone()), host(Xl.grad)

    Z0, dX0 = run(X)
    assert bool(torch.isfinite(Z0).all()) and bool(torch.isfinite(dX0).all())
    for where, idx in (("first frame, channel 0", (bad, 0, 0)), ("last frame, last channel", (bad, d["C"] - 1, d["T"] - 1))):
        Z1, dX1 = run(N.poisoned(X, idx, N.INF))
        others = [b for b in range(d["B"]) if b != bad]
        for what, got, clean in (("Z", Z1, Z0), ("dX", dX1, dX0)):
            assert not bool(torch.isfinite(got[bad]).all()), (dtype, where, what, "the inf vanished from its own sample")
            ref = clean.clone().float()
            ref[bad] = N.NAN                                                   # the sample's own results: whatever non-finite the maths gives
            res = N.check(ref[others], got[others], clean[others], ref[others])
            assert not res, (dtype, where, what, res)


@pytest.mark.parametrize("dtype", ["fp32", "bf16", "fp16"])
def test_retrieve_keeps_a_non_finite_query_inside_its_row(dtype):
    """retrieve() with one non-finite query row (an inf, then a NaN): every other query's scores, indices and ranks carry the bits
    of the clean run.  (A non-finite candidate row is out of scope.)"""
    from speech_decoding_amd import SpeechBank, retrieve
    Nq, M, F, T = 40, 300, 24, 50
    dt = {"fp32": torch.float32, "bf16": torch.bfloat16, "fp16": torch.float16}[dtype]
    g = torch.Generator().manual_seed(1234 + 17 * Nq + M)
    bank = torch.randn(M, F, T, generator=g)
    labels = torch.randint(M, (Nq,), generator=g)
    queries = 0.35 * bank[labels] + torch.randn(Nq, F, T, generator=g)
    b = SpeechBank.from_tensor(bank.to(DEV), dtype=dt)
    clean = retrieve(queries.to(DEV), b, k=10, labels=labels.to(DEV))
    for bad, v in ((0, N.INF), (Nq - 1, N.NAN), (17, -N.INF)):
        got = retrieve(N.poisoned(queries, (bad, F - 1, T - 1), v).to(DEV), b, k=10, labels=labels.to(DEV))
        others = torch.tensor([i for i in range(Nq) if i != bad])
        for what in ("scores", "indices", "ranks"):
            a, c = host(getattr(got, what))[others], host(getattr(clean, what))[others]
            assert torch.equal(N._bits(a), N._bits(c)), (dtype, bad, v, what)
        assert not bool(torch.isfinite(host(got.scores)[bad]).any()), (dtype, bad, v, "the bad query's own scores are finite")
