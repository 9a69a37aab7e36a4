"""The standalone submodules `SpatialAttention`, `SubjectBlock` and `ConvBlock` on the MI355X: the reference's own activations,
running statistics and gradients (tests/golden/e2e_small.npz) from standalone calls, every compute dtype x input dtype in train
and eval mode against float64 autograd of the oracle's stage functions on the same rounded operands, RNG and BatchNorm modes,
isolation from the encoder's engine, and the row-layout hand-off between chained calls (ops.pack_rows / unpack_rows / rows_of included)."""
import numpy as np
import pytest
import torch
import torch.nn.functional as TF

pytestmark = pytest.mark.gpu

from oracle import brain_oracle as O                                      # noqa: E402
from tests import builders as TB                                           # noqa: E402
from tests import golden_io as G                                           # noqa: E402
from tests.parity import operands_as_device_sees_them, rel_l2, round_to   # noqa: E402

DEV = "cuda:0"
DT = {"fp32": torch.float32, "bf16": torch.bfloat16, "fp16": torch.float16}
OUT_REL = {"fp32": 1e-4, "bf16": 4e-2, "fp16": 5e-3}           # activations (storage rounding between kernels)
GRAD_REL = {"fp32": 1e-4, "bf16": 6e-2, "fp16": 8e-3}          # every gradient
X_OUT_REL = {"fp32": 0.0, "bf16": 6e-3, "fp16": 1e-3}          # + the rounding of dX to X's own dtype
TOY = dict(TB.TOY, B=6)
SHAPES = {"toy": TOY, "toy_c64": dict(TOY, C=64),
          "208": dict(C=208, S=27, D1=270, D2=320, K=32, T=96, B=4), "60": dict(C=60, S=1, D1=270, D2=320, K=32, T=96, B=4)}
KINDS = ["sa", "sb", "cb0", "cb1", "cb2", "cb3", "cb4"]
PREFIX = {"sa": "subject_block.spatial_attention.", "sb": "subject_block.", **{f"cb{k}": f"conv_blocks.conv{k}." for k in range(5)}}


def make_args(d, loc, dtype="fp32", F=8):
    return TB.encoder_args(d, loc, dtype, F=F, reduction="mean", init_temperature=5.1)


def positions_and_params(d, F=8):
    loc = O.synthetic_positions(d["C"], seed=1)
    return loc, O.seeded_params(d["C"], d["S"], d["D1"], d["D2"], F, d["K"], seed=2, loc=loc)


def sub_state(P, prefix):
    return {k[len(prefix):]: v for k, v in P.items() if k.startswith(prefix)}


def build(kind, d, loc, P, dtype="fp32", training=True):
    from speech_decoding.models import ConvBlock, SpatialAttention, SubjectBlock
    if kind == "sa":
        m = SpatialAttention(make_args(d, loc, dtype))
    elif kind == "sb":
        m = SubjectBlock(make_args(d, loc, dtype))
    else:
        m = ConvBlock(int(kind[2:]), d["D1"], d["D2"]).set_compute_dtype(DT[dtype])
    missing, unexpected = m.load_state_dict(sub_state(P, PREFIX[kind]), strict=True)
    assert not missing and not unexpected
    return m.to(DEV).train(training)


def channels(kind, d):
    """(input channels, output channels) of a module."""
    if kind in ("sa", "sb"):
        return d["C"], d["D1"]
    return (d["D1"] if kind == "cb0" else d["D2"]), d["D2"]


def call(m, kind, X, subj):
    return m(X, subj) if kind == "sb" else m(X)


def pin_centre(m, kind, centre):
    if kind in ("sa", "sb"):
        (m if kind == "sa" else m.spatial_attention).set_drop_centre(centre)


def param_grads(m, kind):
    """{state key of the reference: gradient} with the per-subject weight split like the reference's ModuleList."""
    out = {}
    for n, p in m.named_parameters():
        if n == "subject_layer.weight":
            for s in range(p.shape[0]):
                out[f"{PREFIX[kind]}subject_layer.{s}.weight"] = None if p.grad is None else p.grad[s]
        else:
            out[PREFIX[kind] + n] = p.grad
    return out


def null_grad(key, training):
    return training and key.startswith("conv_blocks.") and key.endswith((".conv0.bias", ".conv1.bias"))


def to64(P):
    return {k: (v.to(torch.complex128) if v.is_complex() else v.double()) if (v.is_floating_point() or v.is_complex()) else v.clone()
            for k, v in P.items()}


def oracle(kind, Q, X, subj, mask, training, stats):
    if kind == "sa":
        return O.spatial_attention(Q, X, mask)
    if kind == "sb":
        return O.subject_block(Q, X, subj, mask)
    return O.conv_block(Q, X, int(kind[2:]), training, stats)


# ------------------------------------------------------------------------------------------------------------------------------
# 1-2. the reference's numbers (e2e_small.npz: forward hooks of step 0, running statistics after it, every gradient)
# ------------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def small():
    return G.load("e2e_small.npz")


def small_setup(small):
    C, S, D1, D2, F, K, T, B = (int(v) for v in small["dims"])
    d = dict(C=C, S=S, D1=D1, D2=D2, K=K, T=T, B=B)
    P = G.state_from(small, "init/")
    temp = P.pop("temp")
    X = torch.from_numpy(small["X"]).to(DEV)
    subj = torch.from_numpy(small["subject_idxs"])
    return d, P, temp, X, subj


def close(got, ref, rtol=1e-4, atol=1e-5):
    np.testing.assert_allclose(got.detach().float().cpu().numpy(), ref, rtol=rtol, atol=atol)


def test_reference_activations_and_running_statistics(small):
    d, P, _, X, subj = small_setup(small)
    loc = small["loc"]
    np.random.seed(100)                                        # make_golden.py: step 0 draws its centre after seed(100)
    assert int(np.random.randint(d["C"])) == int(small["drop_centres"][0])
    sa = build("sa", d, loc, P)
    np.random.seed(100)
    close(sa(X), small["act/spatial_attention"])
    sb = build("sb", d, loc, P)
    np.random.seed(100)
    out = sb(X, subj)
    assert out.shape == (d["B"], d["D1"], d["T"]) and out.dtype == torch.float32
    close(out, small["act/subject_block"])
    for k in range(5):
        cb = build(f"cb{k}", d, loc, P)
        src = small["act/subject_block"] if k == 0 else small[f"act/conv_block{k - 1}"]
        close(cb(torch.from_numpy(src).to(DEV)), small[f"act/conv_block{k}"])
        for j, bn in ((0, cb.batchnorm0), (1, cb.batchnorm1)):
            key = f"after1fwd/conv_blocks.conv{k}.batchnorm{j}."
            close(bn.running_mean, small[key + "running_mean"])
            close(bn.running_var, small[key + "running_var"])
            assert int(bn.num_batches_tracked) == int(small[key + "num_batches_tracked"]) == 1


def test_reference_gradients_from_standalone_calls(small):
    """The reference's step 0 rebuilt from the submodules: SubjectBlock, the five ConvBlocks through enc.conv_blocks, the final
    projections with GELU (torch, here in the test only), this package's CLIPLoss."""
    from speech_decoding.utils.loss import CLIPLoss
    d, P, temp, X, subj = small_setup(small)
    args = make_args(d, small["loc"], F=int(small["dims"][4]))
    enc = TB.build_encoder(P, args, DEV)
    lossf = CLIPLoss(args)
    with torch.no_grad():
        lossf.temp.copy_(temp.reshape(1))
    lossf = lossf.to(DEV)
    np.random.seed(100)
    h = enc.conv_blocks(enc.subject_block(X, subj))
    h = TF.gelu(TF.conv1d(h, enc.conv_final1.weight, enc.conv_final1.bias))
    Z = TF.gelu(TF.conv1d(h, enc.conv_final2.weight, enc.conv_final2.bias))
    loss = lossf(torch.from_numpy(small["Y"]).to(DEV), Z)
    assert abs(float(loss.detach()) - float(small["step0/loss"])) < 1e-4
    loss.backward()
    errs = {}
    for n, p in list(enc.named_parameters()):
        if n == "subject_block.subject_layer.weight":
            items = [(f"subject_block.subject_layer.{s}.weight", p.grad[s]) for s in range(p.shape[0])]
        else:
            items = [(n, p.grad)]
        for k, g in items:
            assert g is not None and g.shape == p.shape[-g.dim():] and g.dtype == p.dtype, k
            if k.endswith(".z"):
                errs[k + "@re"] = rel_l2(g.real, torch.from_numpy(small[f"grad/{k}@re"]))
                errs[k + "@im"] = rel_l2(g.imag, torch.from_numpy(small[f"grad/{k}@im"]))
            elif null_grad(k, True):         # exactly zero in exact arithmetic; the reference reports rounding noise
                assert float(g.abs().max()) == 0.0 and np.abs(small[f"grad/{k}"]).max() < 1e-4, k
            else:
                errs[k] = rel_l2(g, torch.from_numpy(small[f"grad/{k}"]))
    errs["temp"] = rel_l2(lossf.temp.grad, torch.from_numpy(small["grad/temp"]))
    bad = {k: v for k, v in errs.items() if not v <= 1e-4}
    assert not bad, bad
    assert len(errs) >= 2 + 2 + 3 + 5 * 8 + 4 + 1


# ------------------------------------------------------------------------------------------------------------------------------
# 3. against float64 autograd of the oracle's stages, on the operands the device sees
# ------------------------------------------------------------------------------------------------------------------------------
CASES = ([("toy", k, dt, xdt, mode) for k in KINDS for dt in DT for xdt in DT for mode in ("train", "eval")]
         + [("toy_c64", k, dt, "fp32", mode) for k in ("sa", "sb") for dt in DT for mode in ("train", "eval")]
         + [(tag, k, dt, "fp32", "train") for tag in ("208", "60") for k in ("sa", "sb", "cb0", "cb1") for dt in DT]
         + [(tag, k, "fp32", "fp32", "eval") for tag in ("208", "60") for k in ("sb", "cb2", "cb4")])


@pytest.mark.parametrize("shape,kind,dtype,xdt,mode", CASES)
def test_against_float64_oracle(shape, kind, dtype, xdt, mode):
    d = SHAPES[shape]
    training = mode == "train"
    loc, P = positions_and_params(d)
    m = build(kind, d, loc, P, dtype, training)
    cin, cout = channels(kind, d)
    g = torch.Generator().manual_seed(5)
    X = torch.randn(d["B"], cin, d["T"], generator=g)
    subj = torch.randint(0, d["S"], (d["B"],), generator=g)
    R = torch.randn(d["B"], cout, d["T"], generator=g)
    centre = 3
    pin_centre(m, kind, centre)
    Xl = X.to(DEV).to(DT[xdt]).requires_grad_(True)
    out = call(m, kind, Xl, subj)
    assert out.shape == (d["B"], cout, d["T"]) and out.dtype == DT[dtype]
    (out.float() * R.to(DEV)).sum().backward()

    Q = to64(operands_as_device_sees_them(P, dtype))
    keys = [k for k in param_grads(m, kind)]
    for k in keys:
        Q[k].requires_grad_(True)
    stats = {k: v.clone() for k, v in Q.items() if "running" in k or "num_batches" in k}
    Xd = round_to(round_to(X, xdt), dtype).double().requires_grad_(True)
    mask = O.dropout_mask(loc.double(), centre, 0.1) if training and kind in ("sa", "sb") else None
    ref = oracle(kind, Q, Xd, subj, mask, training, stats)
    grads = torch.autograd.grad((ref * round_to(R, dtype).double()).sum(), [Xd] + [Q[k] for k in keys], allow_unused=True)
    # (a subject absent from the batch takes no part in the oracle's graph: its gradient is zero)
    grads = grads[:1] + tuple(torch.zeros_like(Q[k]) if gk is None else gk for k, gk in zip(keys, grads[1:]))

    assert rel_l2(out.detach().float(), ref.detach()) <= OUT_REL[dtype], rel_l2(out.detach().float(), ref.detach())
    assert Xl.grad is not None and Xl.grad.dtype == DT[xdt] and Xl.grad.shape == X.shape and Xl.grad.is_contiguous()
    err = rel_l2(Xl.grad, grads[0])
    assert err <= GRAD_REL[dtype] + X_OUT_REL[xdt], ("X", err)
    for (n, p) in m.named_parameters():
        assert p.grad is not None and p.grad.shape == p.shape and p.grad.dtype == p.dtype and p.grad.is_contiguous(), n
    for k, gk, want in zip(keys, [param_grads(m, kind)[k] for k in keys], grads[1:]):
        if null_grad(k, training):
            assert float(gk.abs().max()) == 0.0 and float(want.abs().max()) < 1e-9, k
            continue
        err = rel_l2(gk, want)
        assert err <= GRAD_REL[dtype], (k, err)
    if kind.startswith("cb"):
        for j, bn in ((0, m.batchnorm0), (1, m.batchnorm1)):
            key = f"{PREFIX[kind]}batchnorm{j}."
            if training:
                assert rel_l2(bn.running_mean, stats[key + "running_mean"]) <= OUT_REL[dtype]
                assert rel_l2(bn.running_var, stats[key + "running_var"]) <= OUT_REL[dtype]
                assert int(bn.num_batches_tracked) == 1
            else:
                assert torch.equal(bn.running_mean.cpu(), P[key + "running_mean"]) and int(bn.num_batches_tracked) == 0


@pytest.mark.parametrize("kind", ["sb", "cb0", "cb3"])
def test_frozen_parameters_and_inputs_without_gradient(kind, monkeypatch):
    from speech_decoding_amd import ops
    d = TOY
    loc, P = positions_and_params(d)
    cin, cout = channels(kind, d)
    X = torch.randn(d["B"], cin, d["T"]).to(DEV)
    subj = torch.tensor([0, 1, 2, 0, 1, 2])
    calls = {"wgrad": 0, "input_grad": 0}
    real_w, real_i = ops.wgrad_gemm, ops.input_grad
    monkeypatch.setattr(ops, "wgrad_gemm", lambda *a, **k: (calls.__setitem__("wgrad", calls["wgrad"] + 1), real_w(*a, **k))[1])
    monkeypatch.setattr(ops, "input_grad", lambda *a, **k: (calls.__setitem__("input_grad", calls["input_grad"] + 1),
                                                            real_i(*a, **k))[1])
    # every parameter frozen: the input gradient alone, no weight gradient launched
    m = build(kind, d, loc, P, "bf16")
    for p in m.parameters():
        p.requires_grad_(False)
    Xl = X.clone().requires_grad_(True)
    call(m, kind, Xl, subj).float().sum().backward()
    assert Xl.grad is not None and Xl.grad.shape == X.shape and Xl.grad.dtype == X.dtype and bool(torch.isfinite(Xl.grad).all())
    assert all(p.grad is None for p in m.parameters()) and calls["wgrad"] == 0
    # an input that needs no gradient: the parameters' gradients, no input gradient
    m = build(kind, d, loc, P, "bf16")
    calls.update(wgrad=0, input_grad=0)
    Xn = X.clone()
    call(m, kind, Xn, subj).float().sum().backward()
    assert Xn.grad is None and calls["input_grad"] == 0 and calls["wgrad"] > 0
    assert all(p.grad is not None for p in m.parameters())
    # no_grad: nothing is kept for a backward
    with torch.no_grad():
        out = call(m, kind, X.clone().requires_grad_(True), subj)
    assert out.grad_fn is None


# ------------------------------------------------------------------------------------------------------------------------------
# 4. modes
# ------------------------------------------------------------------------------------------------------------------------------
def rng_equal(a, b):
    return a[0] == b[0] and np.array_equal(a[1], b[1]) and a[2:] == b[2:]


def test_eval_draws_nothing_and_train_draws_once_per_call():
    d = TOY
    loc, P = positions_and_params(d)
    X = torch.randn(d["B"], d["C"], d["T"]).to(DEV)
    subj = torch.tensor([0, 1, 2, 0, 1, 2])
    np.random.seed(7)
    for kind in ("sa", "sb"):
        m = build(kind, d, loc, P, training=False)
        before = np.random.get_state()
        with torch.no_grad():
            call(m, kind, X, subj)
        assert rng_equal(before, np.random.get_state())
        m.train()
        for _ in range(2):
            before = np.random.get_state()
            out = call(m, kind, X, subj)
            after = np.random.get_state()
            np.random.set_state(before)
            c = int(np.random.randint(d["C"]))
            assert rng_equal(after, np.random.get_state())
            pin_centre(m, kind, c)                          # the same call with that centre pinned: same bits, no draw
            before = np.random.get_state()
            assert torch.equal(call(m, kind, X, subj), out)
            assert rng_equal(before, np.random.get_state())
            pin_centre(m, kind, None)
    cb = build("cb1", d, loc, P, training=False)
    saved = {k: v.clone() for k, v in cb.state_dict().items()}
    h = torch.randn(d["B"], d["D2"], d["T"]).to(DEV)
    out = cb(h)
    out.float().sum().backward()
    assert all(torch.equal(v, saved[k]) for k, v in cb.state_dict().items())
    cb.train()
    cb(h)
    assert int(cb.batchnorm0.num_batches_tracked) == 1 and not torch.equal(cb.batchnorm1.running_mean, saved["batchnorm1.running_mean"])


def test_absent_subject_gets_a_zero_gradient_slice():
    d = TOY
    loc, P = positions_and_params(d)
    for dtype in ("fp32", "bf16"):
        sb = build("sb", d, loc, P, dtype)
        sb.spatial_attention.set_drop_centre(2)
        sb(torch.randn(d["B"], d["C"], d["T"]).to(DEV), torch.tensor([0, 2, 0, 2, 2, 0])).float().square().sum().backward()
        gw = sb.subject_layer.weight.grad
        assert gw.shape == sb.subject_layer.weight.shape
        assert float(gw[1].abs().max()) == 0.0 and float(gw[0].abs().max()) > 0 and float(gw[2].abs().max()) > 0


def test_bad_subject_indices():
    d = TOY
    loc, P = positions_and_params(d)
    sb = build("sb", d, loc, P)
    X = torch.randn(d["B"], d["C"], d["T"]).to(DEV)
    with pytest.raises(IndexError):
        sb(X, torch.tensor([0, 1, 2, 3, 0, 1]))
    with pytest.raises(ValueError):
        sb(X, torch.tensor([0, 1]))


# ------------------------------------------------------------------------------------------------------------------------------
# 5. isolation from the encoder's engine
# ------------------------------------------------------------------------------------------------------------------------------
def build_encoder(P, d, loc, F=16):
    return TB.build_encoder(P, make_args(d, loc, F=F), DEV)


@pytest.mark.parametrize("C", [20, 64])
def test_pending_encoder_backward_is_unaffected(C):
    d = dict(TOY, C=C)
    loc, P = positions_and_params(d, F=16)
    g = torch.Generator().manual_seed(9)
    X = torch.randn(d["B"], d["C"], d["T"], generator=g)
    R = torch.randn(d["B"], 16, d["T"], generator=g)
    subj = torch.tensor([0, 1, 2, 0, 1, 2])

    def run(interleave):
        enc = build_encoder(P, d, loc)
        enc.set_drop_centre(4)
        Xl = X.to(DEV).requires_grad_(True)
        Z = enc(Xl, subj)
        if interleave:
            e = enc.engine
            state = (e._gen, sorted(map(str, e._ws)), sorted(map(str, e._const)), getattr(e, "_plan_key", None))
            X2 = torch.randn(d["B"], d["C"], d["T"]).to(DEV).requires_grad_(True)
            h = enc.conv_blocks(enc.subject_block(X2, subj))
            params = list(enc.subject_block.parameters()) + list(enc.conv_blocks.parameters())
            torch.autograd.grad((h * torch.randn_like(h)).sum(), [X2] + params)      # no .grad accumulation
            with torch.no_grad():
                enc.subject_block.eval()(X2, subj)
            enc.subject_block.train()
            assert state == (e._gen, sorted(map(str, e._ws)), sorted(map(str, e._const)), getattr(e, "_plan_key", None))
        (Z * R.to(DEV)).sum().backward()
        return Z.detach().clone(), Xl.grad.clone(), {n: p.grad.clone() for n, p in enc.named_parameters()}

    Za, dXa, ga = run(False)
    Zb, dXb, gb = run(True)
    assert torch.equal(Za, Zb) and torch.equal(dXa, dXb)
    for n in ga:
        assert torch.equal(ga[n], gb[n]), n


def test_outputs_of_earlier_calls_stay_valid():
    d = TOY
    loc, P = positions_and_params(d)
    sb, cb = build("sb", d, loc, P, "bf16"), build("cb0", d, loc, P, "bf16")
    subj = torch.tensor([0, 1, 2, 0, 1, 2])
    X1 = torch.randn(d["B"], d["C"], d["T"]).to(DEV)
    h1 = sb(X1, subj)
    y1 = cb(h1)
    keep = (h1.detach().clone(), y1.detach().clone())
    for _ in range(2):
        X2 = torch.randn(d["B"], d["C"], d["T"]).to(DEV).requires_grad_(True)
        cb(sb(X2, subj)).float().sum().backward()
    assert torch.equal(h1.detach(), keep[0]) and torch.equal(y1.detach(), keep[1])


# ------------------------------------------------------------------------------------------------------------------------------
# 6. layout
# ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", ["fp32", "bf16"])
def test_chained_calls_hand_over_row_layout_views(dtype, monkeypatch):
    from speech_decoding_amd import ops
    d = TOY
    loc, P = positions_and_params(d, F=16)
    enc = build_encoder(P, d, loc)
    enc.set_compute_dtype(DT[dtype])
    subj = torch.tensor([0, 1, 2, 0, 1, 2])
    X = torch.randn(d["B"], d["C"], d["T"]).to(DEV)
    enc.subject_block.spatial_attention.set_drop_centre(1)
    h = enc.subject_block(X, subj)
    loop = h
    for blk in enc.conv_blocks:
        loop = blk(loop)
    assert torch.equal(enc.conv_blocks(h), loop)

    packs = []                                                 # dtype of the source each pack was handed
    real_pack = ops.pack_rows
    monkeypatch.setattr(ops, "pack_rows", lambda src, *a, **k: (packs.append(src.dtype), real_pack(src, *a, **k))[1])
    Xl = X.clone().requires_grad_(True)
    y = enc.conv_blocks(enc.subject_block(Xl, subj))
    assert packs == [Xl.dtype]                                 # X only, as it came (no widened copy): every stage hands an RL view on
    R = torch.randn(y.shape, device=DEV, dtype=y.dtype)
    (y * R).sum().backward()
    assert packs == [Xl.dtype, y.dtype]                        # + the plain incoming gradient of the last block, in its own dtype
    assert Xl.grad is not None and Xl.grad.is_contiguous()


@pytest.mark.parametrize("T", [40, 70])
@pytest.mark.parametrize("dst", ["fp32", "bf16", "fp16"])
def test_pack_rows_typed_bits_and_contract(T, dst):
    """16-bit inputs give the bits of the fp32 pack of the same values (T = 40: the 16-byte kernel, T = 70: the per-element one);
    valid rows get zero channel padding and the pad rows are left as they were."""
    from speech_decoding_amd import lib as L
    from speech_decoding_amd import ops
    B, C = 3, 70
    Cp = L.pad_channels(C)
    X = torch.randn(B, C, T, device=DEV) * 3
    for src in ("fp32", "bf16", "fp16"):
        Xs = X.to(DT[src])
        want = ops.new_rows(B, T, Cp, DT[dst], DEV)
        ops.pack_rows(Xs.float(), want)
        got = torch.full((L.rows_alloc(B, T), Cp), float("nan"), dtype=DT[dst], device=DEV)
        ops.pack_rows(Xs, got)
        valid = torch.zeros(L.rows_alloc(B, T), dtype=torch.bool)
        for b in range(B):
            valid[b * L.rows_tp(T) + L.ROW_PAD: b * L.rows_tp(T) + L.ROW_PAD + T] = True
        valid = valid.to(DEV)
        assert torch.equal(got[valid], want[valid]), (src, dst)
        assert bool(torch.isnan(got[~valid]).all())                         # pad rows and slack untouched
        assert float(got[valid][:, C:].abs().max()) == 0.0
        assert torch.equal(ops.rows_view(got, B, C, T).float(), Xs.float().to(DT[dst]).float())


def packed_randn(B, C, T, dtype):
    from speech_decoding_amd import lib as L
    from speech_decoding_amd import ops
    return ops.pack_rows(torch.randn(B, C, T, device=DEV) * 3, ops.new_rows(B, T, L.pad_channels(C), dtype, DEV))


@pytest.mark.parametrize("T", [40, 70])
def test_unpack_rows_dtypes(T):
    """Every (buffer dtype, output dtype) pair: the unpack into `dt` is the fp32 unpack rounded once to `dt`, bit for bit, as a
    contiguous (B, C, T) tensor.  C = 70: the second channel tile is mostly padding; T = 70: a partial time tile."""
    from speech_decoding_amd import ops
    B, C = 3, 70
    for src in DT.values():
        buf = packed_randn(B, C, T, src)
        ref = ops.unpack_rows(buf, B, C, T)
        assert ref.dtype == torch.float32 and torch.equal(ref, ops.rows_view(buf, B, C, T).float())
        for dt in DT.values():
            out = ops.unpack_rows(buf, B, C, T, dt)
            assert out.dtype == dt and tuple(out.shape) == (B, C, T) and out.is_contiguous()
            assert torch.equal(out.view(torch.uint8), ref.to(dt).view(torch.uint8)), (src, dt)


@pytest.mark.parametrize("T", [40, 70])
def test_rows_of_roundtrip(T):
    """rows_base is the inverse of rows_view; rows_of recognises such a view (zero copy) and packs anything else — a clone of the
    view, a non-contiguous tensor of equal values — into the same bits."""
    from speech_decoding_amd import ops
    B, C = 3, 70
    for dt in DT.values():
        buf = packed_randn(B, C, T, dt)
        view = ops.rows_view(buf, B, C, T)
        base = ops.rows_base(view, B, C, T, dt)
        assert base is not None and base.shape == buf.shape and base.data_ptr() == buf.data_ptr()
        assert base.untyped_storage().data_ptr() == buf.untyped_storage().data_ptr()
        got, was_view = ops.rows_of(view, C, dt)
        assert was_view and got.data_ptr() == buf.data_ptr()
        assert ops.rows_base(view, B, C, T, torch.float64) is None and ops.rows_base(view.clone(), B, C, T, dt) is None
        strided = view.clone().transpose(1, 2).contiguous().transpose(1, 2)          # (B, C, T) values, t-major memory
        assert not strided.is_contiguous() and torch.equal(strided, view)
        for plain in (view.clone(), view.contiguous(), strided):
            packed, was_view = ops.rows_of(plain, C, dt)
            assert not was_view and packed.data_ptr() != buf.data_ptr()
            assert torch.equal(packed.view(torch.uint8), buf.view(torch.uint8)), dt


@pytest.mark.parametrize("kind", ["sa", "sb", "cb1"])
@pytest.mark.parametrize("dtype", ["bf16", "fp16"])
def test_16bit_input_gives_the_bits_of_its_fp32_values(kind, dtype):
    d = TOY
    loc, P = positions_and_params(d)
    m = build(kind, d, loc, P, dtype, training=False)
    cin, _ = channels(kind, d)
    subj = torch.tensor([0, 1, 2, 0, 1, 2])
    X = torch.randn(d["B"], cin, d["T"]).to(DEV).to(DT[dtype])
    with torch.no_grad():
        assert torch.equal(call(m, kind, X, subj), call(m, kind, X.float(), subj))
