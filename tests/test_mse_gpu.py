"""MSELoss on the MI355X: the reference's own numbers (tests/golden/mse.npz), every operand layout and dtype against float64
torch on the same rounded operands, the row-layout buffer contract of dZ, bit-for-bit determinism, no host sync, one training
step through the encoder against the CPU oracle (fp32 and, at the real widths, bf16 / fp16), and train.py with loss=mse."""
import os
import warnings

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from oracle import brain_oracle as O      # noqa: E402
from tests import builders as TB          # noqa: E402
from tests import golden_io as G           # noqa: E402
from tests.parity import operands_as_device_sees_them, rel_l2, round_to   # noqa: E402

DEV = "cuda:0"
DT = {"fp32": torch.float32, "bf16": torch.bfloat16, "fp16": torch.float16}
# one rounding of a gradient into its storage type (round to nearest: half a unit in the last place, relative to the value),
# and the absolute floor of that rounding where the value is subnormal in that type
ROUND_REL = {"fp32": 2.0 ** -22, "bf16": 2.0 ** -8, "fp16": 2.0 ** -11}
ROUND_ABS = {"fp32": 1e-40, "bf16": 1e-38, "fp16": 2.0 ** -24}
FP32_REL = 2.0 ** -21          # the fp32 value before that rounding: three roundings of its own (difference, scale, product)


def mse():
    from speech_decoding.utils.loss import MSELoss
    return MSELoss()


def as_rows(x, dtype):
    """(B, F, T) -> a rows view of a fresh row-layout buffer of `dtype` (what the encoder hands out), leaf buffer."""
    from speech_decoding_amd import lib as L, ops
    B, F, T = x.shape
    buf = ops.new_rows(B, T, L.pad_channels(F), dtype, DEV)
    ops.pack_rows(x.to(DEV).float(), buf)
    return buf, ops.rows_view(buf, B, F, T)


def operand(x, layout, dtype, requires_grad=False):
    """(tensor handed to the loss, its values as float64 on the host)"""
    if layout == "rows":
        buf, v = as_rows(x, DT[dtype])
        if requires_grad:
            buf.requires_grad_(True)
            from speech_decoding_amd import ops
            v = ops.rows_view(buf, *x.shape)
    else:
        v = x.to(DT[dtype]).to(DEV).requires_grad_(requires_grad)
    return v, v.detach().double().cpu()


def is_rows_view(t):
    from speech_decoding_amd import ops
    return ops.rows_base(t, *t.shape, t.dtype) is not None


def ref_mse(Y, Z):
    Y, Z = Y.double().requires_grad_(True), Z.double().requires_grad_(True)
    loss = ((Y - Z) ** 2).sum(dim=(1, 2)).mean()
    dY, dZ = torch.autograd.grad(loss, [Y, Z])
    return loss.detach(), dY, dZ


# ------------------------------------------------------------------------------------------------------------------------------
# 1. the reference's numbers
# ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("z_layout", ["plain", "rows"])
def test_golden_fixture_fp32(z_layout):
    g = G.load("mse.npz")
    for i in range(len(g["shapes"])):
        Y = torch.from_numpy(g[f"s{i}/Y"]).to(DEV).requires_grad_(True)
        Z, _ = operand(torch.from_numpy(g[f"s{i}/Z"]), z_layout, "fp32", requires_grad=True)
        loss = mse()(Y, Z)
        assert loss.dim() == 0 and loss.dtype == torch.float32
        dY, dZ = torch.autograd.grad(loss, [Y, Z])
        ref = float(g[f"s{i}/loss"])
        assert abs(float(loss) - ref) <= 1e-6 * abs(ref), (i, float(loss), ref)
        for got, key in ((dZ, "dZ"), (dY, "dY")):
            want = g[f"s{i}/{key}"]
            err = np.abs(got.float().cpu().numpy() - want).max()
            assert err <= 1e-6 * np.abs(want).max(), (i, key, err)
        assert is_rows_view(dZ) == (z_layout == "rows")


# ------------------------------------------------------------------------------------------------------------------------------
# 2. every layout pair and dtype against float64 on the same rounded operands
# ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", [(3, 80, 40), (2, 200, 37), (1, 1024, 9)], ids=["vector-T", "odd-T", "B1-wide"])
@pytest.mark.parametrize("y_layout", ["plain", "rows"])
@pytest.mark.parametrize("z_layout", ["plain", "rows"])
def test_every_layout_and_dtype_against_float64(z_layout, y_layout, shape):
    g = torch.Generator().manual_seed(sum(shape))
    Yf = torch.randn(*shape, generator=g)
    Zf = torch.randn(*shape, generator=g) * 0.7 + 0.2 * Yf
    for zd in DT:
        for yd in DT:
            Y, Yr = operand(Yf, y_layout, yd, requires_grad=True)
            Z, Zr = operand(Zf, z_layout, zd, requires_grad=True)
            loss = mse()(Y, Z)
            dY, dZ = torch.autograd.grad(loss * 3.0, [Y, Z])             # d loss = 3, read on the device
            lr, dYr, dZr = ref_mse(Yr, Zr)
            tag = (z_layout, zd, y_layout, yd)
            assert abs(float(loss) - float(lr)) <= 1e-5 * float(lr), tag
            for got, want, d, lay, name in ((dZ, 3 * dZr, zd, z_layout, "dZ"), (dY, 3 * dYr, yd, y_layout, "dY")):
                assert got.dtype == DT[d] and tuple(got.shape) == shape and is_rows_view(got) == (lay == "rows"), (tag, name)
                err = (got.double().cpu() - want).abs()
                bound = (ROUND_REL[d] + FP32_REL) * want.abs() + ROUND_ABS[d]
                assert bool((err <= bound).all()), (tag, name, float((err - bound).max()))


def test_plain_non_contiguous_operands_are_accepted():
    g = torch.Generator().manual_seed(5)
    Y = torch.randn(4, 37, 66, generator=g).to(DEV).transpose(1, 2)                 # (4, 66, 37), non-contiguous
    Z = torch.randn(4, 37, 66, generator=g).to(DEV).transpose(1, 2).requires_grad_(True)
    loss = mse()(Y, Z)
    (dZ,) = torch.autograd.grad(loss, [Z])
    lr, _, dZr = ref_mse(Y.cpu(), Z.detach().cpu())
    assert abs(float(loss) - float(lr)) <= 1e-6 * float(lr)
    assert float((dZ.double().cpu() - dZr).abs().max()) <= 1e-6 * float(dZr.abs().max())


def test_errors():
    from speech_decoding_amd import SdaError
    Y = torch.randn(2, 8, 5, device=DEV)
    with pytest.raises(SdaError, match="no CPU path"):
        mse()(Y, torch.randn(2, 8, 5))
    with pytest.raises(ValueError):
        mse()(Y, torch.randn(2, 8, 6, device=DEV))
    with pytest.raises(SdaError, match="unsupported compute dtype"):
        mse()(Y, torch.randn(2, 8, 5, device=DEV, dtype=torch.float64))
    one = mse()(Y[:1], Y[:1] + 1.0)                       # B = 1 is allowed
    assert float(one) == pytest.approx(40.0, rel=1e-6)


# ------------------------------------------------------------------------------------------------------------------------------
# 3. the row-layout buffer contract of dZ
# ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", ["bf16", "fp32"])
def test_rows_dz_buffer_contract_on_poisoned_memory(dtype):
    from speech_decoding_amd import lib as L
    from speech_decoding_amd import ops
    B, F, T = 5, 100, 45
    Cp = L.pad_channels(F)
    g = torch.Generator().manual_seed(11)
    Y = torch.randn(B, F, T, generator=g).to(DEV)
    _, Z = as_rows(torch.randn(B, F, T, generator=g), DT[dtype])
    Z.requires_grad_(True)
    for _ in range(2):
        # fill the caching allocator's free block of dZ's size with NaN: the backward's buffer comes back out of it
        nbytes = L.rows_alloc(B, T) * Cp * torch.finfo(DT[dtype]).bits // 8
        junk = torch.full((nbytes // 4,), float("nan"), dtype=torch.float32, device=DEV)
        del junk
        (dZ,) = torch.autograd.grad(mse()(Y, Z), [Z])
        buf = ops.rows_base(dZ, B, F, T, DT[dtype]).float().cpu()
        Tp = L.rows_tp(T)
        valid = torch.zeros(buf.shape[0], dtype=torch.bool)
        for b in range(B):
            valid[b * Tp + L.ROW_PAD: (b + 1) * Tp] = True
        assert bool(torch.isfinite(buf).all())
        assert bool((buf[~valid] == 0).all())                      # pad rows and the slack behind the last sample
        assert bool((buf[valid][:, F:] == 0).all())               # pad channels
        assert not bool(torch.signbit(buf[:, F:]).any())           # +0, not -0
        want = 2.0 * (Z.detach().double().cpu() - Y.double().cpu()) / B
        assert float((dZ.double().cpu() - want).abs().max()) <= ROUND_REL[dtype] * float(want.abs().max())


# ------------------------------------------------------------------------------------------------------------------------------
# 4. determinism
# ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", ["bf16", "fp32"])
def test_same_bits_every_call(dtype):
    B, F, T = 24, 1024, 360                      # 9216 tiles: every workgroup of the fixed grid takes several
    g = torch.Generator(device=DEV).manual_seed(3)
    Y = torch.randn(B, F, T, generator=g, device=DEV)
    _, Z = as_rows(torch.randn(B, F, T, generator=g, device=DEV), DT[dtype])
    Z.requires_grad_(True)
    crit = mse()
    runs = []
    for _ in range(2):
        loss = crit(Y, Z)
        (dZ,) = torch.autograd.grad(loss, [Z])
        runs.append((loss.clone(), dZ.clone()))
    assert torch.equal(runs[0][0], runs[1][0]) and torch.equal(runs[0][1], runs[1][1])
    # a no-grad evaluation forward on other operands between a forward and its backward changes nothing
    loss = crit(Y, Z)
    with torch.no_grad():
        other = crit(Y * 0.5, Z.detach() + 1.0)
    (dZ,) = torch.autograd.grad(loss, [Z])
    assert torch.equal(loss, runs[0][0]) and torch.equal(dZ, runs[0][1])
    assert not torch.equal(other, loss)


# ------------------------------------------------------------------------------------------------------------------------------
# 5. no host synchronisation in forward or backward
# ------------------------------------------------------------------------------------------------------------------------------
def test_forward_and_backward_never_sync_the_host():
    B, F, T = 6, 1024, 360
    Y = torch.randn(B, F, T, device=DEV)
    _, Z = as_rows(torch.randn(B, F, T, device=DEV), torch.bfloat16)
    Z.requires_grad_(True)
    crit = mse()
    w = torch.full((), 0.25, device=DEV)
    Yp = torch.randn(B, F, T, device=DEV, dtype=torch.float16).requires_grad_(True)
    torch.autograd.grad(crit(Yp, Z), [Yp, Z])        # first calls: library load, allocator warm-up
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        loss = crit(Y, Z)
        (dZ,) = torch.autograd.grad(loss * w, [Z])   # d loss = w, read on the device
        crit(Yp, Z).backward()                        # Y: a leaf, its gradient accumulated; Z's through the view
        dY, dZ2 = torch.autograd.grad(crit(Yp, Z), [Yp, Z])
    finally:
        torch.cuda.set_sync_debug_mode(0)
    torch.cuda.synchronize()
    assert Yp.grad is not None and torch.isfinite(dZ.float()).all() and torch.isfinite(dY.float()).all()
    assert torch.equal(dY, Yp.grad)


# ------------------------------------------------------------------------------------------------------------------------------
# 6-7. one training step through the encoder against the CPU oracle
# ------------------------------------------------------------------------------------------------------------------------------
def make_encoder(C, S, D1, D2, F, K, P, loc, dtype, last4):
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        return TB.build_encoder(P, TB.encoder_args(dict(S=S, D1=D1, D2=D2, F=F, K=K), loc, dtype, last4), DEV)


def oracle_mse_step(P, X, Y, subj, loc, centre, taps=None):
    """oracle.brain_encoder_forward on leaf copies + a float64 MSE through torch autograd -> (loss, Z, grads by state key)."""
    leaves = {k: v.detach().clone().requires_grad_(True) for k, v in P.items()
              if (v.is_floating_point() or v.is_complex()) and not k.endswith(("running_mean", "running_var", ".cos", ".sin"))}
    Q = dict(P)
    Q.update(leaves)
    Z = O.brain_encoder_forward(Q, X, subj, training=True, loc=loc, drop_centre=centre, taps=taps)
    loss = ((Y.double() - Z.double()) ** 2).sum(dim=(1, 2)).mean()
    loss.backward()
    return loss.detach(), Z.detach(), {k: v.grad for k, v in leaves.items()}


def test_train_step_fp32_matches_oracle():
    C, S, D1, D2, F, K, T, B = 20, 3, 32, 48, 64, 4, 90, 6
    loc, P, X, Y, subj = TB.toy_problem(dict(C=C, S=S, D1=D1, D2=D2, F=F, K=K, T=T), B)
    enc = make_encoder(C, S, D1, D2, F, K, P, loc, "fp32", False)
    enc.set_drop_centre(5)
    Z = enc(X.to(DEV), subj)
    loss = mse()(Y.to(DEV), Z)
    loss.backward()
    lo, Zo, go = oracle_mse_step(P, X, Y, subj, loc, 5)
    assert float((Z.detach().cpu() - Zo).abs().max()) <= 1e-4 * float(Zo.abs().max())
    assert abs(float(loss) - float(lo)) <= 1e-4 * float(lo)
    checked = 0
    for k, g in TB.grads_by_state_key(enc).items():
        ref = go[k]
        if TB.null_bias_grad(k):
            assert float(g.abs().max()) < 1e-4 * max(1.0, float(go[k.replace(".bias", ".weight")].abs().max())), k
            continue
        gf = (torch.view_as_real(g) if g.is_complex() else g).float().cpu()
        rf = (torch.view_as_real(ref) if ref.is_complex() else ref).float()
        assert float((gf - rf).abs().max()) <= 1e-3 * float(rf.abs().max()) + 1e-7, k
        checked += 1
    assert checked >= 20


# relative L2 bounds of the 16-bit step, those tests/test_e2e_gpu.py holds the CLIP step to (storage rounding between kernels)
Z_REL = {"bf16": 4e-2, "fp16": 5e-3}
LOSS_REL = {"bf16": 1e-2, "fp16": 2e-3}
GRAD_REL = {"bf16": 6e-2, "fp16": 8e-3}
CANCEL_SUM = "subject_block.conv.bias"          # a cancelling sum: bounded against the norm of its terms (test_e2e_gpu.py)
CANCEL_REL = {"bf16": 6e-2, "fp16": 8e-3}


@pytest.mark.parametrize("dtype", ["bf16", "fp16"])
def test_train_step_16bit_at_real_widths_against_oracle_on_rounded_operands(dtype):
    from speech_decoding_amd.amp import LossScaler
    C, S, D1, D2, F, K, T, B = 208, 27, 270, 320, 1024, 32, 360, 12
    loc, P, X, Y, subj = TB.toy_problem(dict(C=C, S=S, D1=D1, D2=D2, F=F, K=K, T=T), B, 0, 0, 1234)
    enc = make_encoder(C, S, D1, D2, 512, K, P, loc, dtype, True)
    scaler = LossScaler.for_dtype(DT[dtype])           # fp16: the static scale train.py starts from, halved on overflow
    for _ in range(12):
        enc.zero_grad(set_to_none=True)
        enc.set_drop_centre(9)
        Z = enc(X.to(DEV), subj)
        assert Z.dtype == DT[dtype] and is_rows_view(Z)
        loss = mse()(Y.to(DEV), Z)                      # Y: plain fp32, never packed
        scaler.scale(loss).backward()
        ok = scaler.unscale_(list(enc.parameters()), check=True)
        scaler.update(ok)
        if ok:
            break
    assert ok
    taps = {}
    lo, Zo, go = oracle_mse_step(operands_as_device_sees_them(P, dtype), round_to(X, dtype), Y, subj, loc, 9, taps=taps)
    report = {"Z": (rel_l2(Z.detach().float(), Zo), Z_REL[dtype]),
              "loss": (abs(float(loss.detach()) - float(lo)) / float(lo), LOSS_REL[dtype])}
    for k, g in TB.grads_by_state_key(enc).items():
        ref = go[k]
        if ref is None:                                  # a subject absent from the batch
            assert g is None or float(g.abs().max()) == 0.0, k
            continue
        if TB.null_bias_grad(k):
            assert float(g.abs().max()) < 5e-2 * max(1.0, float(go[k.replace(".bias", ".weight")].abs().max())), k
            continue
        if k == CANCEL_SUM:
            terms = taps["subject_block.conv.out"].grad
            scale = float(terms.double().pow(2).sum(dim=(0, 2)).sqrt().norm())
            report["grad " + k + " / |terms|"] = (float((g.double().cpu() - ref.double()).norm()) / scale, CANCEL_REL[dtype])
            continue
        report["grad " + k] = (rel_l2(g, ref), GRAD_REL[dtype])
    bad = {k: v for k, v in report.items() if not v[0] <= v[1]}
    assert not bad, f"{dtype}: " + ", ".join(f"{k}: {v[0]:.3e} > {v[1]:.1e}" for k, v in bad.items())


# ------------------------------------------------------------------------------------------------------------------------------
# train.py with loss=mse
# ------------------------------------------------------------------------------------------------------------------------------
def test_training_driver_with_mse(tmp_path, monkeypatch):
    import train as TR
    from speech_decoding.models import BrainEncoder
    from speech_decoding_amd import MSELoss, load_config
    monkeypatch.chdir(tmp_path)
    loc = O.synthetic_positions(12, seed=7)
    args = load_config(overrides=["dataset=Gwilliams2022", "num_subjects=3", "D1=16", "D2=24", "F=32", "K=4", "batch_size=28",
                                  "epochs=4", "num_channels=12", "preprocs.last4layers=False", "preprocs.seq_len_sec=1",
                                  "preprocs.brain_resample_rate=40", "preprocs.baseline_len_sec=0.25", "lr=1e-2",
                                  "synthetic_segments=40", "updates_per_epoch=5", "split_ratio=0.7", "loss=mse"])
    args["sensor_positions"] = loc.numpy()
    torch.manual_seed(0)
    np.random.seed(0)
    lines = []
    hist, enc, lossf = TR.run(args, log=lambda *a: lines.append(" ".join(a)))
    assert isinstance(lossf, MSELoss) and len(hist) == 4 and len(lines) == 4
    assert all("temp" not in h for h in hist) and all("temp" not in line for line in lines)
    losses = [h["train_loss"] for h in hist]
    assert all(np.isfinite(losses)) and all(np.isfinite(h["test_loss"]) for h in hist)
    # every batch is the whole 28-segment training split (in a new order): the epochs differ by the training alone
    # (the fp32 CPU oracle on this setup: 1746, 1717, 1645, 1522)
    assert all(b < a for a, b in zip(losses, losses[1:])) and losses[-1] < 0.95 * losses[0], losses
    assert all(0.0 <= h["testTop10acc"] <= 1.0 for h in hist)
    fresh = BrainEncoder(args)
    missing, unexpected = fresh.load_state_dict(torch.load(os.path.join(tmp_path, "model_last.pt"), map_location="cpu"))
    assert not missing and not unexpected
