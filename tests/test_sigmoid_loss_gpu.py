"""The pairwise sigmoid loss on a real MI355X.

Per kernel: sda_sigmoid_pairs, sda_sigmoid_finish and sda_sigmoid_grad_y launched on their own over the shapes x regimes x label
patterns x modes of tests/sigmoid_loss_cases.py — through the ops.* wrapper and through the C entry point into sentinel-filled
buffers the test owns — and held to float64 on the fp32 inputs they are handed, within that file's constants; a, diag, the zeros,
the dropped pairs, the rank counts and run-to-run bits exactly.  tests/test_sigmoid_loss_cpu.py shows that these cases catch the
planted bugs.

Whole loss: SigmoidLoss(x, y[, labels]) against float64 autograd on the operands as the device sees them (loss, dZ, dY, dtemp,
dbias), both reductions, both modes, the three compute dtypes, x as a plain tensor and as a rows view, with the project's
per-tensor bounds.  One training step through the encoder and train.py with loss=sigmoid follow."""
import math
import os

import numpy as np
import pytest
import torch

from speech_decoding_amd import SigmoidLoss  # noqa: F401  (the feature under test: without it this file does not import)
from oracle import brain_oracle as O
from tests import builders as TB
from tests import sigmoid_loss_cases as SC
from tests.parity import rel_l2

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
F32 = torch.float32
DT = {"fp32": torch.float32, "bf16": torch.bfloat16, "fp16": torch.float16}
# DESIGN §5's per-tensor bounds: fp32 loss 1e-4 and gradients within 1e-3 of the tensor's largest magnitude; 16-bit loss
# 1e-2 / 2e-3 and gradients 6e-2 / 8e-3 relative L2
LOSS_REL = {"fp32": 1e-4, "bf16": 1e-2, "fp16": 2e-3}
GRAD_FP32_OF_SCALE = 1e-3
GRAD_REL_L2 = {"bf16": 6e-2, "fp16": 8e-3}
WORST = {}
_BASE = {}


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


def cases(shape, regimes=SC.REGIMES):
    """(case, mode) of every variant of a block; one base case per (shape, regime), shared by the tests and left unchanged"""
    for regime in regimes:
        key = (*shape, regime)
        if key not in _BASE:
            _BASE[key] = SC.sig_case(*shape, regime)
        yield from SC.variants(_BASE[key])


def hold(kern, dtype, name, checks):
    """every figure is recorded and printed before anything is asserted on it"""
    torch.cuda.synchronize()
    for k, r in checks.items():
        WORST[(kern, dtype)] = max(WORST.get((kern, dtype), 0.0), r)
        print(f"{kern} {dtype} {name} {k}: error / tolerance {r:.3f}")
    bad = {k: r for k, r in checks.items() if not r <= 1.0}
    assert not bad, (kern, dtype, name, bad)


def dev(t):
    return None if t is None else t.to(DEV).contiguous()


def ptr(t):
    return None if t is None else t.data_ptr()


def sent(shape, dtype=F32):
    return torch.full(shape, SC.SENT, dtype=dtype, device=DEV)


def same(*pairs):
    return SC.exact(all(torch.equal(a, b) for a, b in pairs))


def check_rc(rc, what):
    from speech_decoding_amd import lib
    lib.check(rc, what)


def launch_pairs(ops, c, mode, dtype):
    """sda_sigmoid_pairs into sentinel-filled buffers -> (inputs on the device, (a, diag, G, part))"""
    from speech_decoding_amd import lib
    Bm, Bn, col0 = c["Bm"], c["Bn"], c["col0"]
    ins = [dev(c["S"]), dev(c["ysq"]), dev(c["zsq"]), dev(c["temp"]), dev(c["bias"])]
    lab = dev(c["labels"])
    a, diag, G, part = sent((Bm + 1, Bn)), sent((Bm + 1,)), sent((Bm + 2, SC.pad64(Bn)), dtype), sent(((Bm + 63) // 64 + 1, Bn, 3))
    check_rc(lib.load().sda_sigmoid_pairs(ptr(ins[0]), ins[0].shape[1], *map(ptr, ins[1:]), ptr(lab), ops.clip_dup_code(mode), col0, ptr(a),
                                          ptr(diag), ptr(G), G.shape[1], ptr(part), Bm, Bn, ops.dt_code(dtype), ops._st()), "sigmoid_pairs")
    return ins, lab, (a, diag, G, part)


# ---------------------------------------------------------------------------------------------------------------
# per kernel
# ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", SC.DTYPES, ids=str)
@pytest.mark.parametrize("shape", SC.SHAPES, ids=str)
def test_pairs(ops, dtype, shape):
    Bm, Bn, col0 = shape
    nparts = (Bm + 63) // 64
    for c, mode in cases(shape):
        ins, lab, (a, diag, G, part) = launch_pairs(ops, c, mode, dtype)
        checks = SC.check_pairs(c, mode, dtype, a, diag, G, part)
        w = ops.sigmoid_pairs(*ins, Bm, Bn, col0, dtype, lab, mode)
        checks["the wrapper, a second run, gives the same bits"] = same(*zip(w, (a[:Bm], diag[:Bm], G[:Bm + 1], part[:nparts])))
        if dtype == F32 and (c["pattern"] in (None, "sizes")):
            u = ops.clip_logits_stats(ins[0], ins[1], ins[2], ins[3], Bm, Bn, col0)
            checks["a and diag are clip_logits_stats' bits"] = same((w[0], u[0]), (w[1], u[4]))
            if lab is None:
                checks["rank counts"] = same((ops.clip_ranks(w[0], w[1], col0), ops.clip_ranks(u[0], u[4], col0)))
            else:
                checks["rank counts"] = same((ops.clip_ranks_labels(w[0], w[1], lab, col0), ops.clip_ranks_labels(u[0], u[4], lab, col0)))
        hold(f"sigmoid_pairs[{mode}]", dtype, c["name"], checks)


@pytest.mark.parametrize("shape", SC.SHAPES, ids=str)
def test_finish(ops, shape):
    from speech_decoding_amd import lib
    Bm, Bn, col0 = shape
    for c, mode in cases(shape):
        if c["pattern"] not in (None, "sizes", "one_class"):
            continue
        part32 = SC.pairs_ref(c, mode, F32)["part"].float()                  # the rounded float64 results of the stage before
        ins = [dev(part32), dev(c["ysq"]), dev(c["zsq"]), dev(c["temp"])]
        rs, cs, sc = sent((Bn + 1,)), sent((Bn + 1,)), sent((4,))
        check_rc(lib.load().sda_sigmoid_finish(ptr(ins[0]), part32.shape[0], *map(ptr, ins[1:]), c["inv_norm"], ptr(rs), ptr(cs), ptr(sc), Bm, Bn,
                                               ops._st()), "sigmoid_finish")
        checks = SC.check_finish(c, part32, rs, cs, sc)
        w = ops.sigmoid_finish(*ins, c["inv_norm"])
        checks["the wrapper, a second run, gives the same bits"] = same(*zip(w, (rs[:Bn], cs[:Bn], sc[:3])))
        hold(f"sigmoid_finish[{mode}]", F32, c["name"], checks)


@pytest.mark.parametrize("dtype", SC.DTYPES, ids=str)
@pytest.mark.parametrize("shape", SC.SHAPES, ids=str)
def test_grad_y(ops, dtype, shape):
    from speech_decoding_amd import lib
    Bm, Bn, col0 = shape
    seg, seg_pitch, groups = SC.gy_layout(Bm, Bn, col0)
    nparts = (Bn + 63) // 64
    for c, mode in cases(shape):
        ins = [dev(c["a"]), dev(c["bias"]), dev(c["zsq"]), dev(c["zsq_all"])]
        lab = dev(c["labels"])
        Gy, part = sent((Bn + 2, groups * seg_pitch), dtype), sent((nparts + 1, Bm))
        check_rc(lib.load().sda_sigmoid_grad_y(*map(ptr, ins), Bm, ptr(lab), ops.clip_dup_code(mode), col0, ptr(Gy), Gy.shape[1], seg, seg_pitch,
                                               ptr(part), Bm, Bn, ops.dt_code(dtype), ops._st()), "sigmoid_grad_y")
        checks = SC.check_grad_y(c, mode, dtype, Gy, part)
        w = ops.sigmoid_grad_y(*ins, col0, dtype, lab, mode, seg=seg, seg_pitch=seg_pitch, groups=groups)
        checks["the wrapper, a second run, gives the same bits"] = same((w[0], Gy[:Bn + 1]), (w[1], part[:nparts]))
        hold(f"sigmoid_grad_y[{mode}]", dtype, c["name"], checks)


@pytest.mark.parametrize("dtype", SC.DTYPES, ids=str)
@pytest.mark.parametrize("shape", [(64, 64, 0), (15, 5, 10), (513, 70, 140)], ids=str)
def test_a_dropped_pair_is_left_out_not_multiplied_by_zero(ops, dtype, shape):
    """mask mode with a NaN in S at a dropped pair: G is exactly zero there and every sum keeps the clean run's bits"""
    base = next(cases(shape, ("trained",)))[0]
    for pattern in ("pair", "sizes"):
        c = SC.with_labels(base, pattern)
        p, ij = SC.dropped_pair_case(c)
        _, _, clean = launch_pairs(ops, c, "mask", dtype)
        _, _, got = launch_pairs(ops, p, "mask", dtype)
        hold("sigmoid_pairs[mask] NaN at a dropped pair", dtype, c["name"], SC.check_dropped_nan(ij, got[2], got[3], clean[2], clean[3]))


@pytest.mark.parametrize("dtype", SC.DTYPES, ids=str)
@pytest.mark.parametrize("value", [math.nan, math.inf], ids=str)
@pytest.mark.parametrize("where", ["S", "ysq", "bias"])
def test_nonfinite_inputs_propagate(ops, where, value, dtype):
    for shape in ((15, 5, 10), (140, 70, 70)):
        c = next(cases(shape, ("trained",)))[0]
        p = SC.poisoned(c, where, value)
        _, _, clean = launch_pairs(ops, c, "positive", dtype)
        ins, _, got = launch_pairs(ops, p, "positive", dtype)
        nparts = (c["Bm"] + 63) // 64
        _, _, scalars = ops.sigmoid_finish(got[3][:nparts].contiguous(), ins[1], ins[2], ins[3], c["inv_norm"])
        hold("sigmoid_pairs + finish, non-finite input", dtype, p["name"], SC.check_nonfinite(c, p, where, "positive", dtype, got[2], scalars, clean[2]))


# ---------------------------------------------------------------------------------------------------------------
# whole loss
# ---------------------------------------------------------------------------------------------------------------
def randn(*shape, seed):
    return torch.randn(*shape, generator=torch.Generator().manual_seed(seed))


def batch_labels(B):
    """a pair, a class of three and (B = 70) a class of a quarter of the batch"""
    lab = np.arange(B, dtype=np.int64) + 100
    lab[[1, B - 2]] = 7
    lab[[0, 2, B - 1]] = 8
    if B >= 40:
        lab[10:10 + B // 4] = 9
    return lab


def sigmoid(reduction="mean", temp=2.0, bias=-3.0, duplicates="positive"):
    from speech_decoding.utils.loss import SigmoidLoss
    return SigmoidLoss(TB.Config(reduction=reduction, sigmoid_init_temperature=temp, sigmoid_init_bias=bias, clip_duplicates=duplicates)).to(DEV)


def packed(x, dtype):
    """(B, F, T) -> the rows view of a fresh row-layout buffer of `dtype` whose BUFFER is the leaf (what an encoder hands out)"""
    from speech_decoding_amd import lib as L, ops
    B, F, T = x.shape
    buf = ops.new_rows(B, T, L.pad_channels(F), dtype, DEV)
    ops.pack_rows(x.to(DEV).float(), buf)
    buf.requires_grad_(True)
    return ops.rows_view(buf, B, F, T)


def operands(B, F, T, dtype, x_form, x_grad):
    """speech x and brain y as the device sees them (rounded to the compute dtype): (x, y, their values)"""
    xv = randn(B, F, T, seed=1000 * B).to(DT[dtype])
    yv = (0.6 * xv.float() + randn(B, F, T, seed=1000 * B + 1)).to(DT[dtype])
    y = yv.to(DEV).requires_grad_(True)
    if x_form == "rows":
        x = packed(xv.float(), DT[dtype])
        if not x_grad:
            x = x.detach()
    else:
        x = xv.to(DEV).requires_grad_(x_grad)
    return x, y, xv, yv


def grad_ok(got, ref, dtype):
    """(figure, bound) of DESIGN §5's per-tensor bound"""
    if dtype == "fp32":
        return float((got.double().cpu() - ref).abs().max()), GRAD_FP32_OF_SCALE * float(ref.abs().max())
    return rel_l2(got, ref), GRAD_REL_L2[dtype]


@pytest.mark.parametrize("x_form,x_grad", [("plain", True), ("plain", False), ("rows", True), ("rows", False)])
@pytest.mark.parametrize("dtype", ["fp32", "bf16", "fp16"])
@pytest.mark.parametrize("labels", [None, "positive", "mask"])
@pytest.mark.parametrize("reduction", ["mean", "sum"])
@pytest.mark.parametrize("shape", [(5, 20, 7), (70, 64, 33)], ids=str)
def test_whole_loss_against_float64_autograd(shape, reduction, labels, dtype, x_form, x_grad):
    B, F, T = shape
    x, y, xv, yv = operands(B, F, T, dtype, x_form, x_grad)
    lab = None if labels is None else batch_labels(B)
    crit = sigmoid(reduction, 2.0, -3.0, labels or "positive")
    logits, loss = crit(x, y, return_logits=True, labels=lab)
    grads = torch.autograd.grad(loss, [y, crit.temp, crit.bias] + ([x] if x_grad else []))
    r = SC.loss_ref_embeddings(xv, yv, 2.0, -3.0, lab, labels or "positive", reduction)
    figs = dict(loss=(abs(float(loss.detach()) - float(r["loss"])), LOSS_REL[dtype] * abs(float(r["loss"]))), dy=grad_ok(grads[0], r["dy"], dtype),
                dtemp=(abs(float(grads[1]) - float(r["dtemp"])), LOSS_REL[dtype] * r["abs_Da"]),
                dbias=(abs(float(grads[2]) - float(r["dbias"])), LOSS_REL[dtype] * r["abs_D"]),
                # the operands are the rounded ones on both sides: what is left is fp32 accumulation over K = F T <= 2112 terms, K u
                logits=(rel_l2(logits, r["logits"]), 2112 * 2.0 ** -24))
    if x_grad:
        figs["dx"] = grad_ok(grads[3], r["dx"], dtype)
        assert grads[3].shape == x.shape and grads[3].dtype == x.dtype
    print(shape, reduction, labels, dtype, x_form, x_grad, {k: f"{a:.3e} / {b:.3e}" for k, (a, b) in figs.items()})
    bad = {k: v for k, v in figs.items() if not v[0] <= v[1]}
    assert not bad, bad
    assert loss.dim() == 0 and loss.dtype == torch.float32 and logits.shape == (B, B)
    if labels is not None:           # the labels are in it
        plain = SC.loss_ref_embeddings(xv, yv, 2.0, -3.0, None, "positive", reduction)["loss"]
        assert abs(float(plain) - float(r["loss"])) > 1e-3 * abs(float(r["loss"]))


def test_two_runs_give_the_same_bits_and_the_ranks_are_cached():
    from speech_decoding.models import Classifier
    from speech_decoding_amd import loss as sda_loss
    B, F, T = 70, 64, 33
    x, y, _, _ = operands(B, F, T, "bf16", "plain", True)
    outs = []
    for _ in range(2):
        crit = sigmoid()
        loss = crit(x, y)
        cached = sda_loss._cached_ranks(x, y)
        assert cached is not None
        outs.append((loss.detach().clone(), cached.clone(), *[g.clone() for g in torch.autograd.grad(loss, [x, y, crit.temp, crit.bias])]))
    assert all(torch.equal(u, v) for u, v in zip(*outs))
    clip = TB.clip_loss(2.0, DEV)           # the bias moves no order: the ranks are those of the CLIP loss at the same temperature
    clip(x, y)
    assert torch.equal(sda_loss._cached_ranks(x, y), outs[0][1])
    crit = sigmoid()
    crit(x, y)
    assert torch.equal(Classifier(None).ranks(y, x), outs[0][1])


def test_saturated_logits_stay_finite():
    """e^temp = 22000: every |l| in the hundreds or thousands; the loss is the sum of the wrong pairs' |l|, D is -+1 or 0"""
    B, F, T = 12, 64, 33
    x, y, xv, yv = operands(B, F, T, "fp32", "plain", True)
    crit = sigmoid("mean", 10.0, 0.0)
    loss = crit(x, y)
    dx, dy, dt, db = torch.autograd.grad(loss, [x, y, crit.temp, crit.bias])
    r = SC.loss_ref_embeddings(xv, yv, 10.0, 0.0, None, "positive")
    assert all(bool(torch.isfinite(g).all()) for g in (loss, dx, dy, dt, db))
    assert abs(float(loss.detach()) - float(r["loss"])) <= LOSS_REL["fp32"] * abs(float(r["loss"]))
    assert abs(float(db) - float(r["dbias"])) <= LOSS_REL["fp32"] * r["abs_D"]


# ---------------------------------------------------------------------------------------------------------------
# one training step through the encoder
# ---------------------------------------------------------------------------------------------------------------
def reference_step(P, X, Y, subj, loc, centre, temp, bias):
    """the CPU reference encoder on leaf copies + the float64 sigmoid loss through autograd -> (loss, Z, grads by state key)"""
    leaves = {k: v.detach().clone().requires_grad_(True) for k, v in P.items()
              if (v.is_floating_point() or v.is_complex()) and not k.endswith(("running_mean", "running_var", ".cos", ".sin"))}
    Q = dict(P)
    Q.update(leaves)
    Z = O.brain_encoder_forward(Q, X, subj, training=True, loc=loc, drop_centre=centre)
    t = torch.tensor([temp], dtype=torch.float64, requires_grad=True)
    b = torch.tensor([bias], dtype=torch.float64, requires_grad=True)
    B = X.shape[0]
    Yn, Zn = Y.double().reshape(B, -1), Z.double().reshape(B, -1)
    lg = (Yn / Yn.norm(dim=1, keepdim=True)) @ (Zn / Zn.norm(dim=1, keepdim=True)).T * torch.exp(t) + b
    loss = SC.loss_ref(lg, None, "positive", "mean")
    loss.backward()
    grads = {k: v.grad for k, v in leaves.items()}
    grads.update(temp=t.grad, bias=b.grad)
    return loss.detach(), Z.detach(), grads


def test_train_step_fp32_matches_the_float64_reference():
    d, B = TB.TOY, 6
    loc, P, X, Y, subj = TB.toy_problem(d, B)
    enc = TB.build_encoder(P, TB.encoder_args(d, loc, "fp32"), DEV)
    crit = sigmoid("mean", 2.0, -3.0)
    enc.set_drop_centre(5)
    Yd = Y.to(DEV)
    crit.prefetch(Yd, torch.float32)
    Z = enc(X.to(DEV), subj)
    loss = crit(Yd, Z)
    loss.backward()
    lo, Zo, go = reference_step(P, X, Y, subj, loc, 5, 2.0, -3.0)
    assert float((Z.detach().cpu() - Zo).abs().max()) <= 1e-4 * float(Zo.abs().max())
    assert abs(float(loss.detach()) - float(lo)) <= 1e-4 * float(lo)
    got = TB.grads_of(enc, ("temp", crit.temp), ("bias", crit.bias))
    split = {}
    for k, g in got.items():
        if k == "subject_block.subject_layer.weight":
            split.update({f"subject_block.subject_layer.{s}.weight": g[s] for s in range(g.shape[0])})
        else:
            split[k] = g
    checked = 0
    for k, g in split.items():
        ref = go[k]
        ref = (torch.view_as_real(ref) if ref.is_complex() else ref).float()
        if TB.null_bias_grad(k):
            assert float(g.abs().max()) < 1e-4 * max(1.0, float(go[k.replace(".bias", ".weight")].abs().max())), k
            continue
        assert float((g.float() - ref).abs().max()) <= 1e-3 * float(ref.abs().max()) + 1e-7, k
        checked += 1
    assert checked >= 22 and "temp" in split and "bias" in split


# ---------------------------------------------------------------------------------------------------------------
# train.py with loss=sigmoid
# ---------------------------------------------------------------------------------------------------------------
def run_train(tmp_path, monkeypatch, *extra):
    import train as TR
    from speech_decoding_amd import load_config
    monkeypatch.chdir(tmp_path)
    loc = O.synthetic_positions(12, seed=7)
    args = load_config(overrides=["dataset=Gwilliams2022", "num_subjects=3", "D1=16", "D2=24", "F=32", "K=4", "batch_size=28",
                                  "epochs=4", "num_channels=12", "preprocs.last4layers=False", "preprocs.seq_len_sec=1",
                                  "preprocs.brain_resample_rate=40", "preprocs.baseline_len_sec=0.25", "lr=1e-2",
                                  "synthetic_segments=40", "updates_per_epoch=5", "split_ratio=0.7", "loss=sigmoid", *extra])
    args["sensor_positions"] = loc.numpy()
    torch.manual_seed(0)
    np.random.seed(0)
    lines = []
    hist, enc, lossf = TR.run(args, log=lambda *a: lines.append(" ".join(a)))
    return args, hist, lossf, lines


def check_run(args, hist, lossf, lines, tmp_path):
    from speech_decoding.models import BrainEncoder
    from speech_decoding_amd import SigmoidLoss
    assert isinstance(lossf, SigmoidLoss) and len(hist) == 4 and len(lines) == 4
    assert all("temp" in h and "bias" in h for h in hist) and all("temp: " in line and "bias: " in line for line in lines)
    losses = [h["train_loss"] for h in hist]
    assert all(np.isfinite(losses)) and all(np.isfinite(h["test_loss"]) for h in hist)
    assert all(b < a for a, b in zip(losses, losses[1:])), losses
    assert hist[-1]["temp"] != hist[0]["temp"] and hist[-1]["bias"] != hist[0]["bias"]          # Adam steps both
    assert all(0.0 <= h["testTop10acc"] <= 1.0 for h in hist)
    fresh = BrainEncoder(args)
    missing, unexpected = fresh.load_state_dict(torch.load(os.path.join(tmp_path, "model_last.pt"), map_location="cpu"))
    assert not missing and not unexpected


def test_training_driver_with_sigmoid(tmp_path, monkeypatch):
    args, hist, lossf, lines = run_train(tmp_path, monkeypatch)
    check_run(args, hist, lossf, lines, tmp_path)
    assert lossf.duplicates == "positive"


def test_training_driver_with_sigmoid_masked_and_guarded(tmp_path, monkeypatch):
    args, hist, lossf, lines = run_train(tmp_path, monkeypatch, "clip_duplicates=mask", "max_grad_norm=1.0")
    check_run(args, hist, lossf, lines, tmp_path)
    assert lossf.duplicates == "mask" and all("grad_norm" in h for h in hist)
