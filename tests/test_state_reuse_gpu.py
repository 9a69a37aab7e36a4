"""Warm state never changes a result: one scripted training sequence on long-lived objects (reused workspace buffers, the
two-shape LRU of buffer sets, no-grad ping-pong buffers shared across layer widths, the loss's packed-input ring, the norm and
rank caches, the packed-operand caches, side-stream backward with no host synchronisation between calls) against cold runs.

The engine has no atomics, so a call on brand-new objects (engine.reuse_workspace = False) loaded with the warm objects' state
just before that call is an exact reference: every output, gradient, parameter and running statistic must match bit for bit.
The warm sequence runs first, queued back to back; its per-call snapshots (device clones, stream-ordered) and results are
compared afterwards, one fresh set of objects per call.  test_warm_sequence_anchor_against_the_oracle ties the first calls to
the CPU oracle so that the sequence is right, not only self-consistent."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from oracle import brain_oracle as O                       # noqa: E402
from tests.builders import build_encoder, null_bias_grad     # noqa: E402
from tests.test_e2e_gpu import make_args                      # noqa: E402

DEV = "cuda:0"
LR = 1e-4
# real widths (D1 = 270 and D2 = 320 both pad to 320, F = 1024 with last4layers), small batches; (B, T), ragged B', third T''
SHAPES = {
    "gwilliams": dict(C=208, S=27, B=16, T=130, B2=11, T3=360),
    "brennan": dict(C=60, S=1, B=24, T=40, B2=10, T3=129),
}
D1, D2, F, K = 270, 320, 1024, 32


def _clone(x):
    if torch.is_tensor(x):
        return x.detach().clone()
    if isinstance(x, dict):
        return {k: _clone(v) for k, v in x.items()}
    if isinstance(x, (list, tuple)):
        return type(x)(_clone(v) for v in x)
    return x


def _bits(t):
    if t.is_complex():
        t = torch.view_as_real(t)
    if t.dtype == torch.bool:
        return t
    return t.contiguous().view({8: torch.int64, 4: torch.int32, 2: torch.int16, 1: torch.uint8}[t.element_size()])


class World:
    """BrainEncoder + CLIPLoss + Classifier + torch.optim.Adam (as train.py) in a given state."""

    def __init__(self, shape, dtype, composed, snap, cold):
        from speech_decoding.models import Classifier
        from speech_decoding.utils.loss import CLIPLoss
        self.loc = O.synthetic_positions(shape["C"], seed=0)
        args = make_args(shape["C"], shape["S"], D1, D2, F, K, True, self.loc, dtype)
        self.enc = build_encoder(snap["enc"], args, DEV)
        self.lossf = CLIPLoss(args).to(DEV)
        self.clf = Classifier(args)
        with torch.no_grad():
            self.lossf.temp.copy_(snap["temp"])
        eng = self.enc.engine
        eng.compose_subject_block = composed
        assert eng.composed == composed
        eng.reuse_workspace = not cold
        self.opt = torch.optim.Adam(list(self.enc.parameters()) + list(self.lossf.parameters()), lr=LR)
        if snap.get("opt") is not None:
            self.opt.load_state_dict(_clone(snap["opt"]))

    def snapshot(self):
        return {"enc": _clone(self.enc.state_dict()), "temp": self.lossf.temp.detach().clone(),
                "opt": _clone(self.opt.state_dict())}


# ---------------------------------------------------------------------------------------------------- the scripted calls
def _rec_state(w, rec):
    for k, v in w.enc.state_dict().items():
        rec["state " + k] = v.detach().clone()
    rec["temp"] = w.lossf.temp.detach().clone()


def _rec_grads(w, rec):
    for n, p in w.enc.named_parameters():
        assert p.grad is not None, n
        rec["grad " + n] = p.grad.detach().clone()
    rec["grad temp"] = w.lossf.temp.grad.detach().clone()


def _forward_loss(w, bt, centre, rec, tag=""):
    X, Y, subj = bt
    w.enc.train()
    w.enc.set_drop_centre(centre)
    Z = w.enc(X, subj)
    logits, loss = w.lossf(Y, Z, return_logits=True)
    rec["Z" + tag], rec["loss" + tag], rec["logits" + tag] = Z.detach().clone(), loss.detach().clone(), logits.clone()
    rec["ranks" + tag] = w.clf.ranks(Z, Y).clone()
    return Z, loss


def train_step(bt, centre):
    def call(w, rec):
        _, loss = _forward_loss(w, bt, centre, rec)
        w.opt.zero_grad()
        loss.backward()
        _rec_grads(w, rec)
        w.opt.step()
        _rec_state(w, rec)
    return call


def eval_forward(bt):
    def call(w, rec):
        X, _, subj = bt
        w.enc.eval()
        with torch.no_grad():
            rec["Z"] = w.enc(X, subj).clone()
        w.enc.train()
    return call


def nograd_train_forward(bt, centre):
    """Training-mode forward under no_grad: BatchNorm still moves its running statistics (torch semantics)."""
    def call(w, rec):
        X, _, subj = bt
        w.enc.train()
        w.enc.set_drop_centre(centre)
        with torch.no_grad():
            rec["Z"] = w.enc(X, subj).clone()
        _rec_state(w, rec)
    return call


def forward_eval_then_backward(bt, bt_eval, centre):
    """A training forward, a no-grad eval forward of another batch, then the pending backward of the first."""
    def call(w, rec):
        _, loss = _forward_loss(w, bt, centre, rec)
        w.enc.eval()
        with torch.no_grad():
            rec["Z eval"] = w.enc(bt_eval[0], bt_eval[2]).clone()
        w.enc.train()
        w.opt.zero_grad()
        loss.backward()
        _rec_grads(w, rec)
        w.opt.step()
        _rec_state(w, rec)
    return call


def two_losses_one_backward(bt, Y2, centre):
    """Two CLIPLoss forwards on the same Z (within ring_depth) before the backward of the first."""
    def call(w, rec):
        Z, loss = _forward_loss(w, bt, centre, rec)
        logits2, loss2 = w.lossf(Y2, Z, return_logits=True)
        rec["loss 2"], rec["logits 2"] = loss2.detach().clone(), logits2.clone()
        w.opt.zero_grad()
        loss.backward()
        _rec_grads(w, rec)
        w.opt.step()
        _rec_state(w, rec)
    return call


def classifier_after_edit(bt, cold_reference):
    """Classifier on the Z the loss just saw (rank cache hit), then after an in-place edit of Z through a view (must miss; the
    loss on the edited Z must not take the norms the encoder left either).  The cold run drops the rank cache before its
    second call: its result is the rank count computed from scratch."""
    def call(w, rec):
        from speech_decoding_amd import loss as loss_mod
        X, Y, subj = bt
        w.enc.eval()
        with torch.no_grad():
            Z = w.enc(X, subj)
            rec["loss"] = w.lossf(Y, Z).clone()
            rec["ranks"] = w.clf.ranks(Z, Y).clone()
            Z[: Z.shape[0] // 2].neg_()
            if cold_reference:
                loss_mod._rank_cache.clear()
            rec["ranks edited"] = w.clf.ranks(Z, Y).clone()
            rec["loss edited"] = w.lossf(Y, Z if not cold_reference else Z.clone()).clone()
        w.enc.train()
    return call


def sequence(shape, batches):
    B, T, B2, T3 = shape["B"], shape["T"], shape["B2"], shape["T3"]
    b = batches
    return [
        ("step 1 (B, T)", train_step(b[(B, T, 0)], 3)),
        ("step 2 (B, T)", train_step(b[(B, T, 1)], 17)),
        ("step 3 (B, T)", train_step(b[(B, T, 2)], 5)),
        ("no-grad eval forward", eval_forward(b[(B, T, 3)])),
        ("no-grad training forward", nograd_train_forward(b[(B, T, 4)], 9)),
        ("ragged step (B', T)", train_step(b[(B2, T, 0)], 11)),
        ("step at a third shape (B, T'')", train_step(b[(B, T3, 0)], 2)),
        ("step back at (B, T)", train_step(b[(B, T, 5)], 7)),
        ("training forward, eval forward, then backward", forward_eval_then_backward(b[(B, T, 6)], b[(B, T, 7)], 13)),
        ("two loss forwards, one backward", two_losses_one_backward(b[(B, T, 8)], b[(B, T, 9)][1], 1)),
        ("classifier before and after an edit of Z", None),        # (built per run: the cold run differs)
    ]


def make_batches(shape):
    B, T, B2, T3, C, S = shape["B"], shape["T"], shape["B2"], shape["T3"], shape["C"], shape["S"]
    out = {}
    for (b, t, n) in [(B, T, i) for i in range(10)] + [(B2, T, 0), (B, T3, 0)]:
        X, Y, subj = O.synthetic_batch(b, C, t, F, S, seed=1000 * b + 10 * t + n)
        out[(b, t, n)] = (X.to(DEV), Y.to(DEV), subj)
    return out


def initial_snapshot(shape, dtype, composed):
    C, S = shape["C"], shape["S"]
    loc = O.synthetic_positions(C, seed=0)
    P = O.seeded_params(C, S, D1, D2, F, K, seed=C + S, loc=loc)
    temp = torch.tensor([5.1])
    snap = {"enc": {k: v.to(DEV) for k, v in P.items()}, "temp": temp.to(DEV), "opt": None}
    return P, temp, snap


def run_warm(shape, dtype, composed, calls_upto=None):
    """Runs the scripted sequence on one warm World; returns (snapshots before each call, records, the calls, batches)."""
    batches = make_batches(shape)
    _, _, snap0 = initial_snapshot(shape, dtype, composed)
    warm = World(shape, dtype, composed, snap0, cold=False)
    calls = sequence(shape, batches)
    calls[-1] = (calls[-1][0], classifier_after_edit(batches[(shape["B"], shape["T"], 0)], False))
    if calls_upto is not None:
        calls = calls[:calls_upto]
    torch.cuda.synchronize()
    snaps, recs = [], []
    for _, call in calls:                          # back to back: no host synchronisation between the calls
        snaps.append(warm.snapshot())
        rec = {}
        call(warm, rec)
        recs.append(rec)
    torch.cuda.synchronize()
    return snaps, recs, calls, batches, warm


def compare(label, got, want):
    assert got.keys() == want.keys(), (label, sorted(set(got) ^ set(want)))
    for name in want:
        a, b = got[name], want[name]
        assert a.shape == b.shape and a.dtype == b.dtype, f"{label}: {name}: {a.shape}/{a.dtype} vs {b.shape}/{b.dtype}"
        ba, bb = _bits(a), _bits(b)
        if not torch.equal(ba, bb):
            idx = tuple(int(i) for i in (ba != bb).nonzero()[0])
            va = (torch.view_as_real(a) if a.is_complex() else a)[idx]
            vb = (torch.view_as_real(b) if b.is_complex() else b)[idx]
            raise AssertionError(f"{label}: warm {name} differs from the cold run; first at index {idx}: "
                                 f"{va.tolist()} (warm) vs {vb.tolist()} (cold)")


@pytest.mark.parametrize("composed", [True, False])
@pytest.mark.parametrize("dtype", ["fp32", "bf16", "fp16"])
@pytest.mark.parametrize("shape_name", ["gwilliams", "brennan"])
def test_warm_sequence_equals_cold_calls_bit_for_bit(shape_name, dtype, composed):
    shape = SHAPES[shape_name]
    snaps, recs, calls, batches, warm = run_warm(shape, dtype, composed)
    del warm
    cold_calls = sequence(shape, batches)
    cold_calls[-1] = (cold_calls[-1][0], classifier_after_edit(batches[(shape["B"], shape["T"], 0)], True))
    for i, ((label, call), snap, rec) in enumerate(zip(cold_calls, snaps, recs)):
        cold = World(shape, dtype, composed, snap, cold=True)
        want = {}
        call(cold, want)
        compare(f"{shape_name} {dtype} composed={composed}, call {i + 1} ({label})", rec, want)
        del cold
    last = recs[-1]                                # the edit must have changed the ranks, else the cache check proves nothing
    assert not torch.equal(last["ranks"], last["ranks edited"])


def test_warm_sequence_anchor_against_the_oracle():
    """fp32, Gwilliams-like: the first five calls of the warm sequence (three steps, an eval forward, a no-grad training forward
    that moves the running statistics, a ragged step) against the CPU oracle — per call on the state the GPU held before it
    (test_e2e_gpu's one-step tolerances), and the final parameters and running statistics against the oracle's own run of
    the same five calls with torch.optim.Adam on the CPU (test_e2e_gpu's Adam tolerance per step)."""
    shape = SHAPES["gwilliams"]
    snaps, recs, calls, batches, warm = run_warm(shape, "fp32", True, calls_upto=6)
    del warm
    B, T, B2 = shape["B"], shape["T"], shape["B2"]
    plan = [("step", (B, T, 0), 3), ("step", (B, T, 1), 17), ("step", (B, T, 2), 5), ("eval", (B, T, 3), None),
            ("nograd", (B, T, 4), 9), ("step", (B2, T, 0), 11)]
    P0, temp0, _ = initial_snapshot(shape, "fp32", True)
    loc = O.synthetic_positions(shape["C"], seed=0)
    cpu = lambda t: t.detach().cpu()                                    # noqa: E731
    stat_key = lambda k: "running" in k or "num_batches" in k           # noqa: E731
    # the oracle's own trajectory: its parameters stepped by torch.optim.Adam on the CPU
    leaves = {k: v.clone().requires_grad_(True) for k, v in P0.items()
              if (v.is_floating_point() or v.is_complex()) and not stat_key(k) and not k.endswith((".cos", ".sin"))}
    otemp = temp0.clone().requires_grad_(True)
    oopt = torch.optim.Adam(list(leaves.values()) + [otemp], lr=LR)
    ostats = {k: v.clone() for k, v in P0.items() if stat_key(k)}
    nsteps = 0
    for i, (kind, key, centre) in enumerate(plan):
        X, Y, subj = (cpu(t) if torch.is_tensor(t) else t for t in batches[key])
        rec = recs[i]
        # (a) this call on the GPU's own state before it
        Pg = {k: cpu(v) for k, v in snaps[i]["enc"].items()}
        tg = cpu(snaps[i]["temp"])
        sg = {k: v.clone() for k, v in Pg.items() if stat_key(k)}
        if kind == "step":
            lo, Zo, _, go = O.train_step(Pg, tg, X, Y, subj, loc=loc, drop_centre=centre, stats=sg)
            np.testing.assert_allclose(cpu(rec["Z"]).numpy(), Zo.numpy(), rtol=1e-4, atol=1e-4 * float(Zo.abs().max()),
                                       err_msg=f"call {i + 1}: Z")
            assert abs(float(rec["loss"]) - float(lo)) < 1e-4, (i, float(rec["loss"]), float(lo))
            for n, p in go.items():
                if n == "temp" or n.startswith("subject_block.subject_layer."):
                    continue
                g = cpu(rec["grad " + n])
                if null_bias_grad(n):
                    assert float(g.abs().max()) < 1e-4, n
                    continue
                scale = max(float(p.abs().max()), 1e-8)
                assert float((g - p).abs().max()) <= 1e-3 * scale + 1e-7, (i, n, float((g - p).abs().max()), scale)
            gs = cpu(rec["grad subject_block.subject_layer.weight"])
            for s in range(shape["S"]):
                ref = go[f"subject_block.subject_layer.{s}.weight"]
                if ref is None:                                                 # no sample of subject s in this batch
                    assert float(gs[s].abs().max()) == 0.0, (i, s)
                    continue
                assert float((gs[s] - ref).abs().max()) <= 1e-3 * max(float(ref.abs().max()), 1e-8) + 1e-7, (i, s)
        elif kind in ("eval", "nograd"):
            Zo = O.brain_encoder_forward(Pg, X, subj, training=kind == "nograd", loc=loc, drop_centre=centre, stats=sg)
            np.testing.assert_allclose(cpu(rec["Z"]).numpy(), Zo.numpy(), rtol=1e-4, atol=1e-4 * float(Zo.abs().max()),
                                       err_msg=f"call {i + 1}: Z")
        if kind in ("step", "nograd"):
            for k, v in sg.items():
                got = cpu(rec["state " + k])
                if "num_batches" in k:
                    assert int(got) == int(v), (i, k)
                else:
                    np.testing.assert_allclose(got.numpy(), v.numpy(), rtol=1e-4, atol=1e-5, err_msg=f"call {i + 1}: {k}")
        # (b) the oracle's own trajectory
        Po = {k: v.detach() for k, v in leaves.items()}
        Po.update({k: v for k, v in P0.items() if k.endswith((".cos", ".sin"))})
        Po.update(ostats)
        if kind == "step":
            _, _, _, go = O.train_step(Po, otemp.detach(), X, Y, subj, loc=loc, drop_centre=centre, stats=ostats)
            for k, leaf in leaves.items():
                leaf.grad = torch.zeros_like(leaf) if null_bias_grad(k) else go[k]     # exactly zero in exact arithmetic
            otemp.grad = go["temp"]
            oopt.step()
            nsteps += 1
        elif kind == "nograd":
            O.brain_encoder_forward(Po, X, subj, training=True, loc=loc, drop_centre=centre, stats=ostats)
    final = recs[-1]
    lim = 2 * LR * nsteps + 1e-6                   # Adam moves an entry whose gradient is rounding noise by up to +-lr per step
    for k, leaf in leaves.items():
        got = cpu(final["state " + k])
        assert got.shape == leaf.shape, k
        d = float((torch.view_as_real(got) - torch.view_as_real(leaf.detach())).abs().max()) if got.is_complex() \
            else float((got - leaf.detach()).abs().max())
        assert d <= lim, (k, d, lim)
    assert abs(float(final["temp"]) - float(otemp)) <= lim
    for k, v in ostats.items():
        got = cpu(final["state " + k])
        if "num_batches" in k:
            assert int(got) == int(v) == 5, k
        else:
            np.testing.assert_allclose(got.numpy(), v.numpy(), rtol=1e-4, atol=2e-4, err_msg=k)
