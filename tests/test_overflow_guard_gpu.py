"""The fp16 overflow guard, run for real on an MI355X: train.make_backward_and_step with the project's Adam and
LossScaler(scale, enabled=True) on the toy shape, under CLIPLoss and MSELoss, single process and two data-parallel ranks; and
under the losses whose kernels tests/test_nonfinite_losses_gpu.py holds — CLIPLoss with speech labels (one repeated segment in
the batch, as a positive and masked), CLIPLoss with extra negatives from a small WindowBank, SigmoidLoss — single process, the
labelled loss (mask) on two ranks as well.

An activation gradient that overflows fp16 must reach a parameter gradient as inf / NaN (tests/test_nonfinite_gpu.py holds every
kernel on the way to that); then unscale_(check=True) returns False, the step is skipped and the scale halved.  A swallowed
overflow would not crash: Adam would be fed a wrong, finite gradient.

The overflow scale comes from the float64 oracle, never from the code under test: g = max |dL/dZ| at scale 1, and the scale is
the smallest power of two s with s g >= 4 x 65504 — two binades past fp16's range, far more than the fp16 path's gradient error
(GRAD_REL 8e-3 in tests/test_e2e_gpu.py), so the first stored activation gradient overflows whatever the rounding does.
Backward is linear in the scale: no other number is needed.  The default scale (1024) at these shapes is the one
tests/test_e2e_gpu.py asserts healthy: it is the "no false alarm" scale here."""
import math

import numpy as np
import pytest
import torch
import torch.nn.functional as TF

pytestmark = pytest.mark.gpu

from oracle import brain_oracle as O                                                 # noqa: E402
from tests.builders import TOY, build_encoder, clip_loss, encoder_args, toy_problem   # noqa: E402
from tests.ranks import run_ranks                                                     # noqa: E402

DEV = "cuda:0"
B = 12                        # one process; two ranks take 6 each
TEMP = 3.0
CENTRE = 4
FP16_MAX = 65504.0
MARGIN = 4.0
LOSSES = ["clip", "mse"]
# the losses that came after: CLIPLoss with speech labels (a repeated segment counted as a positive, or masked), CLIPLoss with
# extra negatives from a WindowBank, SigmoidLoss.  Single process; the labelled loss also on two ranks (mask mode).
LABELLED = {"clip-labels-positive": "positive", "clip-labels-mask": "mask"}
NEW_LOSSES = [*LABELLED, "clip-negatives", "sigmoid"]
DP_LOSSES = LOSSES + ["clip-labels-mask"]
REPEAT = (1, B // 2 - 1)      # the repeated speech segment of the labelled kinds: both samples in rank 0's shard of two
NEG_N, NEG_ROWS = 40, 120     # the negatives: 40 windows of a 120-row track
SIG_TEMP, SIG_BIAS = math.log(10.0), -10.0          # SigmoidLoss's initial values


def problem():
    return toy_problem(TOY, B)


def labels_of(kind):
    """the speech ids of a batch of a labelled kind: samples REPEAT carry one segment (None: the kind takes no labels)"""
    if kind not in LABELLED:
        return None
    lab = np.arange(B, dtype=np.int64) + 100
    lab[REPEAT[1]] = lab[REPEAT[0]]
    return lab


def batch_of(kind, X, Y, subj):
    """the batch as `kind` sees it: a labelled kind's second REPEAT sample hears the first one's speech"""
    if kind in LABELLED:
        Y = Y.clone()
        Y[REPEAT[1]] = Y[REPEAT[0]]
    return X, Y, subj


def negatives_track():
    """(F, NEG_ROWS) values of the negatives' track, fp16-exact, and the window starts"""
    from tests import clip_negative_cases as NC
    g = torch.Generator().manual_seed(77)
    E = (3.0 * torch.randn(TOY["F"], NEG_ROWS, generator=g) * torch.exp(0.5 * torch.randn(1, NEG_ROWS, generator=g))).half()
    return E, NC.starts_of(NEG_N, NEG_ROWS, TOY["T"], "edges")


def negatives_bank():
    from speech_decoding_amd.retrieval import WindowBank
    E, starts = negatives_track()
    bank = WindowBank(TOY["F"], TOY["T"], dtype=torch.float16, device=DEV)
    bank.add_track(E.to(DEV), np.asarray(starts))
    return bank


def double(P):
    return {k: (v.to(torch.complex128) if v.is_complex() else v.double() if v.is_floating_point() else v) for k, v in P.items()}


def pow2_at_least(x):
    return 2.0 ** math.ceil(math.log2(x))


def oracle_Z(loc, P, X, subj):
    """the float64 oracle's embeddings of a training-mode forward"""
    return O.brain_encoder_forward(double(P), X.double(), subj, training=True, loc=loc, drop_centre=CENTRE).detach()


def oracle_dZ(kind, Y, Z):
    """dL/dZ of the float64 oracle at loss scale 1: (B, F, T).  The later losses: loss_ref_embeddings of the kind's own case
    module (float64 autograd of the loss's two-line form), never the code under test"""
    if kind in LABELLED:
        from tests import clip_label_cases as LC
        return LC.loss_ref_embeddings(Y, Z, TEMP, labels_of(kind), LABELLED[kind])[2]
    if kind == "clip-negatives":
        from tests import clip_negative_cases as NC
        E, starts = negatives_track()
        w = torch.stack([E.float()[:, int(s): int(s) + TOY["T"]] for s in starts])
        return NC.loss_ref_embeddings(Y, Z, w, TEMP)[2]
    if kind == "sigmoid":
        from tests import sigmoid_loss_cases as SG
        return SG.loss_ref_embeddings(Y, Z, SIG_TEMP, SIG_BIAS, None, "positive")["dy"]
    Z = Z.clone().requires_grad_(True)
    if kind == "clip":
        loss, _ = O.clip_loss(Y.double(), Z, torch.tensor([TEMP], dtype=torch.float64))
    else:
        loss = ((Y.double() - Z) ** 2).sum(dim=(1, 2)).mean()
    (dZ,) = torch.autograd.grad(loss, [Z])
    return dZ


def overflow_scale(dZ):
    return pow2_at_least(MARGIN * FP16_MAX / float(dZ.abs().max()))


def build(kind, P, loc):
    from speech_decoding.utils.loss import CLIPLoss, MSELoss
    from tests.builders import Config
    enc = build_encoder(P, encoder_args(TOY, loc, "fp16"), DEV)
    enc.set_drop_centre(CENTRE)
    if kind in LABELLED:
        lossf = CLIPLoss(Config(reduction="mean", init_temperature=TEMP, clip_duplicates=LABELLED[kind])).to(DEV)
    elif kind == "sigmoid":
        from speech_decoding_amd.loss import SigmoidLoss
        lossf = SigmoidLoss(Config(reduction="mean", sigmoid_init_temperature=SIG_TEMP, sigmoid_init_bias=SIG_BIAS)).to(DEV)
    else:
        lossf = clip_loss(TEMP, DEV) if kind.startswith("clip") else MSELoss().to(DEV)
    lossf.train()
    return enc, lossf


class Run:
    """encoder + loss + Adam + scaler + train.py's step, as train.run() wires them"""

    def __init__(self, kind, P, loc, world=1, scale=None):
        import train
        from speech_decoding_amd.amp import DEFAULT_FP16_SCALE, LossScaler
        from speech_decoding_amd.optim import FusedAdam
        self.enc, self.lossf = build(kind, P, loc)
        self.labels = labels_of(kind)                 # of the whole batch; a rank hands its shard's over
        self.negatives = negatives_bank() if kind == "clip-negatives" else None
        self.params = list(self.enc.parameters()) + list(self.lossf.parameters())
        self.opt = FusedAdam(self.params, lr=1e-3)
        self.scaler = LossScaler(DEFAULT_FP16_SCALE if scale is None else scale, enabled=True)
        self.oks = []                 # what every unscale_() of the step returned, in order
        unscale = self.scaler.unscale_
        self.scaler.unscale_ = lambda params, check=False: self.oks.append(unscale(params, check=check)) or self.oks[-1]
        self.step = train.make_backward_and_step(self.enc, self.lossf, self.params, self.opt, self.scaler, world, torch.device(DEV))

    def forward(self, X, Y, subj, rows=slice(None)):
        Z = self.enc(X.to(DEV), subj)
        kw = {}
        if self.labels is not None:
            kw["labels"] = self.labels[rows]
        if self.negatives is not None:
            kw["negatives"] = self.negatives
        return self.lossf(Y.to(DEV), Z, **kw)

    def train_step(self, X, Y, subj, rows=slice(None)):
        loss = self.forward(X, Y, subj, rows)
        self.step(loss)
        return float(loss.detach())

    def state(self):
        """every parameter (the temperature included), every Adam moment and step count, as host copies"""
        torch.cuda.synchronize()
        real = lambda t: (torch.view_as_real(t) if t.is_complex() else t).detach().cpu().clone()
        out = {}
        for i, p in enumerate(self.params):
            out[f"param {i}"] = real(p)
            st = self.opt.state.get(p, {})
            out[f"step {i}"] = torch.tensor(int(st.get("step", 0)))
            for k in ("exp_avg", "exp_avg_sq"):
                if k in st:
                    out[f"{k} {i}"] = real(st[k])
        return out

    def bn_state(self):
        torch.cuda.synchronize()
        return {k: v.detach().cpu().clone() for k, v in self.enc.state_dict().items()
                if k.endswith(("running_mean", "running_var", "num_batches_tracked"))}


def same_bits(a, b):
    assert a.keys() == b.keys(), sorted(set(a) ^ set(b))
    bad = [k for k in a if a[k].dtype != b[k].dtype or a[k].shape != b[k].shape
           or not torch.equal(a[k].reshape(-1).contiguous().view(torch.uint8), b[k].reshape(-1).contiguous().view(torch.uint8))]
    return bad


@pytest.mark.parametrize("kind", LOSSES + NEW_LOSSES)
def test_backward_overflow_skips_the_step_and_leaves_no_trace(kind):
    from speech_decoding_amd.amp import DEFAULT_FP16_SCALE
    loc, P, X, Y, subj = problem()
    X, Y, subj = batch_of(kind, X, Y, subj)
    dZ = oracle_dZ(kind, Y, oracle_Z(loc, P, X, subj))
    s = overflow_scale(dZ)
    print(f"{kind}: oracle max |dL/dZ| {float(dZ.abs().max()):.4e}, overflow scale 2^{int(math.log2(s))}")
    assert s * float(dZ.abs().max()) >= MARGIN * FP16_MAX > 0.5 * s * float(dZ.abs().max()) and s > DEFAULT_FP16_SCALE
    X2, Y2, subj2 = O.synthetic_batch(B, TOY["C"], TOY["T"], TOY["F"], TOY["S"], seed=5)
    X2, Y2, subj2 = batch_of(kind, X2, Y2, subj2)
    run, twin = Run(kind, P, loc), Run(kind, P, loc)
    # a healthy step first: Adam's moments exist, and the two runs start from the same bits
    for r in (run, twin):
        r.train_step(X2, Y2, subj2)
        assert r.oks == [True] and r.scaler.skipped_steps == 0 and r.scaler.scale_value == DEFAULT_FP16_SCALE, "a false alarm at the default scale"
    before = run.state()
    assert same_bits(before, twin.state()) == [] and all(int(v) == 1 for k, v in before.items() if k.startswith("step"))
    # the overflowing step
    run.scaler.scale_value = s
    loss = run.train_step(X, Y, subj)
    assert math.isfinite(loss), "the forward does not depend on the loss scale"
    assert run.oks == [True, False], run.oks                    # unscale_(check=True) itself returned False
    assert run.scaler.skipped_steps == 1 and run.scaler.scale_value == s / 2, (run.scaler.skipped_steps, run.scaler.scale_value)
    assert same_bits(run.state(), before) == [], "a skipped step moved a parameter, a moment or a step count"
    # the forward moved the running statistics as it does in any step; the overflowing backward did not touch them
    float(twin.forward(X, Y, subj).detach())
    assert same_bits(run.bn_state(), twin.bn_state()) == []
    # back at the default scale the next step is taken and equals the twin's, which never saw the overflow
    run.scaler.scale_value = DEFAULT_FP16_SCALE
    X3, Y3, subj3 = O.synthetic_batch(B, TOY["C"], TOY["T"], TOY["F"], TOY["S"], seed=7)
    X3, Y3, subj3 = batch_of(kind, X3, Y3, subj3)
    for r in (run, twin):
        r.train_step(X3, Y3, subj3)
    assert run.oks == [True, False, True] and twin.oks == [True, True]
    assert run.scaler.skipped_steps == 1 and twin.scaler.skipped_steps == 0
    after = run.state()
    assert all(int(v) == 2 for k, v in after.items() if k.startswith("step"))
    assert same_bits(after, twin.state()) == [], "the skipped step left a trace in a parameter or a moment"
    assert same_bits(after, before) != []
    assert same_bits(run.bn_state(), twin.bn_state()) == []


def pre_batchnorm_activation(loc, P, X, subj):
    """the first ConvBlock's conv0 output: the last tensor in front of the first BatchNorm, which the encoder stores in fp16 for
    that BatchNorm's statistics.  Everything up to it scales with the input; nothing behind the BatchNorm does."""
    Q = double(P)
    h = O.subject_block(Q, X.double(), subj, O.dropout_mask(loc, CENTRE, 0.1))
    d0 = O.block_dilations(0)[0]
    return TF.conv1d(h, Q["conv_blocks.conv0.conv0.weight"], Q["conv_blocks.conv0.conv0.bias"], padding=d0, dilation=d0)


@pytest.mark.parametrize("kind", LOSSES + NEW_LOSSES)
def test_forward_overflow_skips_the_step(kind):
    """the input scaled until a stored fp16 activation passes 65504 by the margin of 4: the loss is non-finite, the step is skipped,
    parameters and moments stay.  (The running statistics have moved, as under torch.cuda.amp; train.py says so, and nothing is
    asserted on them.)"""
    from speech_decoding_amd.amp import DEFAULT_FP16_SCALE
    loc, P, X, Y, subj = problem()
    X, Y, subj = batch_of(kind, X, Y, subj)
    a = float(pre_batchnorm_activation(loc, P, X, subj).abs().max())
    f = pow2_at_least(MARGIN * FP16_MAX / a)
    big = float(pre_batchnorm_activation(loc, P, X * f, subj).abs().max())
    print(f"{kind}: oracle max |activation in front of the first BatchNorm| {a:.4e}, input factor 2^{int(math.log2(f))}, then {big:.4e}")
    assert big >= 0.5 * MARGIN * FP16_MAX                       # (the bias does not scale: within a factor of two of f a)
    run = Run(kind, P, loc)
    X2, Y2, subj2 = O.synthetic_batch(B, TOY["C"], TOY["T"], TOY["F"], TOY["S"], seed=5)
    X2, Y2, subj2 = batch_of(kind, X2, Y2, subj2)
    run.train_step(X2, Y2, subj2)
    before = run.state()
    loss = run.train_step(X * f, Y, subj)
    assert not math.isfinite(loss)
    assert run.oks == [True, False], run.oks
    assert run.scaler.skipped_steps == 1 and run.scaler.scale_value == DEFAULT_FP16_SCALE / 2
    assert same_bits(run.state(), before) == []


# ---------------------------------------------------------------------------------------------------------------
# data parallel: two gloo ranks on one device; only rank 0's shard carries the sample that overflows
# ---------------------------------------------------------------------------------------------------------------
def dp_problem(kind):
    """(X, Y, subj, scale, per-sample max |dL/dZ| x scale).  MSE: sample 0's target is scaled until its own dL/dZ overflows at the
    DEFAULT scale; every other sample's gradient is as healthy as ever.  CLIP (whose dZ couples the ranks through the global
    negatives): rank 1's speech rows are its own brain embeddings, which leaves its dL/dZ an order of magnitude below rank
    0's; the scale is the oracle's overflow scale of the whole batch, and rank 1's dL/dZ stays inside fp16 at it."""
    from speech_decoding_amd.amp import DEFAULT_FP16_SCALE
    loc, P, X, Y, subj = problem()
    X, Y, subj = batch_of(kind, X, Y, subj)
    Z = oracle_Z(loc, P, X, subj)
    Y = Y.clone()
    if kind == "mse":
        g0 = float(oracle_dZ(kind, Y, Z)[0].abs().max())
        k = pow2_at_least(2 * MARGIN * FP16_MAX / (DEFAULT_FP16_SCALE * g0))      # dL/dZ[0] = 2 (Z[0] - k Y[0]) / B grows with k
        Y[0] *= k
        scale = DEFAULT_FP16_SCALE
    else:
        Y[B // 2:] = Z[B // 2:].float()
        scale = overflow_scale(oracle_dZ(kind, Y, Z))
    per_sample = scale * oracle_dZ(kind, Y, Z).abs().amax(dim=(1, 2))
    return loc, P, X, Y, subj, scale, per_sample


@pytest.mark.parametrize("kind", DP_LOSSES)
def test_dp_problem_overflows_on_rank_0_only(kind):
    """the oracle's word on the data-parallel cases (no GPU work): scaled dL/dZ passes 4 x 65504 in rank 0's shard and stays
    inside fp16, with the fp16 path's error to spare, in every sample of rank 1's"""
    *_, Y, _, scale, per_sample = dp_problem(kind)
    print(f"{kind}: scale 2^{int(math.log2(scale))}, scaled max |dL/dZ| per sample {[f'{float(v):.3e}' for v in per_sample]}")
    assert float(per_sample[:B // 2].max()) >= MARGIN * FP16_MAX
    assert float(per_sample[B // 2:].max()) * 1.1 < FP16_MAX
    assert float(Y.abs().max()) < FP16_MAX


DP_CASES = [(kind, overlap) for kind in DP_LOSSES for overlap in (True, False)]       # overlap: the engine's own reduction inside backward


def _worker(rank, world, dev):
    from speech_decoding_amd.distributed import shard_range
    problems = {kind: dp_problem(kind) for kind in DP_LOSSES}
    lo, hi = shard_range(B, rank, world)
    res = {}
    for kind, overlap in DP_CASES:
        loc, P, X, Y, subj, scale, _ = problems[kind]
        run = Run(kind, P, loc, world=world, scale=scale)
        run.enc.engine.overlap_grad_allreduce = overlap
        assert run.enc.grads_are_reduced == overlap
        before = run.state()
        loss = run.train_step(X[lo:hi], Y[lo:hi], subj[lo:hi], rows=slice(lo, hi))
        after = run.state()
        res[(kind, overlap)] = dict(ok=run.oks, scale=run.scaler.scale_value, skipped=run.scaler.skipped_steps, loss=loss, start_scale=scale,
                                     moved=same_bits(after, before), params={k: v for k, v in after.items() if k.startswith("param")})
    return res


@pytest.fixture(scope="module")
def two_ranks():
    """one pair of processes (the worker and spawn pattern of tests/test_dp_gpu.py) steps every case of DP_CASES once"""
    return run_ranks(_worker, 2)


@pytest.mark.parametrize("kind,overlap", DP_CASES, ids=[f"{k}-{'engine-reduction' if o else 'allreduce_gradients'}" for k, o in DP_CASES])
def test_two_ranks_skip_the_same_step(two_ranks, kind, overlap):
    """train.py: "SUM of the still-scaled gradients: every rank then sees the same overflow, or none".  If one rank skipped and
    the other stepped, the replicas would diverge and nothing would report it.  Both gradient paths: the engine's own reduction
    inside backward (grads_are_reduced) and allreduce_gradients after it."""
    out = [two_ranks[r][(kind, overlap)] for r in range(2)]
    for r in range(2):
        assert out[r]["ok"] == [False], (r, out[r]["ok"])
        assert out[r]["skipped"] == 1 and out[r]["scale"] == out[r]["start_scale"] / 2, (r, out[r]["scale"])
        assert out[r]["moved"] == [], (r, "a skipped step moved", out[r]["moved"])
    assert out[0]["scale"] == out[1]["scale"]
    assert same_bits(out[0]["params"], out[1]["params"]) == []
