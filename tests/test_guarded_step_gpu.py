"""train.make_guarded_step + GuardedAdam on an MI355X, on the toy problem and the oracle-derived overflow scale of
tests/test_overflow_guard_gpu.py:
  * against the host path (make_backward_and_step + FusedAdam + LossScaler(enabled=True)) with clipping off: the same skip
    decisions and scale trajectory, and after every step the same bits in parameters, moments and BatchNorm buffers (a
    power-of-two un-scaling is exact; entries whose un-scaled gradient is an fp32 subnormal are masked and counted);
  * clipping at half the float64 oracle's gradient norm: the logged norm within tests/test_e2e_gpu.py's gradient bound of the
    dtype, three steps within tests/test_state_reuse_gpu.py's per-step Adam limit of float64 CPU Adam + clip_grad_norm_;
  * no device read-back inside the step (the host path's read-back is seen by the same trap);
  * two data-parallel ranks, the overflow on rank 0's shard only: both skip, identical bits;
  * train.run with max_grad_norm / fp16_guard=device: the epoch row's new keys, the default row unchanged."""
import math

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from oracle import brain_oracle as O                                                 # noqa: E402
from tests.builders import TOY, build_encoder, clip_loss, encoder_args, toy_problem   # noqa: E402
from tests.ranks import run_ranks                                                     # noqa: E402
from tests.test_e2e_gpu import GRAD_REL                                               # noqa: E402

DEV = "cuda:0"
B = 12
TEMP = 3.0
CENTRE = 4
FP16_MAX = 65504.0
MARGIN = 4.0
LR = 1e-3
LOSSES = ["clip", "mse"]
DEFAULT_SCALE = 1024.0
SUBNORMAL = 2.0 ** -126


def double(P):
    return {k: (v.to(torch.complex128) if v.is_complex() else v.double() if v.is_floating_point() else v) for k, v in P.items()}


def pow2_at_least(x):
    return 2.0 ** math.ceil(math.log2(x))


def oracle_Z(loc, P, X, subj):
    return O.brain_encoder_forward(double(P), X.double(), subj, training=True, loc=loc, drop_centre=CENTRE).detach()


def oracle_dZ(kind, Y, Z):
    """dL/dZ of the float64 oracle at loss scale 1"""
    Z = Z.clone().requires_grad_(True)
    if kind == "clip":
        loss, _ = O.clip_loss(Y.double(), Z, torch.tensor([TEMP], dtype=torch.float64))
    else:
        loss = ((Y.double() - Z) ** 2).sum(dim=(1, 2)).mean()
    (dZ,) = torch.autograd.grad(loss, [Z])
    return dZ


def overflow_scale(dZ):
    """the smallest power of two that puts max |dL/dZ| two binades past fp16's range (tests/test_overflow_guard_gpu.py)"""
    return pow2_at_least(MARGIN * FP16_MAX / float(dZ.abs().max()))


class Run:
    """encoder + loss + optimiser + train.py's step on one of the two paths, as train.run() wires them"""

    def __init__(self, kind, P, loc, path, dtype="fp16", world=1, scale=DEFAULT_SCALE, max_grad_norm=None):
        import train
        from speech_decoding.utils.loss import MSELoss
        from speech_decoding_amd.amp import LossScaler
        from speech_decoding_amd.optim import FusedAdam, GuardedAdam
        self.enc = build_encoder(P, encoder_args(TOY, loc, dtype), DEV)
        self.enc.set_drop_centre(CENTRE)
        self.lossf = clip_loss(TEMP, DEV) if kind == "clip" else MSELoss().to(DEV)
        self.lossf.train()
        self.params = list(self.enc.parameters()) + list(self.lossf.parameters())
        self.path = path
        if path == "host":
            self.opt = FusedAdam(self.params, lr=LR)
            self.scaler = LossScaler(scale, enabled=True)
            self.step = train.make_backward_and_step(self.enc, self.lossf, self.params, self.opt, self.scaler, world, torch.device(DEV))
        else:
            self.opt = GuardedAdam(self.params, lr=LR, max_grad_norm=max_grad_norm, loss_scale=scale, dynamic=dtype == "fp16")
            self.step = train.make_guarded_step(self.enc, self.lossf, self.params, self.opt, world, torch.device(DEV))

    def forward(self, X, Y, subj):
        return self.lossf(Y.to(DEV), self.enc(X.to(DEV), subj))

    def train_step(self, X, Y, subj):
        self.step(self.forward(X, Y, subj))

    def set_scale(self, s):
        if self.path == "host":
            self.scaler.scale_value = s
        else:
            self.opt.set_loss_scale(s)

    def scale_and_skips(self):
        if self.path == "host":
            return self.scaler.scale_value, self.scaler.skipped_steps
        return self.opt.loss_scale, self.opt.skipped_steps

    def state(self):
        """parameters, Adam moments and BatchNorm buffers as host copies"""
        torch.cuda.synchronize()
        real = lambda t: (torch.view_as_real(t) if t.is_complex() else t).detach().cpu().clone()
        out = {}
        for i, p in enumerate(self.params):
            out[f"param {i}"] = real(p)
            for k in ("exp_avg", "exp_avg_sq"):
                if k in self.opt.state.get(p, {}):
                    out[f"{k} {i}"] = real(self.opt.state[p][k])
        for k, v in self.enc.state_dict().items():
            if k.endswith(("running_mean", "running_var", "num_batches_tracked")):
                out[k] = v.detach().cpu().clone()
        return out

    def scaled_grads(self):
        torch.cuda.synchronize()
        return [None if p.grad is None else (torch.view_as_real(p.grad) if p.grad.is_complex() else p.grad).detach().cpu().clone()
                for p in self.params]


def differing(a, b, masks=None):
    """keys whose bits differ outside the masked entries"""
    assert a.keys() == b.keys(), sorted(set(a) ^ set(b))
    bad = []
    for k in a:
        if a[k].dtype != b[k].dtype or a[k].shape != b[k].shape:
            bad.append(k)
            continue
        x, y = a[k].reshape(-1).contiguous(), b[k].reshape(-1).contiguous()
        same = x.view(torch.uint8).reshape(x.numel(), -1).eq(y.view(torch.uint8).reshape(x.numel(), -1)).all(1)
        kind, _, index = k.partition(" ")
        if masks is not None and kind in ("param", "exp_avg", "exp_avg_sq") and index in masks:
            same = same | masks[index].reshape(-1)
        if not bool(same.all()):
            bad.append(k)
    return bad


@pytest.mark.parametrize("kind", LOSSES)
def test_device_guard_equals_the_host_guard(kind):
    loc, P, X, Y, subj = toy_problem(TOY, B)
    s = overflow_scale(oracle_dZ(kind, Y, oracle_Z(loc, P, X, subj)))
    assert s > DEFAULT_SCALE
    healthy = [O.synthetic_batch(B, TOY["C"], TOY["T"], TOY["F"], TOY["S"], seed=seed) for seed in (5, 7)]
    host, dev = Run(kind, P, loc, "host"), Run(kind, P, loc, "device")
    masks = {}                      # parameter index -> entries whose un-scaled gradient was an fp32 subnormal at some step
    plan = [(DEFAULT_SCALE, healthy[0], False), (s, (X, Y, subj), True), (DEFAULT_SCALE, healthy[1], False)]
    skips = 0
    for i, (scale, batch, overflows) in enumerate(plan):
        for r in (host, dev):
            r.set_scale(scale)
            r.train_step(*batch)
        skips += overflows
        want_scale = scale / 2 if overflows else scale
        assert host.scale_and_skips() == dev.scale_and_skips() == (want_scale, skips), (i, host.scale_and_skips(), dev.scale_and_skips())
        assert dev.opt.steps_taken == i + 1 - skips
        if not overflows:
            for j, g in enumerate(dev.scaled_grads()):
                if g is not None:
                    sub = (g != 0) & (g.abs().double() / scale < SUBNORMAL)
                    masks[str(j)] = masks.get(str(j), torch.zeros_like(sub)) | sub
        masked = sum(int(m.sum()) for m in masks.values())
        print(f"{kind} step {i + 1}: scale {want_scale:g}, skipped {skips}, masked subnormal entries {masked}")
        assert masked <= 0.001 * sum(m.numel() for m in masks.values())
        assert differing(host.state(), dev.state(), masks) == [], f"step {i + 1}"
    assert math.isfinite(dev.opt.last_grad_norm) and dev.opt.last_coef == 1.0 / DEFAULT_SCALE


@pytest.mark.parametrize("dtype", ["fp16", "bf16"])
def test_clipping_follows_float64_adam_with_clip_grad_norm(dtype):
    loc, P, X, Y, subj = toy_problem(TOY, B)
    batches = [(X, Y, subj)] + [O.synthetic_batch(B, TOY["C"], TOY["T"], TOY["F"], TOY["S"], seed=seed) for seed in (5, 7)]
    stat_key = lambda k: "running" in k or "num_batches" in k           # noqa: E731
    Pd = double(P)
    leaves = {k: v.clone().requires_grad_(True) for k, v in Pd.items()
              if (v.is_floating_point() or v.is_complex()) and not stat_key(k) and not k.endswith((".cos", ".sin"))}
    otemp = torch.tensor([TEMP], dtype=torch.float64, requires_grad=True)
    oopt = torch.optim.Adam(list(leaves.values()) + [otemp], lr=LR)

    def oracle_grads(batch):
        Po = dict(Pd)
        Po.update({k: v.detach() for k, v in leaves.items()})
        Xb, Yb, sb = batch
        _, _, _, go = O.train_step(Po, otemp.detach(), Xb.double(), Yb.double(), sb, loc=loc, drop_centre=CENTRE)
        return go

    def norm_of(go):
        return math.sqrt(sum(float((torch.view_as_real(g) if g.is_complex() else g).double().pow(2).sum()) for g in go.values() if g is not None))
    max_norm = 0.5 * norm_of(oracle_grads(batches[0]))
    run = Run("clip", P, loc, "device", dtype=dtype, scale=DEFAULT_SCALE if dtype == "fp16" else 1.0, max_grad_norm=max_norm)
    for i, batch in enumerate(batches):
        go = oracle_grads(batch)
        want_norm = norm_of(go)
        for k, leaf in leaves.items():
            leaf.grad = go[k]
        otemp.grad = go["temp"]
        total = torch.nn.utils.clip_grad_norm_(list(leaves.values()) + [otemp], max_norm)
        assert abs(float(total) - want_norm) <= 1e-9 * want_norm
        oopt.step()
        run.train_step(*batch)
        got_norm, coef, scale = run.opt.last_grad_norm, run.opt.last_coef, run.opt.loss_scale
        print(f"{dtype} step {i + 1}: grad norm {got_norm:.6e} vs oracle {want_norm:.6e} ({abs(got_norm - want_norm) / want_norm:.2e} rel), "
              f"coef x scale {coef * scale:.4f}")
        assert abs(got_norm - want_norm) <= GRAD_REL[dtype] * want_norm, (i, got_norm, want_norm)
        if i == 0:
            assert coef * scale < 0.6, "clipping is not active"
        assert run.opt.skipped_steps == 0 and run.opt.steps_taken == i + 1
    lim = 2 * LR * len(batches) + 1e-6                   # tests/test_state_reuse_gpu.py: +-lr per step for a noise gradient, twice
    state = {k: v.detach().cpu() for k, v in run.enc.state_dict().items()}
    for k, leaf in leaves.items():
        got, ref = state[k], leaf.detach()
        d = float((torch.view_as_real(got).double() - torch.view_as_real(ref)).abs().max()) if got.is_complex() \
            else float((got.double() - ref).abs().max())
        assert got.shape == ref.shape and d <= lim, (k, d, lim)
    assert abs(float(run.lossf.temp.detach()) - float(otemp.detach())) <= lim


READ_BACKS = ("item", "cpu", "tolist", "numpy", "__bool__", "__float__", "__int__")


class no_device_read_back:
    """inside the block, every host read-back of a DEVICE tensor through torch.Tensor raises"""

    def __enter__(self):
        self.saved = {n: getattr(torch.Tensor, n) for n in READ_BACKS}
        for n, fn in self.saved.items():
            def trap(t, *a, _fn=fn, _n=n, **kw):
                if t.is_cuda:
                    raise RuntimeError(f"device read-back: Tensor.{_n}")
                return _fn(t, *a, **kw)
            setattr(torch.Tensor, n, trap)

    def __exit__(self, *exc):
        for n, fn in self.saved.items():
            setattr(torch.Tensor, n, fn)


def test_the_guarded_step_reads_nothing_back():
    loc, P, X, Y, subj = toy_problem(TOY, B)
    dev, host = Run("clip", P, loc, "device"), Run("clip", P, loc, "host")
    for _ in range(10):
        loss = dev.forward(X, Y, subj)
        with no_device_read_back():
            dev.step(loss)
    assert dev.opt.steps_taken == 10 and dev.opt.skipped_steps == 0
    loss = host.forward(X, Y, subj)
    with pytest.raises(RuntimeError, match="device read-back"):
        with no_device_read_back():
            host.step(loss)
    assert float(torch.ones(1, device=DEV).item()) == 1.0          # the trap is gone


# ---------------------------------------------------------------------------------------------------------------
# data parallel: two gloo ranks on one device; only rank 0's shard carries the sample that overflows
# ---------------------------------------------------------------------------------------------------------------
def dp_problem(kind):
    """tests/test_overflow_guard_gpu.py's data-parallel cases: MSE — sample 0's target scaled until its own dL/dZ overflows at
    the default scale; CLIP — rank 1's speech rows are its own brain embeddings, the scale is the oracle's overflow scale."""
    loc, P, X, Y, subj = toy_problem(TOY, B)
    Z = oracle_Z(loc, P, X, subj)
    Y = Y.clone()
    if kind == "mse":
        g0 = float(oracle_dZ(kind, Y, Z)[0].abs().max())
        Y[0] *= pow2_at_least(2 * MARGIN * FP16_MAX / (DEFAULT_SCALE * g0))
        scale = DEFAULT_SCALE
    else:
        Y[B // 2:] = Z[B // 2:].float()
        scale = overflow_scale(oracle_dZ(kind, Y, Z))
    per_sample = scale * oracle_dZ(kind, Y, Z).abs().amax(dim=(1, 2))
    assert float(per_sample[:B // 2].max()) >= MARGIN * FP16_MAX and float(per_sample[B // 2:].max()) * 1.1 < FP16_MAX
    return loc, P, X, Y, subj, scale


DP_CASES = [(kind, overlap) for kind in LOSSES for overlap in (True, False)]


def _worker(rank, world, dev):
    from speech_decoding_amd.distributed import shard_range
    lo, hi = shard_range(B, rank, world)
    res = {}
    for kind, overlap in DP_CASES:
        loc, P, X, Y, subj, scale = dp_problem(kind)
        run = Run(kind, P, loc, "device", world=world, scale=scale)
        run.enc.engine.overlap_grad_allreduce = overlap
        assert run.enc.grads_are_reduced == overlap
        before = run.state()
        run.train_step(X[lo:hi], Y[lo:hi], subj[lo:hi])
        after = run.state()
        moved = [k for k in before if not torch.equal(before[k], after[k])]
        moved += [k for k in after if k not in before and bool(after[k].any())]        # the moments made by this step are zeros
        res[(kind, overlap)] = dict(start_scale=scale, moved=moved, state=after,
                                     guard=run.opt.state_dict()["guard"].cpu().clone(), skipped=run.opt.skipped_steps,
                                     scale=run.opt.loss_scale, steps=run.opt.steps_taken)
    return res


@pytest.fixture(scope="module")
def two_ranks():
    return run_ranks(_worker, 2)


@pytest.mark.parametrize("kind,overlap", DP_CASES, ids=[f"{k}-{'engine-reduction' if o else 'allreduce_gradients'}" for k, o in DP_CASES])
def test_two_ranks_take_the_same_decision(two_ranks, kind, overlap):
    out = [two_ranks[r][(kind, overlap)] for r in range(2)]
    for r in range(2):
        assert (out[r]["skipped"], out[r]["steps"], out[r]["scale"]) == (1, 0, out[r]["start_scale"] / 2), (r, out[r]["scale"])
        moved = [k for k in out[r]["moved"] if not k.endswith(("running_mean", "running_var", "num_batches_tracked"))]
        assert moved == [], (r, "a skipped step moved", moved)
    assert differing(out[0]["state"], out[1]["state"]) == []
    assert torch.equal(out[0]["guard"].view(torch.int64), out[1]["guard"].view(torch.int64))


# ---------------------------------------------------------------------------------------------------------------
# train.run
# ---------------------------------------------------------------------------------------------------------------
DEFAULT_ROW = {"epoch", "train_loss", "test_loss", "trainTop1acc", "trainTop10acc", "testTop1acc", "testTop10acc", "lrate", "temp"}


def tiny_args(*extra):
    """the tiny shapes of tests/test_train_gpu.py"""
    from speech_decoding_amd import load_config
    args = load_config(overrides=["dataset=Gwilliams2022", "num_subjects=3", "D1=16", "D2=24", "F=32", "K=4", "batch_size=12",
                                  "epochs=2", "num_channels=12", "preprocs.last4layers=False", "preprocs.seq_len_sec=1",
                                  "preprocs.brain_resample_rate=40", "preprocs.baseline_len_sec=0.25", "lr=3e-4",
                                  "synthetic_segments=40", "updates_per_epoch=2", "split_ratio=0.7", *extra])
    args["sensor_positions"] = O.synthetic_positions(12, seed=7).numpy()
    return args


def test_train_run_on_the_guarded_path(tmp_path, monkeypatch):
    import train as T
    monkeypatch.chdir(tmp_path)
    for extra in (("max_grad_norm=1.0", "fp16_guard=device"), ("compute_dtype=fp16", "fp16_guard=device")):
        torch.manual_seed(0)
        np.random.seed(0)
        hist, _, _ = T.run(tiny_args(*extra), log=lambda *a: None)
        assert len(hist) == 2
        for row in hist:
            assert set(row) == DEFAULT_ROW | {"grad_norm", "skipped_steps"}
            assert math.isfinite(row["train_loss"]) and math.isfinite(row["grad_norm"]) and row["grad_norm"] > 0 and row["skipped_steps"] == 0
    torch.manual_seed(0)
    np.random.seed(0)
    hist, _, _ = T.run(tiny_args("epochs=1"), log=lambda *a: None)
    assert len(hist) == 1 and set(hist[0]) == DEFAULT_ROW
