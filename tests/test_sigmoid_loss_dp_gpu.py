"""SigmoidLoss under data parallelism on ONE MI355X: two ranks (gloo rendezvous, both on cuda:0, a fresh process each) hold the two
halves of a batch.  Every rank reports the global loss; the concatenated dZ and dY rows and the summed shares of dtemp and dbias
equal one process on the global batch; each rank's result is the same bits run to run; and the forward never merges row statistics
across ranks — a rank's block of pairs is complete on its own."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from speech_decoding_amd import SigmoidLoss  # noqa: F401,E402  (the feature under test: without it this file does not import)
from tests.ranks import run_ranks          # noqa: E402

B_RANK, F, T = 6, 64, 70
TEMP, BIAS = 2.0, -3.0


def sigmoid(dev, duplicates):
    from speech_decoding.utils.loss import SigmoidLoss
    from tests.builders import Config
    return SigmoidLoss(Config(reduction="mean", sigmoid_init_temperature=TEMP, sigmoid_init_bias=BIAS, clip_duplicates=duplicates)).to(dev)


def global_labels(Bg):
    """a pair inside rank 0, a pair across the two ranks, a class of three across them"""
    lab = np.arange(Bg, dtype=np.int64) + 50
    lab[[1, 4]] = 7
    lab[[2, Bg - 1]] = 8
    lab[[0, B_RANK, B_RANK + 2]] = 9
    return lab


def _worker(rank, world, dev, labelled, duplicates):
    from speech_decoding_amd import distributed
    from speech_decoding_amd.distributed import shard_range
    from tests import sigmoid_loss_cases as SC

    def refuse(*a, **k):
        raise AssertionError("SigmoidLoss merged row statistics across ranks")

    distributed.merge_row_softmax_stats = refuse
    Bg = B_RANK * world
    g = torch.Generator().manual_seed(77)
    Yf, Zf = torch.randn(Bg, F, T, generator=g), torch.randn(Bg, F, T, generator=g)
    Zf = Zf + 0.5 * Yf
    lab = global_labels(Bg) if labelled else None
    lo, hi = shard_range(Bg, rank, world)
    res = {}
    for name, dtype in (("fp32", torch.float32), ("bf16", torch.bfloat16)):
        runs = []
        crit = sigmoid(dev, duplicates)
        for _ in range(2):
            x = Yf[lo:hi].to(dtype).to(dev).requires_grad_(True)
            y = Zf[lo:hi].to(dtype).to(dev).requires_grad_(True)
            loss = crit(x, y, labels=None if lab is None else lab[lo:hi])
            dx, dy, dt, db = torch.autograd.grad(loss, [x, y, crit.temp, crit.bias])
            runs.append(dict(loss=float(loss.detach()), dx=dx.float().cpu(), dy=dy.float().cpu(), dt=dt.cpu(), db=db.cpu()))
        res[name] = runs
        if rank == 0:      # single-process reference on the whole batch, collectives switched off
            crit1 = sigmoid(dev, duplicates)
            crit1.global_negatives = False
            x1 = Yf.to(dtype).to(dev).requires_grad_(True)
            y1 = Zf.to(dtype).to(dev).requires_grad_(True)
            logits, l1 = crit1(x1, y1, return_logits=True, labels=lab)
            dx1, dy1, dt1, db1 = torch.autograd.grad(l1, [x1, y1, crit1.temp, crit1.bias])
            lg = logits.double().cpu().requires_grad_(True)
            (D,) = torch.autograd.grad(SC.loss_ref(lg, None if lab is None else torch.from_numpy(lab), duplicates), [lg])
            res[name + "/ref"] = dict(loss=float(l1.detach()), dx=dx1.float().cpu(), dy=dy1.float().cpu(), dt=float(dt1), db=float(db1),
                                      abs_Da=float((D * (lg.detach() - BIAS)).abs().sum()), abs_D=float(D.abs().sum()))
    return res


@pytest.mark.parametrize("labelled,duplicates", [(False, "positive"), (True, "positive"), (True, "mask")],
                         ids=["unlabelled", "labels-positive", "labels-mask"])
def test_two_ranks_match_one_process_on_the_global_batch(labelled, duplicates):
    world = 2
    out = run_ranks(_worker, world, labelled, duplicates)
    for name, tol in (("fp32", 1e-5), ("bf16", 2e-2)):          # the bounds of tests/test_clip_dy_dp_gpu.py
        ref = out[0][name + "/ref"]
        for r in range(world):
            a, b = out[r][name]
            for k in ("dx", "dy", "dt", "db"):
                assert torch.equal(a[k], b[k]), (name, r, k)                  # the same bits run to run
            assert abs(a["loss"] - ref["loss"]) <= 1e-5 * abs(ref["loss"])    # every rank reports the global loss
        for key in ("dx", "dy"):
            got = torch.cat([out[r][name][0][key] for r in range(world)])
            want = ref[key]
            err = float((got - want).abs().max()) if name == "fp32" else float((got - want).norm() / want.norm())
            lim = tol * float(want.abs().max()) if name == "fp32" else tol
            print(name, key, err, lim)
            assert err <= lim, (name, key, err, lim)
        # the scalar gradients are fp32 sums of D a and D in every dtype: the ranks' shares add up to the one process's
        for key, scale in (("dt", "abs_Da"), ("db", "abs_D")):
            got = sum(float(out[r][name][0][key]) for r in range(world))
            print(name, key, got, ref[key], ref[scale])
            assert abs(got - ref[key]) <= 1e-5 * ref[scale], (name, key, got, ref[key])
