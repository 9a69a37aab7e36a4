"""X's gradient through BrainEncoder under data parallelism on ONE MI355X: two ranks (gloo rendezvous, both on cuda:0, a fresh
process each) hold the two halves of a batch with synchronised BatchNorm; the concatenated per-rank dX equals one process on
the global batch, is the same bits run to run, and a frozen encoder (the data-gradient-only backward) completes as well."""
import pytest
import torch

pytestmark = pytest.mark.gpu

from tests.builders import TOY as TOY_DIMS, build_encoder, toy_problem      # noqa: E402
from tests.ranks import run_ranks                                          # noqa: E402

TOY = dict(TOY_DIMS, B=6)       # per rank


def dx_of(enc, crit, X, Y, subj, dev, frozen=False):
    for p in enc.parameters():
        p.requires_grad_(not frozen)
        p.grad = None
    enc.set_drop_centre(4)
    Xl = X.to(dev).requires_grad_(True)
    loss = crit(Y.to(dev), enc(Xl, subj))
    loss.backward()
    if frozen:
        assert all(p.grad is None for p in enc.parameters())
    return Xl.grad.cpu()


def _worker(rank, world, dev, d):
    from speech_decoding.utils.loss import MSELoss
    from speech_decoding_amd.distributed import shard_range
    Bg = d["B"] * world
    _, P, X, Y, subj = toy_problem(d, Bg)
    lo, hi = shard_range(Bg, rank, world)
    res = {"rows": (lo, hi)}
    for mode in ("train", "eval"):
        enc = build_encoder(P, d, dev, training=mode == "train")
        crit = MSELoss()
        runs = [dx_of(enc, crit, X[lo:hi], Y[lo:hi], subj[lo:hi], dev) for _ in range(2)]
        runs.append(dx_of(enc, crit, X[lo:hi], Y[lo:hi], subj[lo:hi], dev, frozen=True))
        res[mode] = runs
        if rank == 0:      # single-process reference on the whole batch, collectives switched off
            enc1 = build_encoder(P, d, dev, training=mode == "train")
            enc1.sync_batchnorm = False
            crit1 = MSELoss()
            crit1.global_batch = False
            res[mode + "/ref"] = dx_of(enc1, crit1, X, Y, subj, dev)
    return res


def test_two_ranks_dx_matches_one_process_on_the_global_batch():
    world, d = 2, TOY
    out = run_ranks(_worker, world, d)
    for mode in ("train", "eval"):
        ref = out[0][mode + "/ref"]
        for r in range(world):
            a, b, frozen = out[r][mode]
            assert torch.equal(a, b), (mode, r)                 # the same bits run to run
            assert torch.equal(a, frozen), (mode, r)            # the frozen encoder's data-gradient-only backward: the same dX
        got = torch.cat([out[r][mode][0] for r in range(world)])
        err = float((got - ref).abs().max())
        assert err <= 1e-3 * float(ref.abs().max()), (mode, err, float(ref.abs().max()))
