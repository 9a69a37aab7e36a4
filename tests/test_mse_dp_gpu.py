"""MSELoss under data parallelism on ONE MI355X: two ranks (gloo rendezvous, both on cuda:0, a fresh process each) train on the
two halves of a batch; every rank reports the global loss and the summed gradients equal one process on the whole batch."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from tests.builders import TOY as TOY_DIMS, build_encoder, grads_of, null_bias_grad, toy_problem      # noqa: E402
from tests.ranks import run_ranks                                                                  # noqa: E402

TOY = dict(TOY_DIMS, B=6)       # per rank


def _worker(rank, world, dev, d):
    from speech_decoding.utils.loss import MSELoss
    from speech_decoding_amd.distributed import shard_range
    Bg = d["B"] * world
    _, P, X, Y, subj = toy_problem(d, Bg)
    lo, hi = shard_range(Bg, rank, world)
    enc = build_encoder(P, d, dev)
    enc.set_drop_centre(4)
    crit = MSELoss()
    Z = enc(X[lo:hi].to(dev), subj[lo:hi])
    loss = crit(Y[lo:hi].to(dev), Z)
    loss.backward()
    assert enc.grads_are_reduced                     # encoder gradients: summed over the ranks inside backward
    # the loss alone on fixed operands: this rank's dZ is its rows of the single-process dZ on the global batch
    g = torch.Generator().manual_seed(9)
    Zf = torch.randn(Bg, d["F"], d["T"], generator=g)
    Zl = Zf[lo:hi].to(dev).requires_grad_(True)
    lz = crit(Y[lo:hi].to(dev), Zl)
    (dZl,) = torch.autograd.grad(lz, [Zl])
    res = dict(loss=float(loss.detach()), grads=grads_of(enc), lz=float(lz), dZl=dZl.cpu())
    if rank == 0:      # single-process reference on the whole batch, collectives switched off
        enc1 = build_encoder(P, d, dev)
        enc1.sync_batchnorm = False
        enc1.set_drop_centre(4)
        crit1 = MSELoss()
        crit1.global_batch = False
        l1 = crit1(Y.to(dev), enc1(X.to(dev), subj))
        l1.backward()
        Z1 = Zf.to(dev).requires_grad_(True)
        lz1 = crit1(Y.to(dev), Z1)
        (dZ1,) = torch.autograd.grad(lz1, [Z1])
        res["ref"] = dict(loss=float(l1.detach()), grads=grads_of(enc1), lz=float(lz1), dZ=dZ1.cpu())
    return res


def test_two_ranks_match_one_process_on_the_global_batch():
    world, d = 2, TOY
    out = run_ranks(_worker, world, d)
    ref = out[0]["ref"]
    B = d["B"]
    for r in range(world):
        assert abs(out[r]["loss"] - ref["loss"]) <= 1e-5 * ref["loss"]           # every rank reports the global loss
        assert abs(out[r]["lz"] - ref["lz"]) <= 1e-6 * ref["lz"]
        assert torch.equal(out[r]["dZl"], ref["dZ"][r * B:(r + 1) * B])          # the local share: exactly the same gradient
        for k, g in out[r]["grads"].items():
            gr = ref["grads"][k]
            if null_bias_grad(k):
                continue                                                           # zero up to rounding noise
            assert float((g - gr).abs().max()) <= 2e-3 * float(gr.abs().max()) + 1e-7, (r, k)
    np.testing.assert_array_equal(out[0]["dZl"].shape, (B, d["F"], d["T"]))
