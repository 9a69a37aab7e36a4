"""Data-parallel correctness on ONE MI355X: two ranks (gloo rendezvous, both on cuda:0) each train on half
of a batch with synchronised BatchNorm statistics, all-gathered speech embeddings (global negatives) and a
SUM gradient all-reduce; loss, embeddings and gradients must equal the single-process run on the whole
batch.  (The 8-GPU RCCL run is the driver's; this covers the algebra and the collective call sequence.)"""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from oracle import brain_oracle as O      # noqa: E402
from tests import builders as TB          # noqa: E402
from tests.ranks import run_ranks          # noqa: E402

TOY = dict(TB.TOY, B=12)
# BASELINE configs[2] / configs[3] per-rank shapes (Gwilliams 208 ch x 27 subjects, Brennan 60 ch x 1 subject) at the
# real layer widths, 12 segments per rank (the Classifier needs 10 candidates): SyncBN + global negatives + per-group gradient all-reduce at full dims
REAL_208 = dict(C=208, S=27, D1=270, D2=320, F=1024, K=32, T=360, B=12)
REAL_60 = dict(C=60, S=1, D1=270, D2=320, F=1024, K=32, T=360, B=12)


def build(dtype, P, d, dev="cuda:0"):
    loc = O.synthetic_positions(d["C"], seed=1)
    return TB.build_encoder(P, TB.encoder_args(d, loc, dtype), dev), TB.clip_loss(3.0, dev)


def _worker(rank, world, DEV, d):
    from speech_decoding_amd.distributed import allreduce_gradients, shard_range
    Bg = d["B"] * world
    _, P, X, Y, subj = TB.toy_problem(d, Bg)
    lo, hi = shard_range(Bg, rank, world)
    enc, lossf = build("fp32", P, d, DEV)
    enc.set_drop_centre(4)
    Yl = Y[lo:hi].to(DEV)
    lossf.prefetch(Yl, torch.float32)                          # async all-gather of Y overlapping the encoder
    Z = enc(X[lo:hi].to(DEV), subj[lo:hi])
    loss = lossf(Yl, Z)
    loss.backward()
    assert enc.grads_are_reduced                                  # encoder grads: all-reduced inside backward
    allreduce_gradients(list(lossf.parameters()))
    from speech_decoding.models import Classifier
    top = Classifier(None)(Z, Yl)                              # served from the loss's global ranks
    top_again = Classifier(None)(Z, Yl.clone())                # uncached path: gathers and ranks globally
    assert top == top_again
    res = dict(loss=float(loss.detach()), Z=Z.detach().float().cpu(), grads=TB.grads_of(enc, ("temp", lossf.temp)), top=top,
               rm=enc.conv_blocks.conv2.batchnorm1.running_mean.cpu().clone())
    if rank == 0:      # single-process reference on the whole batch, collectives switched off
        enc1, lossf1 = build("fp32", P, d, DEV)
        enc1.sync_batchnorm = False
        lossf1.global_negatives = False
        enc1.set_drop_centre(4)
        Z1 = enc1(X.to(DEV), subj)
        l1 = lossf1(Y.to(DEV), Z1)
        l1.backward()
        local_clf = Classifier(None)
        local_clf.global_candidates = False
        res["ref"] = dict(loss=float(l1.detach()), Z=Z1.detach().float().cpu(), grads=TB.grads_of(enc1, ("temp", lossf1.temp)),
                          rm=enc1.conv_blocks.conv2.batchnorm1.running_mean.cpu().clone(),
                          top=local_clf(Z1, Y.to(DEV)))
    return res


@pytest.mark.parametrize("world,dims", [(2, TOY), (4, TOY), (2, REAL_208), (2, REAL_60)],
                         ids=["toy-2", "toy-4", "config3-dims-2", "config4-dims-2"])
def test_ranks_match_single_process_global_batch(world, dims):
    _run_ranks(world, dims, "gloo")


def test_two_ranks_on_rccl_when_two_gpus_are_visible():
    """The same check over the real backend: torch.distributed "nccl" = RCCL over xGMI, one device per rank.  Needs two
    GPUs (the driver's multi-GPU box); on the one-GPU test box the RCCL call sequence is covered at world size 1 by
    tests/test_rccl_gpu.py."""
    if torch.cuda.device_count() < 2:
        pytest.skip("needs two GPUs")
    _run_ranks(2, TOY, "nccl")
    _run_ranks(2, REAL_208, "nccl")


def _run_ranks(world, dims, backend):
    out = run_ranks(_worker, world, dims, backend=backend)
    ref = out[0]["ref"]
    B = dims["B"]
    for r in range(world):
        assert abs(out[r]["loss"] - ref["loss"]) < 2e-5                       # every rank reports the global loss
        np.testing.assert_allclose(out[r]["Z"].numpy(), ref["Z"][r * B:(r + 1) * B].numpy(), rtol=2e-4, atol=2e-5)
        np.testing.assert_allclose(out[r]["rm"].numpy(), ref["rm"].numpy(), rtol=1e-4, atol=1e-6)
        for k, g in out[r]["grads"].items():
            gr = ref["grads"][k]
            scale = float(gr.abs().max()) + 1e-12
            if TB.null_bias_grad(k):
                continue
            assert float((g - gr).abs().max()) <= 2e-3 * scale + 1e-7, (r, k)
    # retrieval accuracy over the global batch = mean of the per-rank accuracies
    top1 = np.mean([out[r]["top"][0] for r in range(world)])
    top10 = np.mean([out[r]["top"][1] for r in range(world)])
    assert (top1, top10) == pytest.approx(ref["top"])
