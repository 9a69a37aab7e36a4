"""MSELoss under data parallelism on ONE MI355X: two ranks (gloo rendezvous, both on cuda:0, a fresh process each) train on the
two halves of a batch; every rank reports the global loss and the summed gradients equal one process on the whole batch."""
import datetime
import os
import socket

import numpy as np
import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

pytestmark = pytest.mark.gpu

from oracle import brain_oracle as O      # noqa: E402

TOY = dict(C=20, S=3, D1=32, D2=48, F=64, K=4, T=70, B=6)       # per rank


class Args(dict):
    __getattr__ = dict.__getitem__


def build(P, d, dev):
    from speech_decoding.models import BrainEncoder
    loc = O.synthetic_positions(d["C"], seed=1)
    args = Args(num_subjects=d["S"], D1=d["D1"], D2=d["D2"], F=d["F"], K=d["K"], dataset="Gwilliams2022", d_drop=0.1,
                root_dir=".", preprocs={"last4layers": False}, reduction="mean", init_temperature=3.0,
                sensor_positions=loc.numpy(), compute_dtype="fp32")
    enc = BrainEncoder(args)
    enc.load_state_dict(P)
    return enc.to(dev).train()


def grads_of(enc):
    return {n: (torch.view_as_real(p.grad) if p.grad.is_complex() else p.grad).detach().cpu().clone()
            for n, p in enc.named_parameters()}


def _worker(rank, world, port, ret, d):
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(world),
                      HSA_ENABLE_IPC_MODE_LEGACY="0")
    dev = "cuda:0"
    torch.cuda.set_device(dev)
    # short collective timeout: if one rank fails, the other errors out instead of blocking the run
    dist.init_process_group("gloo", rank=rank, world_size=world, timeout=datetime.timedelta(seconds=90))
    try:
        from speech_decoding.utils.loss import MSELoss
        from speech_decoding_amd.distributed import shard_range
        loc = O.synthetic_positions(d["C"], seed=1)
        P = O.seeded_params(d["C"], d["S"], d["D1"], d["D2"], d["F"], d["K"], seed=2, loc=loc)
        Bg = d["B"] * world
        X, Y, subj = O.synthetic_batch(Bg, d["C"], d["T"], d["F"], d["S"], seed=3)
        lo, hi = shard_range(Bg, rank, world)
        enc = build(P, d, dev)
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
            enc1 = build(P, d, dev)
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
        ret[rank] = res
    finally:
        dist.destroy_process_group()


def test_two_ranks_match_one_process_on_the_global_batch():
    world, d = 2, TOY
    ctx = mp.get_context("spawn")
    ret = ctx.Manager().dict()
    with socket.socket() as sock:
        sock.bind(("127.0.0.1", 0))
        port = sock.getsockname()[1]
    procs = [ctx.Process(target=_worker, args=(r, world, port, ret, d)) for r in range(world)]
    for p in procs:
        p.start()
    for p in procs:
        p.join(300)
    for p in procs:
        if p.is_alive():
            p.terminate()
            p.join(10)
    assert [p.exitcode for p in procs] == [0] * world
    out = dict(ret)
    ref = out[0]["ref"]
    B = d["B"]
    for r in range(world):
        assert abs(out[r]["loss"] - ref["loss"]) <= 1e-5 * ref["loss"]           # every rank reports the global loss
        assert abs(out[r]["lz"] - ref["lz"]) <= 1e-6 * ref["lz"]
        assert torch.equal(out[r]["dZl"], ref["dZ"][r * B:(r + 1) * B])          # the local share: exactly the same gradient
        for k, g in out[r]["grads"].items():
            gr = ref["grads"][k]
            if k.startswith("conv_blocks.") and k.endswith((".conv0.bias", ".conv1.bias")):
                continue                                                           # zero up to rounding noise
            assert float((g - gr).abs().max()) <= 2e-3 * float(gr.abs().max()) + 1e-7, (r, k)
    np.testing.assert_array_equal(out[0]["dZl"].shape, (B, d["F"], d["T"]))
