"""X's gradient through BrainEncoder under data parallelism on ONE MI355X: two ranks (gloo rendezvous, both on cuda:0, a fresh
process each) hold the two halves of a batch with synchronised BatchNorm; the concatenated per-rank dX equals one process on
the global batch, is the same bits run to run, and a frozen encoder (the data-gradient-only backward) completes as well."""
import datetime
import os
import socket

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
                root_dir=".", preprocs={"last4layers": False}, sensor_positions=loc.numpy(), compute_dtype="fp32")
    enc = BrainEncoder(args)
    enc.load_state_dict(P)
    return enc.to(dev).train()


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
        res = {"rows": (lo, hi)}
        for mode in ("train", "eval"):
            enc = build(P, d, dev)
            enc.train(mode == "train")
            crit = MSELoss()
            runs = [dx_of(enc, crit, X[lo:hi], Y[lo:hi], subj[lo:hi], dev) for _ in range(2)]
            runs.append(dx_of(enc, crit, X[lo:hi], Y[lo:hi], subj[lo:hi], dev, frozen=True))
            res[mode] = runs
            if rank == 0:      # single-process reference on the whole batch, collectives switched off
                enc1 = build(P, d, dev)
                enc1.train(mode == "train")
                enc1.sync_batchnorm = False
                crit1 = MSELoss()
                crit1.global_batch = False
                res[mode + "/ref"] = dx_of(enc1, crit1, X, Y, subj, dev)
        ret[rank] = res
    finally:
        dist.destroy_process_group()


def test_two_ranks_dx_matches_one_process_on_the_global_batch():
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
    for mode in ("train", "eval"):
        ref = out[0][mode + "/ref"]
        for r in range(world):
            a, b, frozen = out[r][mode]
            assert torch.equal(a, b), (mode, r)                 # the same bits run to run
            assert torch.equal(a, frozen), (mode, r)            # the frozen encoder's data-gradient-only backward: the same dX
        got = torch.cat([out[r][mode][0] for r in range(world)])
        err = float((got - ref).abs().max())
        assert err <= 1e-3 * float(ref.abs().max()), (mode, err, float(ref.abs().max()))
