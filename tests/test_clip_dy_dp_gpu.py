"""CLIPLoss's speech-side gradient under data parallelism on ONE MI355X: two ranks (gloo rendezvous, both on cuda:0, a fresh
process each) hold the two halves of a batch; the concatenated dY rows and dZ rows equal one process on the global batch, and
each rank's result is the same bits run to run."""
import pytest
import torch

pytestmark = pytest.mark.gpu

from tests.builders import clip_loss      # noqa: E402
from tests.ranks import run_ranks          # noqa: E402

B_RANK, F, T = 6, 64, 70


def _worker(rank, world, dev):
    from speech_decoding_amd.distributed import shard_range
    Bg = B_RANK * world
    g = torch.Generator().manual_seed(77)
    Yf, Zf = torch.randn(Bg, F, T, generator=g), torch.randn(Bg, F, T, generator=g)
    lo, hi = shard_range(Bg, rank, world)
    res = {}
    for name, dtype in (("fp32", torch.float32), ("bf16", torch.bfloat16)):
        runs = []
        crit = clip_loss(2.0, dev)
        for _ in range(2):
            x = Yf[lo:hi].to(dtype).to(dev).requires_grad_(True)
            y = Zf[lo:hi].to(dtype).to(dev).requires_grad_(True)
            loss = crit(x, y)
            dx, dy, dt = torch.autograd.grad(loss, [x, y, crit.temp])
            runs.append(dict(loss=float(loss), dx=dx.float().cpu(), dy=dy.float().cpu(), dt=dt.cpu()))
        res[name] = runs
        if rank == 0:      # single-process reference on the whole batch, collectives switched off
            crit1 = clip_loss(2.0, dev)
            crit1.global_negatives = False
            x1 = Yf.to(dtype).to(dev).requires_grad_(True)
            y1 = Zf.to(dtype).to(dev).requires_grad_(True)
            l1 = crit1(x1, y1)
            dx1, dy1 = torch.autograd.grad(l1, [x1, y1])
            res[name + "/ref"] = dict(loss=float(l1), dx=dx1.float().cpu(), dy=dy1.float().cpu())
    return res


def test_two_ranks_dy_matches_one_process_on_the_global_batch():
    world = 2
    out = run_ranks(_worker, world)
    for name, tol in (("fp32", 1e-5), ("bf16", 2e-2)):
        ref = out[0][name + "/ref"]
        for r in range(world):
            a, b = out[r][name]
            for k in ("dx", "dy", "dt"):
                assert torch.equal(a[k], b[k]), (name, r, k)                  # the same bits run to run
            assert abs(a["loss"] - ref["loss"]) <= 1e-5 * abs(ref["loss"])    # every rank reports the global loss
        for key in ("dx", "dy"):
            got = torch.cat([out[r][name][0][key] for r in range(world)])
            want = ref[key]
            err = float((got - want).abs().max()) if name == "fp32" else float((got - want).norm() / want.norm())
            lim = tol * float(want.abs().max()) if name == "fp32" else tol
            assert err <= lim, (name, key, err, lim)
