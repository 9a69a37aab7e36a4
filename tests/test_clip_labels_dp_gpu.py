"""The labelled CLIP loss under data parallelism on ONE MI355X: two ranks (gloo rendezvous, both on cuda:0, a fresh process each)
hold the two halves of a global batch of 24 whose speech labels have classes that span both ranks and a class whose only partner
lives on the other rank.  Each rank's loss, dZ, dY and dtemp equal one process on the global batch within the project's bounds
(tests/test_clip_labels_gpu.py), the gathered class sizes equal them exactly; both modes."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from tests.ranks import run_ranks          # noqa: E402

B_RANK, F, T = 12, 64, 40
MODES = ("positive", "mask")


def global_labels(Bg):
    lab = np.arange(Bg, dtype=np.int64) + 50
    lab[[2, 5, B_RANK + 3, B_RANK + 7]] = 7          # a class of four, two on each rank
    lab[[0, B_RANK]] = 8                             # a pair whose only partner is on the other rank
    lab[[B_RANK + 1, B_RANK + 2]] = -2 ** 31         # a pair inside rank 1
    return lab


def _crit(mode, dev):
    from speech_decoding.utils.loss import CLIPLoss
    from tests.builders import Config
    return CLIPLoss(Config(reduction="mean", init_temperature=2.5, clip_duplicates=mode)).to(dev)


def _worker(rank, world, dev):
    from speech_decoding_amd import ops
    from speech_decoding_amd.distributed import shard_range
    Bg = B_RANK * world
    g = torch.Generator().manual_seed(78)
    Yf = torch.randn(Bg, F, T, generator=g)
    Zf = 0.6 * Yf + torch.randn(Bg, F, T, generator=g)
    lab = global_labels(Bg)
    lo, hi = shard_range(Bg, rank, world)
    seen = []
    real = ops.clip_label_counts
    ops.clip_label_counts = lambda labels: seen.append(real(labels)) or seen[-1]
    res = {}
    for mode in MODES:
        for name, dtype in (("fp32", torch.float32), ("bf16", torch.bfloat16)):
            crit = _crit(mode, dev)
            x = Yf[lo:hi].to(dtype).to(dev).requires_grad_(True)
            y = Zf[lo:hi].to(dtype).to(dev).requires_grad_(True)
            loss = crit(x, y, labels=lab[lo:hi])
            dx, dy, dt = torch.autograd.grad(loss, [x, y, crit.temp])
            res[mode, name] = dict(loss=float(loss), dx=dx.float().cpu(), dy=dy.float().cpu(), dt=dt.cpu(), counts=seen[-1].cpu())
            if rank == 0:      # single-process reference on the whole batch, collectives switched off
                crit1 = _crit(mode, dev)
                crit1.global_negatives = False
                x1 = Yf.to(dtype).to(dev).requires_grad_(True)
                y1 = Zf.to(dtype).to(dev).requires_grad_(True)
                l1 = crit1(x1, y1, labels=lab)
                dx1, dy1, dt1 = torch.autograd.grad(l1, [x1, y1, crit1.temp])
                res[mode, name, "ref"] = dict(loss=float(l1), dx=dx1.float().cpu(), dy=dy1.float().cpu(), dt=dt1.cpu(), counts=seen[-1].cpu())
    ops.clip_label_counts = real
    return res


def rel_l2(got, ref):
    return float((got.double() - ref.double()).norm() / ref.double().norm())


def test_two_ranks_match_one_process_on_the_global_batch():
    world = 2
    out = run_ranks(_worker, world)
    lab = torch.from_numpy(global_labels(B_RANK * world))
    want_counts = (lab[:, None] == lab[None, :]).sum(1).to(torch.int32)
    for mode in MODES:
        for name, gtol, ltol in (("fp32", 1e-5, 1e-5), ("bf16", 6e-2, 1e-2)):
            ref = out[0][mode, name, "ref"]
            assert torch.equal(ref["counts"], want_counts)
            for r in range(world):
                a = out[r][mode, name]
                assert torch.equal(a["counts"], want_counts), (mode, name, r)          # the gathered labels, in rank order
                assert abs(a["loss"] - ref["loss"]) <= ltol * abs(ref["loss"]), (mode, name, r, a["loss"], ref["loss"])
            for key in ("dx", "dy"):
                got = torch.cat([out[r][mode, name][key] for r in range(world)])
                assert rel_l2(got, ref[key]) <= gtol, (mode, name, key, rel_l2(got, ref[key]))
            if name == "fp32":                       # every rank holds its share of d loss / d temp
                dt = sum(float(out[r][mode, name]["dt"]) for r in range(world))
                assert abs(dt - float(ref["dt"])) <= 1e-4 * max(1.0, abs(float(ref["dt"]))), (mode, dt, float(ref["dt"]))


def _emulated_worker(rank, world, dev):
    """one rank as rank 0 of an emulated world of 3 (distributed.emulate_world): the stand-in rows get labels that match nothing"""
    import os
    os.environ["SDA_DP_SINGLE_RANK"] = "1"
    from speech_decoding_amd import clip, lib as L, ops
    from speech_decoding_amd.distributed import active_group, emulate_world
    assert active_group() is not None
    B, W = B_RANK, 3
    g = torch.Generator().manual_seed(79)
    Yl, Zl = torch.randn(B, F, T, generator=g).to(dev), torch.randn(B, F, T, generator=g).to(dev)
    lab = np.arange(B, dtype=np.int64) * 1000 - 5000            # ids that collide with nothing by value alone
    lab[7] = lab[2]
    emulate_world(W)
    res = {}
    for mode in MODES:
        crit = _crit(mode, dev)
        z = Zl.clone().requires_grad_(True)
        loss = crit(Yl, z, labels=lab)
        (dz,) = torch.autograd.grad(loss, [z])
        # the block form on exactly those rows, with the labels the emulation must have built
        rows, nsq = next(iter(crit._state.emulated.values()))
        Tp = L.rows_tp(T)
        Yall = ops.new_rows(W * B, T, L.pad_channels(F), torch.float32, dev)
        ops.pack_rows(Yl, Yall)
        Yall[B * Tp: W * B * Tp].copy_(rows)
        Zt = ops.new_rows(B, T, L.pad_channels(F), torch.float32, dev)
        ops.pack_rows(Zl, Zt)
        dense = np.unique(lab, return_inverse=True)[1]
        lab_all = torch.from_numpy(np.concatenate([dense, np.arange(B, W * B)]).astype(np.int32)).to(dev)
        share, _, cnt, cctx = clip.clip_forward(Yall, Zt, crit.temp.detach(), Bm=W * B, Bn=B, T=T, col0=0, B_global=W * B,
                                                 labels=lab_all, duplicates=mode)
        plain = float(clip.clip_forward(Yall, Zt, crit.temp.detach(), Bm=W * B, Bn=B, T=T, col0=0, B_global=W * B)[0])
        dZt = ops.new_rows(B, T, L.pad_channels(F), torch.float32, dev)
        clip.clip_backward(cctx, dZt, torch.ones(1, device=dev))
        torch.cuda.synchronize()
        res[mode] = dict(loss=float(loss), share=float(share), plain=plain, same_dz=torch.equal(dz, ops.rows_view(dZt, B, F, T)),
                         counts=cctx.counts.cpu())
    emulate_world(1)
    return res


def test_emulated_world_gives_the_stand_in_rows_labels_that_match_nothing():
    out = run_ranks(_emulated_worker, 1)[0]
    want = torch.ones(3 * B_RANK, dtype=torch.int32)
    want[[2, 7]] = 2
    for mode in MODES:
        r = out[mode]
        assert torch.equal(r["counts"], want), (mode, r["counts"])
        assert abs(r["loss"] - r["share"]) <= 1e-6 * max(1.0, abs(r["share"])) and r["same_dz"], (mode, r)
    assert out["mask"]["share"] != out["mask"]["plain"]
