"""The pairwise sigmoid loss against the CLIP loss: forward + backward of SigmoidLoss and CLIPLoss at the one-GPU shape
(B = 256, F = 1024, T = 360, bf16) with the brain-side gradient alone (dZ) and with the speech-side gradient too (dZ + dY), and
the loss tail's launches alone on the 256 x 256 block and on the 2048 x 256 block a rank of eight holds.  The two losses take turns
call by call inside every iteration (harness.alternating), so both see the same clocks.  Device events after warm-up.
Diagnostic; not part of the product.

    python tools/bench_sigmoid_loss.py [--iters 40] [--json profiles/sigmoid_loss_bench.json]
"""
import argparse
import os
import statistics

import torch

from harness import ROOT, alternating, emit, need_gpu, summarize, us
from speech_decoding_amd import lib as L, ops


def stats(samples):
    s = us(summarize(samples))
    return {"mean_us": s.mean, "stdev_us": 1e3 * statistics.pstdev(samples), "median_us": s.median, "min_us": s.min, "max_us": s.max}


def compare(fns, iters):
    """{name: stats} of callables that take turns, plus each one's mean over the first's"""
    out = {k: stats(v) for k, v in zip(fns, alternating(list(fns.values()), iters, 5))}
    base = next(iter(out.values()))["mean_us"]
    for r in out.values():
        r["over_clip"] = r["mean_us"] / base
    return out


def loss_fwd_bwd(B, F, T, dtype, iters, want_dy, dev="cuda:0"):
    from speech_decoding.utils.loss import CLIPLoss, SigmoidLoss
    from speech_decoding_amd.config import Config
    g = torch.Generator(device=dev).manual_seed(0)

    def rows(seed_scale):
        buf = ops.new_rows(B, T, L.pad_channels(F), dtype, dev)
        ops.pack_rows(torch.randn(B, F, T, generator=g, device=dev) * seed_scale, buf)
        buf.requires_grad_(True)
        return buf, ops.rows_view(buf, B, F, T)

    zbuf, Z = rows(1.0)
    if want_dy:                    # a second tower's output: the gradient leaves in row layout
        ybuf, Y = rows(1.0)
    else:
        ybuf, Y = None, torch.randn(B, F, T, generator=g, device=dev)
    crits = {"clip": CLIPLoss(Config(reduction="mean", init_temperature=2.0)).to(dev),
             "sigmoid": SigmoidLoss(Config(reduction="mean")).to(dev)}

    def step(crit):
        def run():
            crit(Y, Z).backward()
            zbuf.grad = None
            if ybuf is not None:
                ybuf.grad = None
            for p in crit.parameters():
                p.grad = None
        return run

    r = {"B": B, "F": F, "T": T, "dtype": str(dtype).replace("torch.", ""), "gradients": "dZ + dY" if want_dy else "dZ",
         **compare({k: step(c) for k, c in crits.items()}, iters)}
    for c in crits.values():
        c.release_buffers()
    return r


def tail(Bm, Bn, col0, dtype, iters, want_dy, dev="cuda:0"):
    """the launches between the similarity GEMM and the dZ / dY GEMMs on one (Bm x Bn) block (the CLIP loss's without the
    cross-rank merge of its row statistics, which a block of several ranks needs besides)"""
    g = torch.Generator(device=dev).manual_seed(1)
    Sm = torch.randn(Bm, L.pad_channels(Bn), generator=g, device=dev) * 30.0
    ysq = torch.rand(Bm, generator=g, device=dev) * 900.0 + 900.0
    zsq_all = torch.rand(Bm, generator=g, device=dev) * 900.0 + 900.0
    zsq = zsq_all[col0:col0 + Bn].contiguous()
    temp, bias = torch.tensor([2.0], device=dev), torch.tensor([-10.0], device=dev)

    def clip():
        logits, _, _, col_lse, diag, row_lse = ops.clip_logits_stats(Sm, ysq, zsq, temp, Bm, Bn, col0)
        ops.clip_grad(logits, row_lse, col_lse, ysq, zsq, temp, 1.0 / (2 * Bm), col0, dtype)
        ops.clip_ranks(logits, diag, col0)
        if want_dy:
            _, part = ops.clip_grad_y(logits, row_lse, col_lse, zsq, zsq_all, col0, dtype)
            ops.clip_grad_y_finish(part, ysq, zsq_all, temp, 1.0 / (2 * Bm), 0, Bm)

    def sigmoid():
        a, diag, _, part = ops.sigmoid_pairs(Sm, ysq, zsq, temp, bias, Bm, Bn, col0, dtype)
        ops.sigmoid_finish(part, ysq, zsq, temp, 1.0 / Bm)
        ops.clip_ranks(a, diag, col0)
        if want_dy:
            _, party = ops.sigmoid_grad_y(a, bias, zsq, zsq_all, col0, dtype)
            ops.clip_grad_y_finish(party, ysq, zsq_all, temp, 1.0 / Bm, 0, Bm)

    return {"Bm": Bm, "Bn": Bn, "col0": col0, "dtype": str(dtype).replace("torch.", ""), "gradients": "dZ + dY" if want_dy else "dZ",
            "launches": {"clip": 5 + 2 * want_dy, "sigmoid": 3 + 2 * want_dy}, **compare({"clip": clip, "sigmoid": sigmoid}, iters)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=40)
    ap.add_argument("--json", default=os.path.join(ROOT, "profiles", "sigmoid_loss_bench.json"))
    a = ap.parse_args()
    need_gpu()
    bf16 = torch.bfloat16
    rec = {"loss_fwd_bwd": [loss_fwd_bwd(256, 1024, 360, bf16, a.iters, want_dy) for want_dy in (False, True)],
           "tail": [tail(Bm, Bn, col0, bf16, a.iters, want_dy) for Bm, Bn, col0 in ((256, 256, 0), (2048, 256, 256)) for want_dy in (False, True)]}
    emit(rec, a.json, digits=3)


if __name__ == "__main__":
    main()
