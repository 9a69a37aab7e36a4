"""What speech labels cost the CLIP loss: forward + backward of CLIPLoss with labels=None and with each `clip_duplicates` mode, the
loss tail's launches alone at the one-GPU block (256 x 256) and at the 8-rank per-rank block (4096 x 512), and bench.py's whole
training step with and without labels.  The callables of one comparison take turns inside every iteration (harness.alternating),
so all of them see the same clocks.  Device events after warm-up.  Diagnostic; not part of the product.

    python tools/bench_clip_labels.py [--iters 40] [--json profiles/clip_labels_bench.json]

Labels are host int64 ids drawn with replacement from 30000 segments (about one repeated pair per 256), handed in per call as a
feed would: the check and the upload are inside the timed region."""
import argparse
import os

import numpy as np
import torch

from harness import ROOT, alternating, emit, headline_batch, headline_modules, need_gpu, settle, summarize, us
from speech_decoding_amd import lib as L, ops

MODES = ("positive", "mask")
N_SEGMENTS = 30000


def stats(samples):
    s = us(summarize(samples))
    return {"median_us": s.median, "min_us": s.min, "max_us": s.max}


def compare(fns, iters):
    """{name: stats} of callables that take turns, plus each one's median over the first's"""
    out = {k: stats(v) for k, v in zip(fns, alternating(list(fns.values()), iters, 5))}
    base = next(iter(out.values()))["median_us"]
    for r in out.values():
        r["over_unlabelled"] = r["median_us"] / base
    return out


def draw_labels(B, seed=0):
    return np.random.RandomState(seed).randint(0, N_SEGMENTS, size=B).astype(np.int64)


def loss_fwd_bwd(B, F, T, dtype, iters, dev="cuda:0"):
    from speech_decoding.utils.loss import CLIPLoss
    from speech_decoding_amd.config import Config
    g = torch.Generator(device=dev).manual_seed(0)
    zbuf = ops.new_rows(B, T, L.pad_channels(F), dtype, dev)
    ops.pack_rows(torch.randn(B, F, T, generator=g, device=dev), zbuf)
    zbuf.requires_grad_(True)
    Z = ops.rows_view(zbuf, B, F, T)
    Y = torch.randn(B, F, T, generator=g, device=dev)
    lab = draw_labels(B)
    crits = {m: CLIPLoss(Config(reduction="mean", init_temperature=2.0, clip_duplicates=m)).to(dev) for m in MODES}

    def step(crit, labels):
        def run():
            crit(Y, Z, labels=labels).backward()
            zbuf.grad = None
            crit.temp.grad = None
        return run

    fns = {"labels=None": step(crits["positive"], None), **{m: step(crits[m], lab) for m in MODES}}
    r = {"B": B, "F": F, "T": T, "dtype": str(dtype).replace("torch.", ""), "repeated_pairs": int(B - len(set(lab.tolist()))), **compare(fns, iters)}
    for c in crits.values():
        c.release_buffers()
    return r


def tail(Bm, Bn, col0, dtype, iters, dev="cuda:0"):
    """the launches between the similarity GEMM and the dZ / dY GEMMs, on one (Bm x Bn) block"""
    g = torch.Generator(device=dev).manual_seed(1)
    Sm = torch.randn(Bm, L.pad_channels(Bn), generator=g, device=dev) * 30.0
    ysq = torch.rand(Bm, generator=g, device=dev) * 900.0 + 900.0
    zsq_all = torch.rand(Bm, generator=g, device=dev) * 900.0 + 900.0
    zsq = zsq_all[col0:col0 + Bn].contiguous()
    temp = torch.tensor([2.0], device=dev)
    lab = ops.upload_small(draw_labels(Bm, 1).astype(np.int32), dev)
    inv = 1.0 / (2 * Bm)

    def unlabelled():
        logits, _, _, col_lse, diag, row_lse = ops.clip_logits_stats(Sm, ysq, zsq, temp, Bm, Bn, col0)
        ops.clip_grad(logits, row_lse, col_lse, ysq, zsq, temp, inv, col0, dtype)
        ops.clip_ranks(logits, diag, col0)
        ops.clip_grad_y(logits, row_lse, col_lse, zsq, zsq_all, col0, dtype)

    def labelled(mode):
        def run():
            st = ops.clip_logits_stats_masked(Sm, ysq, zsq, temp, lab, Bm, Bn, col0) if mode == "mask" else \
                ops.clip_logits_stats(Sm, ysq, zsq, temp, Bm, Bn, col0)
            logits, _, _, col_lse, diag, row_lse = st
            counts = ops.clip_label_counts(lab)
            ops.clip_grad_labels(logits, row_lse, col_lse, ysq, zsq, temp, lab, counts, mode, inv, col0, dtype)
            ops.clip_ranks_labels(logits, diag, lab, col0)
            ops.clip_grad_y_labels(logits, row_lse, col_lse, zsq, zsq_all, lab, counts, mode, col0, dtype)
        return run

    fns = {"labels=None": unlabelled, **{m: labelled(m) for m in MODES}}
    return {"Bm": Bm, "Bn": Bn, "col0": col0, "dtype": str(dtype).replace("torch.", ""), **compare(fns, iters)}


def training_step(iters):
    """bench.py's default shape (bf16, batch 256): the step with labels=None and with a feed's ids (positive mode)"""
    from speech_decoding_amd import loss as sda_loss
    from speech_decoding_amd.optim import FusedAdam
    from speech_decoding_amd.streams import use_training_stream
    B, S = 256, 27
    cfg, enc, lossf, params = headline_modules("bf16")
    use_training_stream()
    opt = FusedAdam(params, lr=float(cfg.lr))
    X, Y = headline_batch(B)
    rng = np.random.RandomState(100)
    one = torch.ones((), dtype=torch.float32, device=X.device)
    lab = draw_labels(B)

    def step(labels):
        def run():
            subj = torch.from_numpy(rng.randint(0, S, size=B).astype(np.int32))
            lossf.prefetch(Y, enc.compute_dtype)
            Z = enc(X, subj)
            lb = None if labels is None else sda_loss.speech_labels(labels, B, X.device)
            loss = lossf(Y, Z, labels=lb)
            sda_loss.retrieval_ranks(Y, Z, labels=lb)
            opt.zero_grad(set_to_none=True)
            loss.backward(gradient=one)
            opt.step()
        return run

    fns = {"labels=None": step(None), "positive": step(lab)}
    for f in fns.values():
        for _ in range(5):
            f()
    settle()
    return {"shape": "bench.py default (bf16, B=256)", **compare(fns, iters)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=40)
    ap.add_argument("--json", default=os.path.join(ROOT, "profiles", "clip_labels_bench.json"))
    ap.add_argument("--skip-step", action="store_true", help="leave the whole training step out")
    a = ap.parse_args()
    need_gpu()
    rec = {"loss_fwd_bwd": loss_fwd_bwd(256, 1024, 360, torch.bfloat16, a.iters),
           "tail": [tail(256, 256, 0, torch.bfloat16, a.iters), tail(4096, 512, 512, torch.bfloat16, a.iters)]}
    if not a.skip_step:
        rec["training_step"] = training_step(a.iters)
    emit(rec, a.json, digits=3)


if __name__ == "__main__":
    main()
