"""Times word-level decoding (speech_decoding_amd/retrieval.py: retrieve_classes) on the MI355X: the class-reduction kernel, the
row-pooling kernel and the selection over classes each alone; retrieve_classes whole beside retrieve whole on the same bank; and
the same pooling as a torch chain on the same device and the same fp32 score matrix (normalise, scatter_reduce amax, scatter_add
of exp, log, logsumexp over classes, topk), the two sides alternating call by call.  Device events after warm-up.

    python tools/bench_class_decode.py [--N 256] [--M 32768] [--C 4096] [--F 1024] [--T 360] [--dtype bf16] [--limit 420]

The measurement runs in a process of its own under a time limit (--limit seconds).  Prints one JSON line (kept as
profiles/class_decode_bench.json), times in milliseconds per call.  Class sizes are Zipf-like (count of the r-th most frequent
class ~ 1 / r, every class at least one member), members dealt over the bank at random.  The byte floor the reduction is
compared against is one read of the score matrix, n * M * 4 bytes (`order` stays in L2).  The default bank takes about 24 GB."""
import argparse
import os
import sys

import harness

HBM_TB_S = 6.29        # measured float4 copy rate of one MI355X (8.0 TB/s is the specification)


def timed(fns, iters, warmup, reps=1):
    """Milliseconds per call of each callable, the callables alternating, reps back-to-back calls per bracket."""
    return [harness.summarize(s).mean for s in harness.alternating(fns, iters, warmup, reps)]


def zipf_classes(M, C, seed):
    import numpy as np
    rng = np.random.default_rng(seed)
    wgt = 1.0 / np.arange(1, C + 1)
    counts = 1 + np.floor(wgt * (M - C) / wgt.sum()).astype(np.int64)
    counts[0] += M - counts.sum()
    return np.repeat(np.arange(C), counts)[rng.permutation(M)], counts


def measure(a):
    import numpy as np
    import torch
    from speech_decoding_amd import ClassIndex, SpeechBank, retrieve, retrieve_classes, lib as L, ops
    from speech_decoding_amd.retrieval import _ScorePass, plan_class_blocks
    harness.need_gpu()
    dev = "cuda:0"
    dt = {"fp32": torch.float32, "bf16": torch.bfloat16, "fp16": torch.float16}[a.dtype]
    N, M, C, F, T, k, scale = a.N, a.M, a.C, a.F, a.T, a.k, a.scale
    g = torch.Generator(device=dev).manual_seed(5)
    bank = SpeechBank(F, T, dtype=dt, device=dev, capacity=M)
    first = None
    for m0 in range(0, M, 512):
        Y = torch.randn((min(512, M - m0), F, T), generator=g, device=dev)
        bank.add(Y)
        first = Y if first is None else first
        del Y
    ids, counts = zipf_classes(M, C, seed=9)
    index = ClassIndex(ids, num_classes=C, device=dev)
    labels_bank = torch.randint(first.shape[0], (N,), generator=g, device=dev)      # planted on candidates of the first batch
    labels_class = torch.from_numpy(ids).to(dev)[labels_bank]
    queries = 0.35 * first[labels_bank] + torch.randn((N, F, T), generator=g, device=dev)
    del first
    K = bank.row_elems
    nb, mc, tiles256, ks = plan_class_blocks(N, M, C, K, dt, a.scratch)
    sp = _ScorePass("bench_class_decode", queries, bank)      # retrieve_classes()'s own pack, norms, scratch and block fill
    sp.start((nb, mc, tiles256, ks))
    n, qsq, csq, S = sp.fill(), sp.qsq, sp.csq, sp.S          # the first block's scores
    Cp, Mp = L.pad_channels(C), L.pad_channels(M)
    order, offsets = index.order_dev, index.offsets_dev
    V = torch.empty((n, Cp), dtype=torch.float32, device=dev)
    row_lse = torch.empty(n, dtype=torch.float32, device=dev)
    ones = torch.ones(max(n, C), dtype=torch.float32, device=dev)
    lab = labels_class[:n].contiguous()
    out = {}

    def reduce_fn(mode):
        return lambda: ops.retrieval_class_reduce(S, qsq, csq, order, offsets, n, M, C, scale, mode, mc, out=V, row_lse=row_lse)

    sum_ms, mean_ms, max_ms = timed([reduce_fn("sum"), reduce_fn("mean"), reduce_fn("max")], a.iters, a.warmup, reps=10)
    reduce_fn("sum")()

    def select():
        out["ours"] = ops.retrieval_select(V, ones, ones, n, C, k, Cp, labels=lab)

    groups = np.arange(n) % max(1, n // 4)                    # groups of four repetitions, interleaved
    G = int(groups.max()) + 1
    rows_dev = torch.from_numpy(np.argsort(groups, kind="stable").astype(np.int32)).to(dev)
    goff_dev = torch.from_numpy(np.concatenate([[0], np.cumsum(np.bincount(groups))]).astype(np.int32)).to(dev)
    P = torch.empty((G, Cp), dtype=torch.float32, device=dev)

    def pool():
        ops.retrieval_pool_rows(V, rows_dev, goff_dev, n, G, C, out=P)

    select_ms, pool_ms = timed([select, pool], a.iters, a.warmup, reps=10)

    # the same pooling as a torch chain on the same fp32 matrix (dense: the plan's single chunk, or a dense copy of the chunks)
    if mc >= M:
        dense = S[: n * Mp].view(n, Mp)[:, :M]
    else:
        dense = torch.empty((n, M), dtype=torch.float32, device=dev)
        for c0 in range(0, M, mc):
            m = min(mc, M - c0)
            mp = L.pad_channels(m)
            dense[:, c0: c0 + m] = sp.chunk(c0, n)[: n * mp].view(n, mp)[:, :m]
    cls = torch.from_numpy(ids).to(dev)[None, :].expand(n, M).contiguous()

    def ours_chain():
        ops.retrieval_class_reduce(S, qsq, csq, order, offsets, n, M, C, scale, "sum", mc, out=V, row_lse=row_lse)
        out["ours"] = ops.retrieval_select(V, ones, ones, n, C, k, Cp, labels=lab)

    def torch_chain():
        den = torch.clamp(torch.sqrt(qsq[:n])[:, None] * torch.sqrt(csq)[None, :], min=1e-8)
        lg = scale * (dense / den)
        m = torch.full((n, C), float("-inf"), device=dev).scatter_reduce(1, cls, lg, "amax", include_self=True)
        s = torch.zeros((n, C), device=dev).scatter_add(1, cls, torch.exp(lg - m.gather(1, cls)))
        f = m + torch.log(s)
        val = f - torch.logsumexp(f, dim=1, keepdim=True)
        out["torch_values"] = val
        out["torch"] = torch.topk(val, k, dim=1)
        out["torch_ranks"] = (val > val.gather(1, lab[:, None])).sum(dim=1)

    ours_ms, torch_ms = timed([ours_chain, torch_chain], a.iters, a.warmup, reps=5)
    diff = float((V[:, :C] - out["torch_values"]).abs().max())
    same_top1 = float((out["ours"][0][:, 0] == out["torch"].indices[:, 0]).float().mean())

    def whole_classes():
        out["whole"] = retrieve_classes(queries, bank, index, k=k, scale=scale, labels=labels_class, scratch_bytes=a.scratch)

    def whole_retrieve():
        out["retrieve"] = retrieve(queries, bank, k=k, labels=labels_bank, scratch_bytes=a.scratch)

    wc_ms, wr_ms = timed([whole_classes, whole_retrieve], a.iters, a.warmup)
    floor_bytes = n * M * 4
    floor_us = floor_bytes / (HBM_TB_S * 1e12) * 1e6
    return {
        "bench": "class_decode", "N": N, "M": M, "C": C, "F": F, "T": T, "dtype": a.dtype, "k": k, "scale": scale,
        "plan": {"nb": nb, "mc": mc, "tiles256": tiles256, "ksplit": ks}, "rows_per_launch": n,
        "class_sizes": {"largest": int(counts.max()), "median": int(np.median(counts)), "above_256": int((counts > 256).sum()),
                        "singletons": int((counts == 1).sum())},
        "class_reduce_sum_ms": round(sum_ms, 4), "class_reduce_mean_ms": round(mean_ms, 4), "class_reduce_max_ms": round(max_ms, 4),
        "reduce_byte_floor_us": round(floor_us, 2), "reduce_byte_floor_is": f"one read of n * M * 4 bytes at {HBM_TB_S} TB/s",
        "class_reduce_sum_tb_per_s": round(floor_bytes / sum_ms / 1e9, 3),
        "class_reduce_sum_share_of_floor": round(floor_us / (sum_ms * 1e3), 4),
        "pool_rows_ms": round(pool_ms, 4), "pool_groups": G, "select_over_classes_ms": round(select_ms, 4),
        "reduce_plus_select_ms": round(ours_ms, 4), "torch_scatter_chain_ms": round(torch_ms, 4),
        "max_abs_diff_to_torch_chain": diff, "top1_equal_torch_chain": same_top1,
        "retrieve_classes_ms": round(wc_ms, 3), "retrieve_ms": round(wr_ms, 3),
        "top1_class_accuracy": out["whole"].accuracy(1),
        "iters": a.iters, "warmup": a.warmup,
    }


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--N", type=int, default=256)
    ap.add_argument("--M", type=int, default=32768)
    ap.add_argument("--C", type=int, default=4096)
    ap.add_argument("--F", type=int, default=1024)
    ap.add_argument("--T", type=int, default=360)
    ap.add_argument("--dtype", default="bf16", choices=["fp32", "bf16", "fp16"])
    ap.add_argument("--k", type=int, default=10)
    ap.add_argument("--scale", type=float, default=164.0219)      # exp(5.1), CLIPLoss' initial temperature
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--scratch", type=int, default=1 << 30)
    ap.add_argument("--limit", type=int, default=420, help="seconds the measurement may take")
    ap.add_argument("--child", action="store_true", help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.child:
        harness.emit(measure(a))
        return 0
    cmd = [sys.executable, os.path.abspath(__file__), "--child"]      # this process never opens the GPU: one fresh child
    for name in ("N", "M", "C", "F", "T", "dtype", "k", "scale", "iters", "warmup", "scratch"):
        cmd += [f"--{name}", str(getattr(a, name))]
    status = harness.run_child(cmd, a.limit)
    if status != 0:
        harness.emit({"bench": "class_decode", "error": harness.child_error(status, a.limit)})
        return 1
    return 0


if __name__ == "__main__":
    sys.exit(main())
