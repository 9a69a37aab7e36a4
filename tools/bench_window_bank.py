"""Times decoding against a WindowBank (windows of one continuous track, speech_decoding_amd/retrieval.py) on the MI355X beside
the SAME candidates materialised into a SpeechBank: bytes held, the similarity GEMM + slab sum alone, and retrieve() whole.
Device events after warm-up; the two sides alternate call by call inside one run; mean and spread of --iters calls.

    python tools/bench_window_bank.py [--M 4096 32768] [--hop 36] [--dense-M 131072] [--dense-hop 9] [--N 256] [--F 1024] [--T 360]

The candidates are one window every `hop` rows of one track, in time order.  The last row (--dense-M windows every --dense-hop
rows, over the table of the largest --M) is measured for the WindowBank alone: no SpeechBank of that size is built (131072
candidates of the default shape would take 101 GB), the point is that it runs.  Every size runs in a process of its own under a
time limit of its own (--limit seconds); after a size that fails or runs out of time no further size is started.  Prints one
JSON line per size and keeps them in --out (profiles/window_bank_bench.json), times in milliseconds per call."""
import argparse
import os
import sys

import harness


def timed(fns, iters, warmup):
    """Per callable (mean, standard deviation, min, max) in milliseconds of `iters` calls, the callables alternating call by call."""
    out = []
    for v in harness.alternating(fns, iters, warmup):
        s = harness.summarize(v)
        out.append({"mean": round(s.mean, 3), "std": round((sum((x - s.mean) ** 2 for x in v) / s.n) ** 0.5, 3),
                    "min": round(s.min, 3), "max": round(s.max, 3)})
    return out


def one_size(a, M, hop, rows, with_speech_bank):
    import numpy as np
    import torch
    from speech_decoding_amd import SpeechBank, WindowBank, retrieve, lib as L
    from speech_decoding_amd.retrieval import _ScorePass, plan_blocks
    harness.need_gpu()
    dev = "cuda:0"
    dt = {"bf16": torch.bfloat16, "fp16": torch.float16}[a.dtype]
    N, F, T, k = a.N, a.F, a.T, a.k
    Cp = L.pad_channels(F)
    g = torch.Generator(device=dev).manual_seed(5)
    track = torch.randn((F, rows), generator=g, device=dev).to(dt)
    starts = np.arange(M, dtype=np.int64) * hop
    assert starts[-1] + T <= rows
    wbank = WindowBank(F, T, dtype=dt, device=dev)
    wbank.add_track(track, starts)
    del track
    labels = torch.randint(M, (N,), generator=g, device=dev)
    queries = torch.randn((N, F, T), generator=g, device=dev)
    sides = {"window": wbank}
    if with_speech_bank:
        # the same candidates, materialised: strided (m, F, T) views of the table, packed batch by batch
        sbank = SpeechBank(F, T, dtype=dt, device=dev, capacity=M)
        flat = wbank.table.reshape(-1)
        for m0 in range(0, M, 512):
            m = min(512, M - m0)
            sbank.add(flat.as_strided((m, F, T), (hop * Cp, 1, Cp), flat.storage_offset() + m0 * hop * Cp))
        sides["speech"] = sbank
    res = {"bench": "window_bank", "N": N, "M": M, "hop": hop, "F": F, "T": T, "dtype": a.dtype, "k": k, "table_rows": rows,
           "iters": a.iters, "warmup": a.warmup}
    span_bytes = (int(starts[-1]) + T) * Cp * 2                   # the distinct table bytes the candidates cover
    res["window_bank_bytes"] = wbank.nbytes
    res["speech_bank_bytes"] = M * L.rows_tp(T) * Cp * 2 + 4 * M        # what the materialised bank holds (built or not)
    res["bytes_ratio"] = round(res["speech_bank_bytes"] / wbank.nbytes, 2)
    passes, fills, wholes, out = {}, [], [], {}
    for name, bank in sides.items():
        sp = _ScorePass("bench_window_bank", queries, bank)
        plan = plan_blocks(N, M, sp.K, dt, a.scratch)
        sp.start(plan)
        passes[name] = sp
        res[name + "_plan"] = {"nb": plan[0], "mc": plan[1], "ksplit": plan[3], "K": sp.K}
        fills.append(sp.fill)                                     # the first block's scores: one GEMM + slab sum per chunk
        wholes.append(lambda bank=bank, name=name: out.__setitem__(name, retrieve(queries, bank, k=k, labels=labels, scratch_bytes=a.scratch)))
    for name, t in zip(sides, timed(fills, a.iters, a.warmup)):
        res[name + "_gemm_ms"] = t
    for name, t in zip(sides, timed(wholes, a.iters, a.warmup)):
        res[name + "_retrieve_ms"] = t
    res["window_gemm_distinct_tb_per_s"] = round(span_bytes / res["window_gemm_ms"]["mean"] / 1e9, 3)
    if with_speech_bank:
        res["speech_gemm_tb_per_s"] = round(M * L.rows_tp(T) * Cp * 2 / res["speech_gemm_ms"]["mean"] / 1e9, 3)
        res["gemm_ratio_window_over_speech"] = round(res["window_gemm_ms"]["mean"] / res["speech_gemm_ms"]["mean"], 3)
        res["retrieve_ratio_window_over_speech"] = round(res["window_retrieve_ms"]["mean"] / res["speech_retrieve_ms"]["mean"], 3)
        w, s = out["window"], out["speech"]
        # different K (the SpeechBank contracts over the zero pad rows too) and K slices: the fp32 sums may differ in the last bits
        res["same_top1"] = float((w.indices[:, 0] == s.indices[:, 0]).float().mean())
        res["max_score_difference"] = float((w.scores - s.scores).abs().max())
        res["ranks_equal"] = bool(torch.equal(w.ranks, s.ranks))
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--M", type=int, nargs="+", default=[4096, 32768])
    ap.add_argument("--hop", type=int, default=36)
    ap.add_argument("--dense-M", type=int, default=131072, help="0: skip the dense row")
    ap.add_argument("--dense-hop", type=int, default=9)
    ap.add_argument("--N", type=int, default=256)
    ap.add_argument("--F", type=int, default=1024)
    ap.add_argument("--T", type=int, default=360)
    ap.add_argument("--dtype", default="bf16", choices=["bf16", "fp16"])
    ap.add_argument("--k", type=int, default=10)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--scratch", type=int, default=1 << 30)
    ap.add_argument("--limit", type=int, default=420, help="seconds one size may take")
    ap.add_argument("--out", default=os.path.join(harness.ROOT, "profiles", "window_bank_bench.json"))
    ap.add_argument("--child", nargs=4, type=int, metavar=("M", "HOP", "ROWS", "SPEECH"), help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.child:
        M, hop, rows, speech = a.child
        harness.emit(one_size(a, M, hop, rows, bool(speech)))
        return 0
    sizes = [(M, a.hop, (M - 1) * a.hop + a.T, 1) for M in a.M]
    if a.dense_M:
        rows = max(max(s[2] for s in sizes), (a.dense_M - 1) * a.dense_hop + a.T)
        sizes.append((a.dense_M, a.dense_hop, rows, 0))
    lines = []
    for size in sizes:                                 # this process never opens the GPU: one fresh child per size
        cmd = [sys.executable, os.path.abspath(__file__), "--child", *map(str, size), "--N", str(a.N), "--F", str(a.F), "--T", str(a.T),
               "--dtype", a.dtype, "--k", str(a.k), "--iters", str(a.iters), "--warmup", str(a.warmup), "--scratch", str(a.scratch)]
        said = []
        status = harness.run_child(cmd, a.limit, lines=said)
        if status != 0:                                # the sweep ends here: nothing is started after a child that ended badly
            harness.emit({"bench": "window_bank", "M": size[0], "error": harness.child_error(status, a.limit)})
            return 1
        print(said[-1], flush=True)
        lines.append(said[-1])
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
