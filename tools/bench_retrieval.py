"""Times decoding against a speech bank (speech_decoding_amd/retrieval.py) on the MI355X: the bank build, the similarity GEMM,
the selection kernel and the whole retrieve(), each beside plain torch on the same device and the same operands (the library
GEMM on the same packed rows with a 16-bit result widened to fp32, `topk` of the normalised matrix) as a library baseline.  Device events after warm-up; the two sides
alternate inside one run.

    python tools/bench_retrieval.py [--M 4096 32768] [--N 256] [--F 1024] [--T 360] [--dtype bf16] [--k 10] [--limit 420]

Every bank size runs in a process of its own under a time limit of its own (--limit seconds); after a size that fails or runs
out of time no further size is started.  Prints one JSON line per size (kept as profiles/retrieval_bench.json), times in
milliseconds per call.  The M = 32768 bank of the default shape takes about 24 GB."""
import argparse
import os
import sys

import harness


def timed(fns, iters, warmup, reps=1):
    """Milliseconds per call of each callable, the callables alternating (short kernels: reps back-to-back calls per bracket,
    the events' own resolution is a few microseconds)."""
    return [harness.summarize(s).mean for s in harness.alternating(fns, iters, warmup, reps)]


def one_size(a, M):
    import torch
    from speech_decoding_amd import SpeechBank, retrieve, lib as L, ops
    harness.need_gpu()
    from speech_decoding_amd.retrieval import _ScorePass, plan_blocks
    dev = "cuda:0"
    dt = {"fp32": torch.float32, "bf16": torch.bfloat16, "fp16": torch.float16}[a.dtype]
    N, F, T, k = a.N, a.F, a.T, a.k
    g = torch.Generator(device=dev).manual_seed(5)
    # bank build: batches of wav2vec2-sized output, timed per add() (pack + norms + the copy into the bank)
    bank = SpeechBank(F, T, dtype=dt, device=dev, capacity=M)
    batch, build_ms = 512, 0.0
    labels = torch.randint(M, (N,), generator=g, device=dev)
    queries = torch.randn((N, F, T), generator=g, device=dev)
    for m0 in range(0, M, batch):
        Y = torch.randn((min(batch, M - m0), F, T), generator=g, device=dev)
        s, e = harness.timing_event(), harness.timing_event()      # (behind the batch's randn on a busy stream, no drain in
        s.record()                                                 # front: not a harness form, whose windows start idle)
        bank.add(Y)
        e.record()
        e.synchronize()
        if m0:                                        # the first add loads the code objects
            build_ms += s.elapsed_time(e)
        del Y
    build_rows = M - min(batch, M)
    K = bank.row_elems
    nb, mc, tiles256, ks = plan_blocks(N, M, K, dt, a.scratch)
    sp = _ScorePass("bench_retrieval", queries, bank)         # retrieve()'s own pack, norms, scratch and block fill
    sp.start((nb, mc, tiles256, ks))
    Qt, qsq, csq, S, gemm = sp.Qt, sp.qsq, sp.csq, sp.S, sp.fill      # gemm(): the first block's scores, one GEMM per chunk
    n = gemm()
    Qm, Bm = Qt[: n * K].view(n, K), bank.rows

    def torch_gemm():
        return (Qm @ Bm.T).float()

    gemm_ms, torch_gemm_ms = timed([gemm, torch_gemm], a.iters, a.warmup)
    # selection on ONE fp32 (n, M) matrix for both sides: the plain matrix when the plan has one chunk, else a dense copy
    gemm()
    if mc >= M:
        plain, Mp = S, L.pad_channels(M)
    else:
        Mp = L.pad_channels(M)
        plain = torch.empty(n * Mp, dtype=torch.float32, device=dev)
        for c0 in range(0, M, mc):
            m = min(mc, M - c0)
            mp = L.pad_channels(m)
            plain.view(n, Mp)[:, c0: c0 + m] = sp.chunk(c0, n)[: n * mp].view(n, mp)[:, :m]
    dense = plain.view(n, Mp)
    lab = labels[:n].contiguous()
    out = {}

    def select():
        out["ours"] = ops.retrieval_select(plain, qsq, csq, n, M, k, None, labels=lab)

    def torch_select():
        den = torch.clamp(torch.sqrt(qsq[:n])[:, None] * torch.sqrt(csq)[None, :], min=1e-8)
        out["torch"] = torch.topk(dense[:, :M] / den, k, dim=1)

    def torch_select_ranks():
        den = torch.clamp(torch.sqrt(qsq[:n])[:, None] * torch.sqrt(csq)[None, :], min=1e-8)
        sc = dense[:, :M] / den
        out["torch"] = torch.topk(sc, k, dim=1)
        out["torch_ranks"] = (sc > sc.gather(1, lab[:, None])).sum(dim=1)

    sel_ms, tsel_ms, tselr_ms = timed([select, torch_select, torch_select_ranks], a.iters, a.warmup, reps=20)
    same_scores = bool(torch.equal(out["ours"][1], out["torch"].values))

    def whole():
        out["whole"] = retrieve(queries, bank, k=k, labels=labels, scratch_bytes=a.scratch)

    def torch_whole():
        sc = (Qt[: N * K].view(N, K) @ bank.rows.T).float() / torch.clamp(torch.sqrt(qsq)[:, None] * torch.sqrt(csq)[None, :], min=1e-8)
        out["torch_whole"] = torch.topk(sc, k, dim=1)

    whole_ms, twhole_ms = timed([whole, torch_whole], a.iters, a.warmup)
    bank_bytes = M * K * bank.rows.element_size()
    return {
        "bench": "retrieval", "N": N, "M": M, "F": F, "T": T, "dtype": a.dtype, "k": k, "plan": {"nb": nb, "mc": mc, "tiles256": tiles256, "ksplit": ks},
        "bank_gb": round(bank_bytes / 1e9, 2),
        "bank_build_ms_per_512": round(build_ms / max(1, build_rows) * 512, 3),
        "gemm_ms": round(gemm_ms, 3), "gemm_tb_per_s": round(bank_bytes / gemm_ms / 1e9, 2), "torch_gemm_ms": round(torch_gemm_ms, 3),
        "select_ms": round(sel_ms, 4), "torch_normalise_topk_ms": round(tsel_ms, 4), "torch_normalise_topk_ranks_ms": round(tselr_ms, 4),
        "select_scores_equal_torch": same_scores,
        "retrieve_ms": round(whole_ms, 3), "torch_whole_ms": round(twhole_ms, 3),
        "iters": a.iters, "warmup": a.warmup,
    }


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--M", type=int, nargs="+", default=[4096, 32768])
    ap.add_argument("--N", type=int, default=256)
    ap.add_argument("--F", type=int, default=1024)
    ap.add_argument("--T", type=int, default=360)
    ap.add_argument("--dtype", default="bf16", choices=["fp32", "bf16", "fp16"])
    ap.add_argument("--k", type=int, default=10)
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--scratch", type=int, default=1 << 30)
    ap.add_argument("--limit", type=int, default=420, help="seconds one bank size may take")
    ap.add_argument("--child", action="store_true", help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.child:
        harness.emit(one_size(a, a.M[0]))
        return 0
    for M in a.M:                                      # this process never opens the GPU: one fresh child per size
        cmd = [sys.executable, os.path.abspath(__file__), "--child", "--M", str(M), "--N", str(a.N), "--F", str(a.F), "--T", str(a.T),
               "--dtype", a.dtype, "--k", str(a.k), "--iters", str(a.iters), "--warmup", str(a.warmup), "--scratch", str(a.scratch)]
        status = harness.run_child(cmd, a.limit)
        if status != 0:                                # the sweep ends here: nothing is started after a child that ended badly
            harness.emit({"bench": "retrieval", "M": M, "error": harness.child_error(status, a.limit)})
            return 1
    return 0


if __name__ == "__main__":
    sys.exit(main())
