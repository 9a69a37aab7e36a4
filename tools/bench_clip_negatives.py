"""What extra speech negatives cost the CLIP loss when they are read in place from resident tracks: the windowed score GEMM and the
three new launches alone, against the materialising route built from kernels that exist beside them (gather the N windows, then
the plain similarity GEMM and the plain dZ GEMM over the packed copy); forward + backward of CLIPLoss with N = 0, 1024, 4096; and
bench.py's whole training step with and without them.  The callables of one comparison take turns inside every iteration
(harness.alternating), so all of them see the same clocks.  Device events after warm-up.  Diagnostic; not part of the product.

    python tools/bench_clip_negatives.py [--iters 20] [--json profiles/clip_negatives_bench.json]

The table is TRACKS tracks of TRACK_ROWS rows (bench.py's F = 1024, T = 360, bf16); the negatives' starts are drawn uniformly
over it and sorted in time order, as a feed would hand them out of neighbouring tracks."""
import argparse
import os

import numpy as np
import torch

from harness import ROOT, alternating, emit, headline_batch, headline_modules, need_gpu, settle, summarize, us
from speech_decoding_amd import clip, lib as L, ops
from speech_decoding_amd.retrieval import WindowBank

NS = (1024, 4096)
TRACKS, TRACK_ROWS = 4, 20000


def stats(samples):
    s = us(summarize(samples))
    return {"median_us": s.median, "min_us": s.min, "max_us": s.max}


def compare(fns, iters):
    """{name: stats} of callables that take turns, plus each one's median over the first's"""
    out = {k: stats(v) for k, v in zip(fns, alternating(list(fns.values()), iters, 3))}
    base = next(iter(out.values()))["median_us"]
    for r in out.values():
        r["over_first"] = r["median_us"] / base
    return out


def make_bank(F, T, dtype, dev="cuda:0"):
    """the resident tracks, with a candidate at every 17th row (the pool a feed would draw from)"""
    g = torch.Generator(device=dev).manual_seed(5)
    bank = WindowBank(F, T, dtype=dtype, device=dev)
    for _ in range(TRACKS):
        bank.add_track(torch.randn(F, TRACK_ROWS, generator=g, device=dev), np.arange(0, TRACK_ROWS - T, 17))
    return bank


def draw(bank, N, seed=0):
    return bank.select(np.sort(np.random.RandomState(seed).choice(len(bank), size=N, replace=False)))


def kernels(B, F, T, dtype, N, iters, dev="cuda:0"):
    """the negatives' four launches on their own, and the two routes to the same scores and the same dZ"""
    Fp, Tp = L.pad_channels(F), L.rows_tp(T)
    K, row_elems = T * Fp, Tp * Fp
    g = torch.Generator(device=dev).manual_seed(1)
    zbuf = ops.new_rows(B, T, Fp, dtype, dev)
    ops.pack_rows(torch.randn(B, F, T, generator=g, device=dev), zbuf)
    zsq = ops.rows_sumsq(zbuf, B, row_elems, row_elems)
    sub = draw(make_bank(F, T, dtype, dev), N)
    ng = clip.ClipNegatives.of(sub)
    temp = torch.tensor([2.0], device=dev)
    Np = L.pad_channels(N)
    ks = L.load().sda_sim_gemm_ksplit(B, N, K, ops.dt_code(dtype))
    Sn = torch.empty((B, Np), dtype=torch.float32, device=dev)
    partial = torch.empty(ks * B * Np if ks > 1 else 0, dtype=torch.float32, device=dev)
    X = zbuf.reshape(-1)[L.ROW_PAD * Fp:]
    col_lse = torch.full((B,), 5.0, device=dev)
    rscale, scalars = torch.zeros(B, device=dev), torch.zeros(2, device=dev)
    dZ = ops.new_rows(B, T, Fp, dtype, dev)
    inv = 1.0 / (2 * B)

    def scores():
        ops.sim_gemm_windows_into(X, row_elems, ng.table.reshape(-1), ng.starts, ng.lo, ng.hi, Fp, B, N, K, ks, partial, Sn)
    scores()
    mlog = ops.clip_neg_stats(Sn, ng.wsq, zsq, temp, col_lse.clone(), B, N)
    Gn, cs_n = ops.clip_neg_grad(mlog, col_lse, ng.wsq, zsq, temp, inv, rscale, scalars, dtype)
    idx = torch.arange(N, device=dev)
    packed = ops.gather_windows(ng.table, ng.starts, idx, N, T)
    G_pl = torch.zeros((N + 1, L.pad_channels(B)), dtype=dtype, device=dev)
    G_pl[:N] = Gn[:N]
    out_pl = ops.new_rows(B, T, Fp, dtype, dev)

    def in_place():
        scores()
        ops.clip_dz_windows(Gn, ng.table, ng.starts, ng.lo, ng.hi, dZ, cs_n, N=N, Bn=B, T=T)

    def materialised():
        rows = ops.gather_windows(ng.table, ng.starts, idx, N, T)
        ops.matmul_nt_splitk(zbuf, rows, B, N, row_elems, row_elems)
        ops.clip_dz(G_pl, rows, zbuf, out_pl, rscale, cs_n, Bm=N, Bn=B, row_elems=row_elems)

    alone = {"sim_gemm_windows": scores,
             "clip_neg_stats": lambda: ops.clip_neg_stats(Sn, ng.wsq, zsq, temp, col_lse, B, N),
             "clip_neg_grad": lambda: ops.clip_neg_grad(mlog, col_lse, ng.wsq, zsq, temp, inv, rscale, scalars, dtype),
             "clip_dz_windows": lambda: ops.clip_dz_windows(Gn, ng.table, ng.starts, ng.lo, ng.hi, dZ, cs_n, N=N, Bn=B, T=T),
             "gather_windows": lambda: ops.gather_windows(ng.table, ng.starts, idx, N, T),
             "sim_gemm (packed copy)": lambda: ops.matmul_nt_splitk(zbuf, packed, B, N, row_elems, row_elems),
             "clip_dz (packed copy)": lambda: ops.clip_dz(G_pl, packed, zbuf, out_pl, rscale, cs_n, Bm=N, Bn=B, row_elems=row_elems)}
    r = {"B": B, "F": F, "T": T, "N": N, "dtype": str(dtype).replace("torch.", ""), "ksplit": ks, "alone": compare(alone, iters),
         "routes": compare({"in place": in_place, "materialised": materialised}, iters)}
    flop = 2.0 * N * B * K
    r["clip_dz_windows_tflops"] = flop / (r["alone"]["clip_dz_windows"]["median_us"] * 1e-6) / 1e12
    r["clip_dz_packed_tflops"] = 2.0 * N * B * row_elems / (r["alone"]["clip_dz (packed copy)"]["median_us"] * 1e-6) / 1e12
    e = 2                                                 # bytes per element
    window_bytes, z_bytes = N * K * e, B * row_elems * e
    # in place: both GEMMs read the windows (overlapping ones share cache lines: an upper bound) and Z or dZ; the dZ pass reads
    # and writes dZ.  materialised: the gather reads the windows and writes the packed copy, both GEMMs read the copy
    r["bytes"] = {"in place (upper bound)": 2 * window_bytes + z_bytes + 2 * z_bytes,
                  "materialised": window_bytes + 3 * N * row_elems * e + z_bytes + 2 * z_bytes,
                  "packed copy": N * row_elems * e}
    return r


def loss_fwd_bwd(B, F, T, dtype, iters, dev="cuda:0"):
    from speech_decoding.utils.loss import CLIPLoss
    from speech_decoding_amd.config import Config
    g = torch.Generator(device=dev).manual_seed(0)
    zbuf = ops.new_rows(B, T, L.pad_channels(F), dtype, dev)
    ops.pack_rows(torch.randn(B, F, T, generator=g, device=dev), zbuf)
    zbuf.requires_grad_(True)
    Z = ops.rows_view(zbuf, B, F, T)
    Y = torch.randn(B, F, T, generator=g, device=dev)
    bank = make_bank(F, T, dtype, dev)
    crit = CLIPLoss(Config(reduction="mean", init_temperature=2.0)).to(dev)

    def step(neg):
        def run():
            crit(Y, Z, negatives=neg).backward()
            zbuf.grad = None
            crit.temp.grad = None
        return run
    fns = {"N=0": step(None), **{f"N={n}": step(draw(bank, n)) for n in NS}}
    r = {"B": B, "F": F, "T": T, "dtype": str(dtype).replace("torch.", ""), **compare(fns, iters)}
    crit.release_buffers()
    return r


def training_step(iters):
    """bench.py's default shape (bf16, batch 256): the step without negatives and with a fixed bank of N of them"""
    from speech_decoding_amd import loss as sda_loss
    from speech_decoding_amd.optim import FusedAdam
    from speech_decoding_amd.streams import use_training_stream
    B, S = 256, 27
    cfg, enc, lossf, params = headline_modules("bf16")
    use_training_stream()
    opt = FusedAdam(params, lr=float(cfg.lr))
    X, Y = headline_batch(B)
    bank = make_bank(1024, 360, torch.bfloat16, X.device)
    rng = np.random.RandomState(100)
    one = torch.ones((), dtype=torch.float32, device=X.device)

    def step(neg):
        def run():
            subj = torch.from_numpy(rng.randint(0, S, size=B).astype(np.int32))
            lossf.prefetch(Y, enc.compute_dtype)
            Z = enc(X, subj)
            loss = lossf(Y, Z, negatives=neg)
            sda_loss.retrieval_ranks(Y, Z)
            opt.zero_grad(set_to_none=True)
            loss.backward(gradient=one)
            opt.step()
        return run

    fns = {"N=0": step(None), **{f"N={n}": step(draw(bank, n)) for n in NS}}
    for f in fns.values():
        for _ in range(3):
            f()
    settle()
    return {"shape": "bench.py default (bf16, B=256)", **compare(fns, iters)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--json", default=os.path.join(ROOT, "profiles", "clip_negatives_bench.json"))
    ap.add_argument("--skip-step", action="store_true", help="leave the whole training step out")
    a = ap.parse_args()
    need_gpu()
    rec = {"kernels": [kernels(256, 1024, 360, torch.bfloat16, n, a.iters) for n in NS],
           "loss_fwd_bwd": loss_fwd_bwd(256, 1024, 360, torch.bfloat16, a.iters)}
    if not a.skip_step:
        rec["training_step"] = training_step(a.iters)
    emit(rec, a.json, digits=3)


if __name__ == "__main__":
    main()
