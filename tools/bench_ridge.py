"""Times the time-lagged ridge baseline (speech_decoding_amd/ridge.py on csrc/lagged_cov.hip) on the MI355X at the headline
segment shape — B 256, C 208, T 360, L 60 lags (12 480 features) — with F = 120 (mel) and F = 1024 (wav2vec 2.0) speech features:

  * `sda_lagged_cov_f32` alone, the Gram blocks (a = b = x) and the cross products (a = x, b = y), and beside each the same lag
    products formed by torch's own fp32 matmul on the same GPU (views d rows apart of contiguous, unpadded lag-layout arrays,
    one matmul per lag), the two alternating call by call;
  * a whole `partial_fit`, and the strided copy into the lag layout alone (its share decides whether a pack kernel is worth it);
  * `solve` for one alpha at P = 12 480 (Gram assembly + Cholesky + substitution);
  * `predict` for one alpha (the window GEMM).

    python tools/bench_ridge.py [--features 120 1024] [--out FILE]

Device events after warm-up; every line is one JSON object, printed and written to --out (profiles/ridge_bench.json unless
given; the file is started afresh), times in milliseconds per call.  Useful FLOP = 2 B T L C C' (C' = C or F): valid rows and
channels only, neither the zero rows between segments nor the channel padding; the share is against the 155 TFLOP/s this
project measured for fp32 MFMA."""
import argparse
import os

import harness

FP32_MATRIX_MEASURED_TF = 155.0


def r3(s):
    return {"ms": round(s.mean, 4), "min_ms": round(s.min, 4), "max_ms": round(s.max, 4)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--features", type=int, nargs="+", default=[120, 1024])
    ap.add_argument("--batch", type=int, default=256)
    ap.add_argument("--channels", type=int, default=208)
    ap.add_argument("--samples", type=int, default=360)
    ap.add_argument("--lags", type=int, default=60)
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(harness.ROOT, "profiles", "ridge_bench.json"))
    a = ap.parse_args()
    import torch
    from speech_decoding_amd import ops
    from speech_decoding_amd.ridge import LaggedRidge
    harness.need_gpu()
    open(a.out, "w").close()
    dev = torch.device("cuda", 0)
    B, C, T, Lg = a.batch, a.channels, a.samples, a.lags
    H, rows = Lg - 1, a.batch * (a.samples + a.lags - 1)

    def emit(rec):
        harness.emit(rec, a.out, append=True)

    def pair(ours, theirs):
        return map(harness.summarize, harness.alternating((ours, theirs), a.iters, a.warmup))

    def torch_lags(p, q):
        """out[d] = p[d:]^T q[:rows - d], one fp32 matmul per lag on views of the same arrays"""
        return torch.stack([p[d:].t() @ q[:rows - d] for d in range(Lg)])

    for F in a.features:
        X, Y = harness.headline_batch(B, C, T, F)
        ridge = LaggedRidge(C, F, n_lags=Lg, device=dev)
        xb, yb = ridge._lag_rows("x", X, ridge.Cp), ridge._lag_rows("y", Y, ridge.Fp)
        xt, yt = xb[:, :C].contiguous(), yb[:, :F].contiguous()              # torch's operands: no channel padding
        base = {"bench": "ridge", "B": B, "C": C, "T": T, "F": F, "L": Lg, "rows": rows, "iters": a.iters, "warmup": a.warmup}
        for what, p, q, pt, qt, Cq in (("gram", xb, xb, xt, xt, C), ("cross", xb, yb, xt, yt, F)):
            slabs = ops.lagged_cov(p, q, Lg, H)
            ours = slabs.sum(dim=0, dtype=torch.float64)[:, :C, :Cq]
            ref = torch_lags(pt.double(), qt.double()) if Cq <= 256 else None            # float64 on the GPU, small shapes only
            theirs = torch_lags(pt, qt)
            k, t = pair(lambda: ops.lagged_cov(p, q, Lg, H, out=slabs), lambda: torch_lags(pt, qt))
            flop = 2.0 * B * T * Lg * C * Cq
            rec = dict(base, line=f"kernel_{what}", what="sda_lagged_cov_f32 alone | one torch fp32 matmul per lag", **r3(k), torch=r3(t),
                       slabs=int(slabs.shape[0]), Ap=int(p.shape[1]), Bp=int(q.shape[1]),
                       useful_tflops=round(flop / (k.mean * 1e-3) / 1e12, 2),
                       share_of_measured_fp32_matrix_rate=round(flop / (k.mean * 1e-3) / 1e12 / FP32_MATRIX_MEASURED_TF, 3),
                       torch_useful_tflops=round(flop / (t.mean * 1e-3) / 1e12, 2), torch_ms_over_ms=round(t.mean / k.mean, 3),
                       max_abs_diff_vs_torch=float((ours - theirs.double()).abs().max()))
            if ref is not None:
                rec["max_abs_err_vs_float64"] = float((ours - ref).abs().max())
                rec["torch_max_abs_err_vs_float64"] = float((theirs.double() - ref).abs().max())
            emit(rec)
            del slabs, ours, ref, theirs
        fit = harness.summarize(harness.rounds(lambda: ridge.partial_fit(X, Y), 1, a.iters, a.warmup))
        pack = harness.summarize(harness.rounds(lambda: (ridge._lag_rows("x", X, ridge.Cp), ridge._lag_rows("y", Y, ridge.Fp)),
                                                1, a.iters, a.warmup))
        emit(dict(base, line="partial_fit", what="partial_fit whole | of it the strided copies into the lag layout", **r3(fit),
                  pack=r3(pack), pack_share=round(pack.mean / fit.mean, 3),
                  segments_per_s=round(B / (fit.mean * 1e-3), 1)))
        host_ms, done_ms = harness.host_clock(lambda: ridge.solve([1.0]), 2, 1)
        emit(dict(base, line="solve", what="solve, one alpha: Gram assembly + Cholesky + substitution, float64", P=Lg * C,
                  ms=round(done_ms, 2), solver=ridge.solver_))
        pred = harness.summarize(harness.rounds(lambda: ridge.predict(X, alpha=0), 1, a.iters, a.warmup))
        pflop = 2.0 * B * T * Lg * C * F
        emit(dict(base, line="predict", what="predict, one alpha: pack + sda_window_gemm_f32 + intercept and (B, F, T) store", **r3(pred),
                  useful_tflops=round(pflop / (pred.mean * 1e-3) / 1e12, 2), segments_per_s=round(B / (pred.mean * 1e-3), 1)))
        del ridge, X, Y, xb, yb, xt, yt
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
