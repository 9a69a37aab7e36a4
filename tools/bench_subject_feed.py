#!/usr/bin/env python3
"""Time Brennan2018's input path on the device at the dataset's shape: the whole-recording robust statistics
(sda_robust_stats), the scale + clamp pass (sda_scale_clamp_rows) and a batch gather (sda_gather_baseline_windows), for both
`subject_wise` modes, next to sklearn's RobustScaler on the host cores (when sklearn is installed) as the baseline.

    python tools/bench_subject_feed.py [--subjects 33] [--channels 60] [--length 87000] [--iters 20] [--out profiles/subject_feed_bench.json]

Prints microseconds and achieved bytes/s per stage (bytes = the compulsory traffic: one read of the recording for the
statistics, one read and one write for the scaling, one read and one write of the batch for the gather) and one JSON line.
No threshold: nobody had measured these when the path was written."""
import argparse
import time

import numpy as np
import torch

import harness
from speech_decoding_amd import collate


def time_us(fn, iters):
    return harness.us(harness.window(fn, iters, 3))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--subjects", type=int, default=33)
    ap.add_argument("--channels", type=int, default=60)
    ap.add_argument("--length", type=int, default=87000)
    ap.add_argument("--seg", type=int, default=360)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--host-baseline", action="store_true", help="also time sklearn's RobustScaler on the host")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    harness.need_gpu()
    dev = torch.device("cuda", 0)
    S, C, Ln, T = a.subjects, a.channels, a.length // a.seg * a.seg, a.seg
    g = torch.Generator().manual_seed(0)
    X = (torch.randn(S, C, Ln, generator=g) * 10.0 ** (2 * torch.rand(S, C, 1, generator=g) - 1)).to(dev)
    nbytes = X.numel() * 4
    rows = []
    for subject_wise in (True, False):
        pooled = not subject_wise
        centre, scale = collate.robust_stats(X, pooled=pooled)
        out = torch.empty_like(X)
        t_stats = time_us(lambda: collate.robust_stats(X, pooled=pooled), a.iters)
        t_scale = time_us(lambda: collate.scale_clamp_rows(X, centre, scale, 20.0, True, pooled=pooled, out=out), a.iters)
        rows.append({"stage": "robust_stats", "subject_wise": subject_wise, "us": t_stats, "bytes_per_s": nbytes / (t_stats * 1e-6)})
        rows.append({"stage": "scale_clamp_rows", "subject_wise": subject_wise, "us": t_scale, "bytes_per_s": 2 * nbytes / (t_scale * 1e-6)})
        if a.host_baseline:
            try:
                from sklearn.preprocessing import RobustScaler
            except ImportError:
                RobustScaler = None
            if RobustScaler is not None:
                Xh = X.cpu().numpy()
                t0 = time.perf_counter()
                if subject_wise:
                    for s in range(S):
                        RobustScaler().fit_transform(Xh[s].T)
                else:
                    RobustScaler().fit_transform(np.ascontiguousarray(Xh.transpose(2, 0, 1)).reshape(-1, C))
                rows.append({"stage": "sklearn RobustScaler (host)", "subject_wise": subject_wise, "us": (time.perf_counter() - t0) * 1e6,
                             "bytes_per_s": None})
    rng = np.random.RandomState(0)
    for B in (64, 256):
        sub, on = rng.randint(0, S, size=B), rng.randint(0, Ln // T, size=B) * T
        t = time_us(lambda: collate.gather_baseline_windows(X, sub, on, T, T // 6), a.iters)
        rows.append({"stage": "gather_baseline_windows", "B": B, "T": T, "us": t, "bytes_per_s": 2 * B * C * T * 4 / (t * 1e-6)})
    for r in rows:
        rate = "" if r["bytes_per_s"] is None else f"{r['bytes_per_s'] / 1e9:9.1f} GB/s"
        tag = f"subject_wise={r['subject_wise']}" if "subject_wise" in r else f"B={r['B']} T={r['T']}"
        print(f"{r['stage']:32s} {tag:20s} {r['us']:12.1f} us {rate}")
    result = {"shape": [S, C, Ln], "device": torch.cuda.get_device_name(0), "rows": rows}
    harness.emit(result, a.out)


if __name__ == "__main__":
    main()
