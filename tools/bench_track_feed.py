#!/usr/bin/env python3
"""Time a training batch's speech side gathered from resident TRACKS (sda_gather_windows, ResidentSegmentFeed with a WindowBank)
beside the same batch gathered from the materialised packed table (sda_zero_pad_rows + sda_gather_samples, the pair a step pays
with pack_embeddings), at the workload's shape.

    python tools/bench_track_feed.py [--batch 256] [--segments 4096] [--hop 40] [--tracks 4] [--iters 100] [--out profiles/track_feed_bench.json]

Method.  The materialised table holds the SAME candidates (it is the bank's windows gathered once, checked against a slice here).
Every timed call is bracketed by its own pair of device events after a warm-up; per iteration the order is reference (series
A), new kernel, reference (series B), each with the next of a few pre-uploaded index batches, so the two kernels alternate call
by call and the reference is measured twice in the same run: |mean A - mean B| / mean is the spread the machine shows between
two series of ONE kernel, and the margin the comparison gets.  feed.batch() in both forms is timed with a host clock around the
call and a device synchronise (collate of X, index upload and the gather; the two forms alternate as well).  Bytes are the
compulsory traffic computed from shapes below; the share is of the 8 TB/s HBM3E rate.  Needs the GPU: there is no fallback."""
import argparse
import itertools

import numpy as np
import torch

import harness

HBM_BYTES_PER_S = 8.0e12
ROW_PAD = 16


def gather_windows_bytes(B, T, rows_alloc, row_bytes):
    """(read, written): T table rows per sample in; every row of the destination out, once."""
    return B * T * row_bytes, rows_alloc * row_bytes


def gather_samples_bytes(B, T, rows_alloc, row_bytes):
    """(read, written) of sda_zero_pad_rows + sda_gather_samples: whole samples in, pad rows included; every sample row out, and
    the pad rows and the slack zeroed by the launch in front (the pad rows are written twice)."""
    return B * (T + ROW_PAD) * row_bytes, (B * (T + ROW_PAD) + B * ROW_PAD + (rows_alloc - B * (T + ROW_PAD))) * row_bytes


def stats(ms):
    s = harness.us(harness.summarize(ms))
    return {"mean_us": s.mean, "median_us": s.median, "min_us": s.min, "max_us": s.max, "calls": s.n}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=256)
    ap.add_argument("--segments", type=int, default=4096)
    ap.add_argument("--hop", type=int, default=40)
    ap.add_argument("--tracks", type=int, default=4)
    ap.add_argument("--iters", type=int, default=100)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if a.iters < 20:
        raise SystemExit("bench_track_feed: --iters must be at least 20")
    harness.need_gpu()
    from speech_decoding_amd import lib as L, load_config, ops
    from speech_decoding_amd.data import ResidentSegmentFeed, synthetic_track_dataset
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    dtype = torch.bfloat16
    args = load_config(overrides=["dataset=Gwilliams2022", "num_subjects=27"])
    B, N = a.batch, a.segments
    feed, _, _ = synthetic_track_dataset(args, dev, n_segments=N, dtype=dtype, n_tasks=a.tracks, seed=1234, hop=a.hop)
    bank = feed.Y
    F, T, Cp = bank.F, bank.T, bank.row_elems
    assert (F, T) == (1024, 360), (F, T)
    row_bytes, rows = Cp * 2, L.rows_alloc(B, T)
    lib = L.load()
    st = torch.cuda.current_stream().cuda_stream

    # the same candidates materialised: the packed table of pack_embeddings (N samples of (T + 16) x Cp, then slack)
    packed = ops.gather_windows(bank.table, bank.starts, torch.arange(N, device=dev), N, T)
    for i in (0, N // 2 + 1, N - 1):
        s = int(bank.starts_host[i])
        assert torch.equal(packed[i * (T + ROW_PAD) + ROW_PAD: (i + 1) * (T + ROW_PAD)], bank.table[s: s + T])
    Y32 = ops.unpack_rows(packed, N, F, T)                        # the (N, F, T) fp32 original the materialised feed also keeps
    rs = feed.rs
    mat = ResidentSegmentFeed(rs.sessions, feed.rec_subject, feed.rec_task, feed.onsets, feed.seg_task, feed.seg_in_task, Y32,
                              seq_len_samp=rs.T, baseline_len_samp=rs.nb, clamp_lim=rs.lim, clamp=rs.clamp, seed=1234 + 17)
    mat.pack_embeddings(dtype)
    assert torch.equal(mat._Yt.view(torch.int16), packed.view(torch.int16))
    del packed
    table_m = mat._Yt

    rng = np.random.RandomState(0)
    host_idx = [rng.randint(0, N, size=B).astype(np.int64) for _ in range(8)]
    dev_idx = [torch.from_numpy(i).to(dev) for i in host_idx]
    dst_w = torch.empty((rows, Cp), dtype=dtype, device=dev)
    dst_s = torch.empty((rows, Cp), dtype=dtype, device=dev)
    sample_bytes = (T + ROW_PAD) * row_bytes

    def new(idx):
        L.check(lib.sda_gather_windows(bank.table.data_ptr(), bank.table.shape[0], bank.starts.data_ptr(), len(bank), idx.data_ptr(),
                                       dst_w.data_ptr(), B, T, row_bytes, st), "gather_windows")

    def reference(idx):
        L.check(lib.sda_zero_pad_rows(dst_s.data_ptr(), B, T, Cp, L.BF16, st), "zero_pad_rows")
        L.check(lib.sda_gather_samples(table_m.data_ptr(), idx.data_ptr(), dst_s.data_ptr(), B, sample_bytes, st), "gather_samples")

    new(dev_idx[0]); reference(dev_idx[0])
    torch.cuda.synchronize()
    assert torch.equal(dst_w.view(torch.int16), dst_s.view(torch.int16))        # the two paths hand the loss the same bytes

    # A / new / A again, every call on the next of the index sets, the GPU kept fed (the brackets are read at the end)
    idx = itertools.cycle(dev_idx)
    order = [lambda: reference(next(idx)), lambda: new(next(idx)), lambda: reference(next(idx))]
    series = dict(zip(("reference_A", "gather_windows", "reference_B"), harness.alternating(order, a.iters, a.warmup, sync_each=False)))

    # feed.batch() ends in the host's wait for its batch: the host's clock around every single call, the two feeds taking turns
    feed_ms = {"tracks": [], "materialised": []}
    for it in range(a.warmup + a.iters):
        for name, f in (("tracks", feed), ("materialised", mat)):
            ms = harness.host_clock(lambda: f.batch(host_idx[it % len(host_idx)]), 1, 0)[1]
            if it >= a.warmup:
                feed_ms[name].append(ms)

    rd_w, wr_w = gather_windows_bytes(B, T, rows, row_bytes)
    rd_s, wr_s = gather_samples_bytes(B, T, rows, row_bytes)
    A, Bs, W = stats(series["reference_A"]), stats(series["reference_B"]), stats(series["gather_windows"])
    ref_mean = 0.5 * (A["mean_us"] + Bs["mean_us"])
    spread = abs(A["mean_us"] - Bs["mean_us"]) / ref_mean
    rate_w, rate_s = (rd_w + wr_w) / (W["mean_us"] * 1e-6), (rd_s + wr_s) / (ref_mean * 1e-6)
    result = {
        "device": torch.cuda.get_device_name(0),
        "shape": {"B": B, "T": T, "F": F, "Cp": Cp, "dtype": "bf16", "tracks": a.tracks, "hop": a.hop, "N": N, "table_rows": int(bank.table.shape[0])},
        "iters": a.iters, "warmup": a.warmup,
        "gather_windows": dict(W, bytes_read=rd_w, bytes_written=wr_w, bytes_per_s=rate_w, share_of_hbm_rate=rate_w / HBM_BYTES_PER_S),
        "zero_pad_rows_plus_gather_samples": {"series_A": A, "series_B": Bs, "mean_us": ref_mean, "bytes_read": rd_s, "bytes_written": wr_s,
                                              "bytes_per_s": rate_s, "share_of_hbm_rate": rate_s / HBM_BYTES_PER_S},
        "aa_spread": spread,
        "new_over_reference": W["mean_us"] / ref_mean,
        "inside_margin": bool(W["mean_us"] <= ref_mean * (1.0 + spread)),
        "feed_batch": {k: stats(v) for k, v in feed_ms.items()},
        "resident_bytes": {"tracks": int(bank.nbytes),
                           "materialised": {"packed_table": int(table_m.numel() * 2), "segments_fp32": int(Y32.numel() * 4)}},
    }
    print(f"sda_gather_windows              {W['mean_us']:9.1f} us mean ({W['median_us']:.1f} median, {W['min_us']:.1f} min)  {rate_w / 1e12:6.2f} TB/s  "
          f"{100 * rate_w / HBM_BYTES_PER_S:5.1f} % of 8 TB/s")
    print(f"zero_pad_rows + gather_samples  {ref_mean:9.1f} us mean (A {A['mean_us']:.1f}, B {Bs['mean_us']:.1f}: spread {100 * spread:.2f} %)  "
          f"{rate_s / 1e12:6.2f} TB/s  {100 * rate_s / HBM_BYTES_PER_S:5.1f} % of 8 TB/s")
    print(f"new / reference = {result['new_over_reference']:.4f}; inside the A/A margin: {result['inside_margin']}")
    for k, v in result["feed_batch"].items():
        print(f"feed.batch() {k:13s} {v['mean_us']:9.1f} us mean ({v['median_us']:.1f} median)")
    print(f"resident: tracks {bank.nbytes / 1e9:.3f} GB; materialised {table_m.numel() * 2 / 1e9:.3f} GB packed + {Y32.numel() * 4 / 1e9:.3f} GB fp32")
    harness.emit(result, a.out)


if __name__ == "__main__":
    main()
