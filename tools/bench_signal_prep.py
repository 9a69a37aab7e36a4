"""Times the signal-conditioning path (speech_decoding_amd/signal_prep.py on csrc/window_gemm.hip) on the MI355X at the shapes the
datasets have: one Gwilliams2022 recording (208 channels x 396 000 samples at 1 kHz) through the 1-60 Hz band-pass (3301 taps),
the same filter through torch.nn.functional.conv1d on the same device and through scipy.signal.oaconvolve on the host's CPUs
(16 threads, float64, as mne computes it), 60 s of 44.1 kHz audio to 16 kHz, and brain_preproc end to end.

    python tools/bench_signal_prep.py [--only filter conv1d cpu audio brain] [--rows 208] [--samples 396000] [--out FILE]

Device events after warm-up; every line is one JSON object, printed and appended to --out (kept as
profiles/signal_prep_bench.json), times in milliseconds per call.  "useful" FLOP = 2 rows L K: the taps, not the zeros the
grouped matrix adds.  The share of peak is against the 157.3 TFLOP/s fp32 matrix rate, which bounds this kernel."""
import argparse

import harness

FP32_MATRIX_PEAK_TF = 157.3
LINES = ("filter", "conv1d", "cpu", "audio", "brain")


def timed(fn, iters, warmup):
    """every call between its own pair of events: (mean, min, max) in ms"""
    s = harness.summarize(harness.alternating((fn,), iters, warmup)[0])
    return s.mean, s.min, s.max


def padded_recording(rows, n, K, seed=0):
    """the odd-padded rows fir_filter builds, fp32 on the device, and the raw rows"""
    import torch
    g = torch.Generator(device="cuda:0").manual_seed(seed)
    x = torch.randn((rows, n), generator=g, device="cuda:0")
    pad = (K - 1) // 2
    left = 2 * x[:, :1] - x[:, 1:pad + 1].flip(-1)
    right = 2 * x[:, -1:] - x[:, n - 1 - pad:n - 1].flip(-1)
    return x, torch.cat([left, x, right], dim=1).contiguous()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--only", nargs="+", default=list(LINES), choices=LINES)
    ap.add_argument("--rows", type=int, default=208)
    ap.add_argument("--samples", type=int, default=396000)
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import numpy as np
    import torch
    from speech_decoding_amd import signal_prep as SP
    harness.need_gpu()
    rows, n = a.rows, a.samples
    taps = SP.bandpass_taps(1000, 1.0, 60)
    K = len(taps)
    flop = 2.0 * rows * n * K
    base = {"bench": "signal_prep", "rows": rows, "samples": n, "taps": K, "iters": a.iters, "warmup": a.warmup}

    def emit(rec):
        harness.emit(dict(base, **rec), a.out, append=True)

    x, xp = padded_recording(rows, n, K)
    h32 = torch.from_numpy(taps.astype(np.float32)).to("cuda:0")

    def cpu_rows(r):
        """float64 reference of the first r rows by oaconvolve on the host"""
        from scipy.signal import oaconvolve
        return oaconvolve(xp[:r].cpu().double().numpy(), taps[None, :], mode="valid", axes=-1)

    if "filter" in a.only:
        G = SP.window_group(1, 1, K)
        Bm = torch.from_numpy(SP.window_matrix(taps[::-1][None, :].copy(), 1, G).astype(np.float32)).to("cuda:0")
        groups = -(-n // G)
        need = (groups - 1) * G + Bm.shape[0]
        xz = torch.cat([xp, xp.new_zeros(rows, max(need - xp.shape[1], 0))], dim=1).contiguous()
        mean, lo, hi = timed(lambda: SP.window_gemm(xz, Bm, groups, G), a.iters, a.warmup)
        y = SP.window_gemm(xz, Bm, groups, G)[:, :n]
        ref = cpu_rows(2)
        emit({"line": "filter_kernel", "what": "sda_window_gemm_f32 alone (device events)", "G": G, "K_grouped": Bm.shape[0],
              "kernel_ms": round(mean, 3), "min_ms": round(lo, 3), "max_ms": round(hi, 3),
              "useful_tflops": round(flop / (mean * 1e-3) / 1e12, 2),
              "share_of_fp32_matrix_peak": round(flop / (mean * 1e-3) / 1e12 / FP32_MATRIX_PEAK_TF, 3),
              "issued_tflops": round(2.0 * rows * groups * Bm.shape[0] * Bm.shape[1] / (mean * 1e-3) / 1e12, 2),
              "max_abs_diff_vs_cpu_float64_2_rows": float(np.abs(y[:2].cpu().double().numpy() - ref).max())})
        mean, lo, hi = timed(lambda: SP.fir_filter(x, taps), a.iters, a.warmup)
        emit({"line": "fir_filter", "what": "fir_filter(): padding, matrix upload, kernel, slice", "ms": round(mean, 3),
              "min_ms": round(lo, 3), "max_ms": round(hi, 3)})
    if "conv1d" in a.only:
        w = h32.flip(0).view(1, 1, K)
        xin = xp.view(rows, 1, -1)
        try:
            mean, lo, hi = timed(lambda: torch.nn.functional.conv1d(xin, w), min(a.iters, 3), 1)
            y = torch.nn.functional.conv1d(xin[:2], w)[:, 0]
            emit({"line": "conv1d", "what": "torch.nn.functional.conv1d, same padded rows and taps, fp32", "ms": round(mean, 3),
                  "min_ms": round(lo, 3), "max_ms": round(hi, 3), "useful_tflops": round(flop / (mean * 1e-3) / 1e12, 2),
                  "max_abs_diff_vs_cpu_float64_2_rows": float(np.abs(y.cpu().double().numpy() - cpu_rows(2)).max())})
        except RuntimeError as e:
            emit({"line": "conv1d", "error": str(e)[:200]})
    if "cpu" in a.only:
        from concurrent.futures import ThreadPoolExecutor
        from scipy.signal import oaconvolve
        threads = 16
        xh = xp.cpu().double().numpy()
        parts = np.array_split(np.arange(rows), threads)

        def run():
            with ThreadPoolExecutor(threads) as ex:
                return list(ex.map(lambda idx: oaconvolve(xh[idx], taps[None, :], mode="valid", axes=-1), [p for p in parts if len(p)]))
        ms = harness.host_clock(run, 2, 1)[1]
        emit({"line": "cpu_oaconvolve", "what": "scipy.signal.oaconvolve, float64, 16 threads over the rows, host clock", "threads": threads,
              "ms": round(ms, 1), "useful_tflops": round(flop / (ms * 1e-3) / 1e12, 3)})
    if "audio" in a.only:
        sec, sr = 60, 44100
        wave = torch.randn(1, sec * sr, device="cuda:0")
        bank, width, orig, new = SP.sinc_resample_bank(sr, 16000, 128)
        mean, lo, hi = timed(lambda: SP.resample_audio(wave, sr, 16000, lowpass_filter_width=128), a.iters, a.warmup)
        Bm = torch.from_numpy(bank.T.astype(np.float32).copy()).to("cuda:0")
        frames = wave.shape[1] // orig + 1
        xa = torch.cat([wave.new_zeros(1, width), wave, wave.new_zeros(1, width + orig)], dim=1).contiguous()
        kmean, klo, khi = timed(lambda: SP.window_gemm(xa, Bm, frames, orig), a.iters, a.warmup)
        aflop = 2.0 * frames * new * bank.shape[1]
        emit({"line": "audio_resample", "what": "60 s of 44.1 kHz -> 16 kHz, lowpass_filter_width 128", "phases": new, "taps_per_phase": bank.shape[1],
              "resample_audio_ms": round(mean, 3), "kernel_ms": round(kmean, 4), "kernel_min_ms": round(klo, 4), "kernel_max_ms": round(khi, 4),
              "useful_tflops": round(aflop / (kmean * 1e-3) / 1e12, 2)})
    if "brain" in a.only:
        pre = {"brain_filter_low": 1.0, "brain_filter_high": 60, "brain_resample_rate": 120}
        mean, lo, hi = timed(lambda: SP.brain_preproc(x, 1000, pre), min(a.iters, 5), 2)
        emit({"line": "brain_preproc", "what": "filter_data + resample_fft (float64 FFT) + fp32, one recording end to end",
              "ms": round(mean, 3), "min_ms": round(lo, 3), "max_ms": round(hi, 3),
              "out_shape": list(SP.brain_preproc(x, 1000, pre).shape)})


if __name__ == "__main__":
    main()
