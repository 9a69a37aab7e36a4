"""Times the log-mel path (speech_decoding_amd/signal_prep.py: stft on csrc/window_gemm.hip or, algorithm="fft", on
csrc/stft_fft.hip, then csrc/mel_power.hip) on the MI355X at the paper's setting — 60 s of 16 kHz audio, n_fft 512, hop 128, 120
mel bands, log(1e-5 + mel) — for one row and for a batch of 32 rows: the STFT window GEMM alone, `sda_mel_power_f32` alone,
`log_mel()` whole, the STFT FFT kernel `sda_stft_fft_f32` alone and `log_mel(algorithm="fft")` whole, and beside each of them
`torch.stft` + `matmul` + `log` on the same GPU, the two alternating call by call.

    python tools/bench_mel.py [--rows 1 32] [--seconds 60] [--out FILE]

Device events after warm-up; every line is one JSON object, printed and appended to --out (kept as profiles/mel_bench.json),
times in milliseconds per call.  The mel kernel's bytes = the spectrum read once, the filterbank once and the output written
once; its share of peak is against the 8 TB/s HBM rate (MI355X data sheet), its FLOP = 2 rows frames n_freqs n_mels.  The FFT
kernel's bytes = the padded rows read once and the spectrum written once: rows (padded samples + frames 2 n_freqs) 4."""
import argparse
import warnings

import harness

HBM_PEAK_TBS = 8.0
FP32_MATRIX_PEAK_TF = 157.3


def timed_pair(fa, fb, iters, warmup):
    """fa and fb alternating, each call between its own pair of events: ((mean, min, max) of fa, of fb)"""
    return tuple((s.mean, s.min, s.max) for s in map(harness.summarize, harness.alternating((fa, fb), iters, warmup)))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, nargs="+", default=[1, 32])
    ap.add_argument("--seconds", type=int, default=60)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import numpy as np
    import torch
    from speech_decoding_amd import ops
    from speech_decoding_amd import signal_prep as SP
    harness.need_gpu()
    sr, n_fft, hop, n_mels, eps = 16000, 512, 128, 120, 1e-5
    n_freqs = n_fft // 2 + 1
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        fb64 = SP.mel_filterbank(n_freqs, 0.0, sr / 2, n_mels, sr)
    fb = torch.from_numpy(fb64.astype(np.float32)).to("cuda:0")
    Bm = torch.from_numpy(SP.stft_matrix(n_fft).astype(np.float32)).to("cuda:0")
    wd = torch.from_numpy(SP.stft_window(n_fft).astype(np.float32)).to("cuda:0")
    twd = torch.from_numpy(SP.fft_twiddles(n_fft).astype(np.float32)).to("cuda:0")
    window = torch.hann_window(n_fft, device="cuda:0")
    wnorm = float(window.pow(2).sum().sqrt())

    def emit(rec):
        harness.emit(rec, a.out, append=True)

    for rows in a.rows:
        n = a.seconds * sr
        wave = torch.randn(rows, n, generator=torch.Generator(device="cuda:0").manual_seed(rows), device="cuda:0")
        frames = 1 + n // hop
        p = n_fft // 2
        xp = torch.cat([wave[:, 1:p + 1].flip(-1), wave, wave[:, n - 1 - p:n - 1].flip(-1)], dim=1).contiguous()
        base = {"bench": "mel", "rows": rows, "samples": n, "frames": frames, "n_fft": n_fft, "hop": hop, "n_mels": n_mels,
                "iters": a.iters, "warmup": a.warmup}

        def torch_spec():
            return torch.stft(wave, n_fft, hop, window=window, center=True, pad_mode="reflect", return_complex=True) / wnorm

        def torch_mel(s):
            return torch.log(eps + torch.matmul(s.real.square().add_(s.imag.square()).transpose(-1, -2), fb).transpose(-1, -2))

        try:
            spec_t = torch_spec()
        except RuntimeError as e:
            emit(dict(base, line="torch", error=str(e)[:200]))
            continue
        spec = SP.window_gemm(xp, Bm, frames, hop).reshape(rows, frames, n_freqs, 2)
        ours = SP.log_mel(wave)
        ref = torch_mel(spec_t)
        (k_stft, t_stft) = timed_pair(lambda: SP.window_gemm(xp, Bm, frames, hop), torch_spec, a.iters, a.warmup)
        (k_mel, t_mel) = timed_pair(lambda: ops.mel_power(spec, fb, eps), lambda: torch_mel(spec_t), a.iters, a.warmup)
        (k_all, t_all) = timed_pair(lambda: SP.log_mel(wave), lambda: torch_mel(torch_spec()), a.iters, a.warmup)
        spec_f = ops.stft_fft(xp, wd, twd, frames, hop, n_fft)
        ours_f = SP.log_mel(wave, algorithm="fft")
        (k_fft, t_fft) = timed_pair(lambda: ops.stft_fft(xp, wd, twd, frames, hop, n_fft), torch_spec, a.iters, a.warmup)
        (k_allf, t_allf) = timed_pair(lambda: SP.log_mel(wave, algorithm="fft"), lambda: torch_mel(torch_spec()), a.iters, a.warmup)
        sflop = 2.0 * rows * frames * n_fft * 2 * n_freqs
        fbytes = 4.0 * rows * (xp.shape[1] + frames * 2 * n_freqs)
        mbytes = 4.0 * (rows * frames * (2 * n_freqs + n_mels) + n_freqs * n_mels)
        mflop = 2.0 * rows * frames * n_freqs * n_mels

        def r3(t):
            return {"ms": round(t[0], 4), "min_ms": round(t[1], 4), "max_ms": round(t[2], 4)}
        emit(dict(base, line="stft_kernel", what="sda_window_gemm_f32 alone, S 128, K 512, N 514 | torch.stft / window norm", **r3(k_stft),
                  torch=r3(t_stft), useful_tflops=round(sflop / (k_stft[0] * 1e-3) / 1e12, 2),
                  share_of_fp32_matrix_peak=round(sflop / (k_stft[0] * 1e-3) / 1e12 / FP32_MATRIX_PEAK_TF, 3)))
        emit(dict(base, line="mel_kernel", what="sda_mel_power_f32 alone | re^2 + im^2, matmul with fb, log in torch", **r3(k_mel),
                  torch=r3(t_mel), bytes=int(mbytes), tb_per_s=round(mbytes / (k_mel[0] * 1e-3) / 1e12, 3),
                  share_of_hbm_peak=round(mbytes / (k_mel[0] * 1e-3) / 1e12 / HBM_PEAK_TBS, 3),
                  tflops=round(mflop / (k_mel[0] * 1e-3) / 1e12, 2)))
        emit(dict(base, line="log_mel", what="log_mel() whole: padding, matrix uploads, both kernels | torch.stft + matmul + log", **r3(k_all),
                  torch=r3(t_all), max_abs_diff_vs_torch=float((ours - ref).abs().max()),
                  out_shape=list(ours.shape)))
        emit(dict(base, line="stft_fft_kernel", what="sda_stft_fft_f32 alone | torch.stft / window norm", **r3(k_fft), torch=r3(t_fft),
                  bytes=int(fbytes), tb_per_s=round(fbytes / (k_fft[0] * 1e-3) / 1e12, 3),
                  share_of_hbm_peak=round(fbytes / (k_fft[0] * 1e-3) / 1e12 / HBM_PEAK_TBS, 3),
                  stft_kernel_ms_over_ms=round(k_stft[0] / k_fft[0], 2), torch_ms_over_ms=round(t_fft[0] / k_fft[0], 3),
                  max_abs_diff_vs_stft_kernel=float((spec_f - spec).abs().max())))
        emit(dict(base, line="log_mel_fft", what="log_mel(algorithm='fft') whole: padding, both kernels | torch.stft + matmul + log",
                  **r3(k_allf), torch=r3(t_allf), log_mel_ms_over_ms=round(k_all[0] / k_allf[0], 2),
                  torch_ms_over_ms=round(t_allf[0] / k_allf[0], 3), max_abs_diff_vs_torch=float((ours_f - ref).abs().max()),
                  max_abs_diff_vs_log_mel=float((ours_f - ours).abs().max()), out_shape=list(ours_f.shape)))


if __name__ == "__main__":
    main()
