"""Micro-benchmark of the loss stages at config-2 (Bm = 256) and config-3 (Bm = 2048, Bn = 256) shapes."""
import torch

from harness import need_gpu, us, window
from speech_decoding_amd import clip, lib as L, ops


def main():
    need_gpu()
    dev = "cuda:0"; T, F = 360, 1024
    timeit = lambda fn: us(window(fn, 10, 2))
    for Bm, Bn in [(256, 256), (2048, 256)]:
        dt = torch.bfloat16
        Yt = ops.new_rows(Bm, T, F, dt, dev); Zt = ops.new_rows(Bn, T, F, dt, dev)
        ops.rows_view(Yt, Bm, F, T).normal_(); ops.rows_view(Zt, Bn, F, T).normal_()
        temp = torch.tensor([5.1], device=dev)
        re = L.rows_tp(T) * F
        print(f"Bm={Bm} Bn={Bn}")
        print("  rows_sumsq(Y) %.1f us" % timeit(lambda: ops.rows_sumsq(Yt, Bm, re, re)))
        print("  sim gemm     %.1f us  (%.0f TF)" % ((t := timeit(lambda: ops.matmul_nt_splitk(Yt, Zt, Bm, Bn, re, re))), 2.0 * Bm * Bn * re / t / 1e6))
        loss, logits, cnt, ctx = clip.clip_forward(Yt, Zt, temp, Bm=Bm, Bn=Bn, T=T)
        print("  clip_forward total %.1f us" % timeit(lambda: clip.clip_forward(Yt, Zt, temp, Bm=Bm, Bn=Bn, T=T)))
        dZ = ops.new_rows(Bn, T, F, dt, dev)
        print("  dZ gemm      %.1f us  (%.0f TF)" % ((t := timeit(lambda: clip.clip_backward(ctx, dZ))), 2.0 * Bm * Bn * re / t / 1e6))
        X = torch.randn(Bn, F, T, device=dev)
        print("  pack_rows(Y local) %.1f us" % timeit(lambda: ops.pack_rows(X, Zt)))


if __name__ == "__main__":
    main()
