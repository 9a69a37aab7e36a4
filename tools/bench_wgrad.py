"""Micro-benchmark of wgrad_gemm alone at the config-2 shapes of the training step (diagnostic): the kernel-3 weight gradients,
the two 1x1 ones (conv_final1 / conv_final2) and the loss's dZ product."""
import os

import torch

from harness import need_gpu, us, window
from speech_decoding_amd import clip, layers, lib as L, ops


def main():
    need_gpu()
    dev = "cuda:0"
    B, T = 256, 360
    dt = torch.float32 if os.environ.get("DTYPE") == "fp32" else torch.bfloat16
    target = layers.WGRAD_TARGET_WGS
    for (cin, cout, KS, dil, wgs) in [(320, 320, 3, 4, 256), (320, 320, 3, 4, 512), (320, 640, 3, 2, 256), (320, 640, 3, 2, 512),
                                      (640, 1024, 1, 0, 256), (640, 1024, 1, 0, 512), (320, 640, 1, 0, 256), (256, 320, 3, 1, 256)]:
        x = ops.new_rows(B, T, cin, dt, dev); x.normal_()
        dy = ops.new_rows(B, T, cout, dt, dev); dy.normal_()
        tile_n = 64 if KS == 3 else (128 if cin % 128 == 0 else 64)     # the kernel's own column tile
        ntiles = layers.wgrad_ntiles(cout, cin, tile_n)
        try:
            layers.WGRAD_TARGET_WGS = wgs            # (this sweep varies the target the step keeps at 256)
            nseg = layers.uniform_nseg(B, cout, cin, tile_n)
        finally:
            layers.WGRAD_TARGET_WGS = target
        seg = torch.from_numpy(layers.uniform_segment_edges(B, nseg)).to(dev)
        fl = 2.0 * B * T * KS * cin * cout
        t = us(window(lambda: ops.wgrad_gemm(dy, x, B=B, T=T, KS=KS, dil=dil, perm=None, seg_start=seg, nseg=nseg, flat_rows=True), 20, 3))
        print(f"wgrad {cin:4d}->{cout:4d} k{KS} tiles {ntiles:3d} nseg {nseg:3d} ({ntiles * nseg:4d} wgs) {t:8.1f} us  {fl / t / 1e6:7.1f} TF", flush=True)
    F = 1024
    if dt == torch.float32:
        return
    for Bm, Bn in [(256, 256), (2048, 256)]:
        Yt = ops.new_rows(Bm, T, F, dt, dev); Zt = ops.new_rows(Bn, T, F, dt, dev)
        ops.rows_view(Yt, Bm, F, T).normal_(); ops.rows_view(Zt, Bn, F, T).normal_()
        temp = torch.tensor([5.1], device=dev)
        re = L.rows_tp(T) * F
        loss, logits, cnt, ctx = clip.clip_forward(Yt, Zt, temp, Bm=Bm, Bn=Bn, T=T)
        dZ = ops.new_rows(Bn, T, F, dt, dev)
        t = us(window(lambda: clip.clip_backward(ctx, dZ), 20, 3))
        print(f"dZ gemm Bm={Bm} Bn={Bn}: {t:8.1f} us  ({2.0 * Bm * Bn * re / t / 1e6:.0f} TF, {(Bm + 2 * Bn) * re * 2 / t / 1e6:.2f} TB/s algorithmic)", flush=True)
        t = us(window(lambda: ops.matmul_nt_splitk(Yt, Zt, Bm, Bn, re, re), 20, 3))
        print(f"similarity Bm={Bm} Bn={Bn}: {t:8.1f} us  ({2.0 * Bm * Bn * re / t / 1e6:.0f} TF, {(Bm + Bn) * re * 2 / t / 1e6:.2f} TB/s algorithmic)", flush=True)


if __name__ == "__main__":
    main()
