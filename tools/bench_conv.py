"""Micro-benchmark of conv_gemm / wgrad_gemm at config-2 shapes (diagnostic; not part of the product)."""
import math
import os

import torch

from harness import need_gpu, us, window
from speech_decoding_amd import layers, lib as L, ops


def main():
    need_gpu()
    dev = "cuda:0"
    B, T = 256, 360
    for dtype in ((torch.float32,) if os.environ.get("DTYPE") == "fp32" else (torch.bfloat16,)):
        for (cin, cout, KS, dil) in [(320, 320, 3, 4), (320, 640, 3, 2)]:
            x = ops.new_rows(B, T, cin, dtype, dev); x.normal_()
            w = torch.randn(cout, cin, KS, device=dev) / math.sqrt(KS * cin)
            wp = ops.pack_conv_weight(w, cout, cin, dtype)
            y = ops.new_rows(B, T, cout, dtype, dev)
            bias = torch.zeros(cout, device=dev)
            stats = torch.zeros((B * ops.n_t_tiles(T), 2, cout), device=dev)
            res = x if cin == cout else None
            fl = 2.0 * B * T * KS * cin * cout
            for name, kw in [("full", dict(bias=bias, res=res, stats=stats)), ("plain", dict()),
                             ("pair_full", dict(bias=bias, res=res, stats=stats, flags=L.CONV_PAIR_TILES)),
                             ("flat", dict(bias=bias, res=res, stats=stats, flags=L.CONV_FLAT_TILES)),
                             ("flat_plain", dict(flags=L.CONV_FLAT_TILES)),
                             ("flat_stagger", dict(bias=bias, res=res, stats=stats, flags=L.CONV_FLAT_TILES | L.CONV_FLAT_STAGGER))]:
                t = us(window(lambda: ops.conv_gemm(x, wp, y, B=B, T=T, KS=KS, dil=dil, **kw), 20, 3))
                print(f"conv {str(dtype)[6:]:8s} {cin}->{cout} k{KS} {name:28s} {t:8.1f} us  {fl/t/1e6:7.1f} TF", flush=True)
            dy = ops.new_rows(B, T, cout, dtype, dev); dy.normal_()
            nseg = layers.uniform_nseg(B, cout, cin)              # the step's own plan
            seg = torch.from_numpy(layers.uniform_segment_edges(B, nseg)).to(dev)
            perm = torch.arange(B, dtype=torch.int32, device=dev)
            t = us(window(lambda: ops.wgrad_gemm(dy, x, B=B, T=T, KS=KS, dil=dil, perm=perm, seg_start=seg, nseg=nseg), 20, 3))
            print(f"wgrad(perm) {str(dtype)[6:]:8s} {cin}->{cout} k{KS} nseg={nseg:3d} {t:8.1f} us  {fl/t/1e6:7.1f} TF", flush=True)
            t = us(window(lambda: ops.wgrad_gemm(dy, x, B=B, T=T, KS=KS, dil=dil, perm=None, seg_start=seg, nseg=nseg), 20, 3))
            print(f"wgrad {str(dtype)[6:]:8s} {cin}->{cout} k{KS} nseg={nseg:3d} {t:8.1f} us  {fl/t/1e6:7.1f} TF", flush=True)


if __name__ == "__main__":
    main()
