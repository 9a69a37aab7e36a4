"""Micro-benchmark of the 1x1 convs of the step (diagnostic): conv_final1/2 forward and data gradient, SubjectBlock GEMM."""
import math

import torch

from harness import need_gpu, us, window
from speech_decoding_amd import lib as L, ops


def main():
    need_gpu()
    dev, dtype = "cuda:0", torch.bfloat16
    B, T = 256, 360
    for name, cin, cout, gelu, pre, widx in [("x0 (composed SubjectBlock)", 256, 320, False, False, True), ("conv_final1 fwd", 320, 640, True, True, False),
                                             ("conv_final2 fwd", 640, 1024, True, True, False), ("conv_final2 dgrad", 1024, 640, False, False, False),
                                             ("conv_final1 dgrad", 640, 320, False, False, False)]:
        x = ops.new_rows(B, T, cin, dtype, dev); x.normal_()
        S = 27 if widx else 1
        w = torch.randn(S, cout, cin, 1, device=dev) / math.sqrt(cin)
        wp = ops.pack_conv_weight(w, cout, cin, dtype)
        y, yp = ops.new_rows(B, T, cout, dtype, dev), ops.new_rows(B, T, cout, dtype, dev)
        bias = torch.zeros(cout, device=dev)
        idx = torch.randint(0, S, (B,), dtype=torch.int32, device=dev) if widx else None
        fl = 2.0 * B * T * cin * cout
        mb = B * T * (cin + cout * (2 if pre else 1)) * 2 / 1e6
        for tag, flags in (("single", 0), ("paired", L.CONV_PAIR_TILES)):
            if widx and flags:
                continue
            t = us(window(lambda: ops.conv_gemm(x, wp, y, B=B, T=T, KS=1, dil=0, bias=bias, gelu=gelu, y_pre=yp if pre else None, widx=idx, flags=flags), 20, 3))
            print(f"{name:28s} {cin:4d}->{cout:4d} {tag:7s} {t:7.1f} us  {fl / t / 1e6:6.1f} TF  {mb:5.0f} MB  {mb / t:5.2f} TB/s", flush=True)


if __name__ == "__main__":
    main()
