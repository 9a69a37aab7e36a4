"""The 1x1 convs of the step with their epilogue added piece by piece (diagnostic): plain, + GELU, + pre-activation, + stats."""
import math

import torch

from harness import need_gpu, us, window
from speech_decoding_amd import ops


def main():
    need_gpu()
    dev, dtype = "cuda:0", torch.bfloat16
    B, T = 256, 360
    for name, cin, cout in [("f2 fwd", 640, 1024), ("f2 dgrad", 1024, 640), ("f1 fwd", 320, 640)]:
        x = ops.new_rows(B, T, cin, dtype, dev); x.normal_()
        w = torch.randn(1, cout, cin, 1, device=dev) / math.sqrt(cin)
        wp = ops.pack_conv_weight(w, cout, cin, dtype)
        y, yp = ops.new_rows(B, T, cout, dtype, dev), ops.new_rows(B, T, cout, dtype, dev)
        bias = torch.zeros(cout, device=dev)
        stats = torch.empty((B * ops.n_t_tiles(T), 2, cout), device=dev)
        fl = 2.0 * B * T * cin * cout
        for tag, kw in [("gelu+pre+stats", dict(bias=bias, gelu=True, y_pre=yp, stats=stats)), ("gelu+pre", dict(bias=bias, gelu=True, y_pre=yp)),
                        ("gelu", dict(bias=bias, gelu=True)), ("plain", dict())]:
            t = us(window(lambda: ops.conv_gemm(x, wp, y, B=B, T=T, KS=1, dil=0, **kw), 20, 3))
            print(f"{name:10s} {tag:16s} {t:7.1f} us {fl/t/1e6:7.1f} TF", flush=True)


if __name__ == "__main__":
    main()
