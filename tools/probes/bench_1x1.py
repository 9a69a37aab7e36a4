"""The row-layout 1 x 1 convs of the config-2 step alone (f1, f2 forward; their data gradients) on each tiling.
Diagnostic, not part of the product."""
import math, os, sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))      # tools/: the harness
from harness import need_gpu, us, window
import torch
from speech_decoding_amd import ops, lib as L


def main():
    need_gpu()
    dev, dt = "cuda:0", torch.bfloat16
    B, T = 256, 360
    for (name, cin, cout, fwd) in [("f1 fwd", 320, 640, True), ("f2 fwd", 640, 1024, True), ("f2 dgrad", 1024, 640, False),
                                   ("f1 dgrad", 640, 320, False)]:
        x = ops.new_rows(B, T, cin, dt, dev); x.normal_()
        w = torch.randn(cout, cin, 1, device=dev) / math.sqrt(cin)
        wp = ops.pack_conv_weight(w, cout, cin, dt)
        y, u = ops.new_rows(B, T, cout, dt, dev), ops.new_rows(B, T, cout, dt, dev)
        bias = torch.zeros(cout, device=dev)
        stats = torch.zeros((B * ops.n_t_tiles(T), 2, cout), device=dev)
        full = dict(bias=bias, y_pre=u, gelu=True, stats=stats) if (fwd and cout == 1024) else \
            dict(bias=bias, y_pre=u, gelu=True) if fwd else dict()
        fullf = {k: v for k, v in full.items() if k != "stats"}
        if "stats" in full:
            fullf["row_sumsq"] = torch.zeros((x.shape[0], cout // 128), device=dev)
        fl = 2.0 * B * T * cin * cout
        wr = B * (T + 16) * cout * 2 * (2 if fwd else 1) / 1e6
        rd = B * (T + 16) * cin * 2 / 1e6
        for vn, kw in [("full", full), ("plain", dict()),
                       ("flat", dict(flags=L.CONV_FLAT_TILES, **fullf)), ("flat_plain", dict(flags=L.CONV_FLAT_TILES)),
                       ("flat_1percu", dict(flags=L.CONV_FLAT_TILES | L.CONV_ONE_PER_CU, **fullf))]:
            t = us(window(lambda: ops.conv_gemm(x, wp, y, B=B, T=T, KS=1, dil=0, **kw), 20, 3))
            print(f"{name:9s} {cin:4d}->{cout:4d} {vn:8s} {t:7.1f} us  {fl / t / 1e6:6.1f} TF  (reads {rd:.0f} MB, writes {wr:.0f} MB"
                  f" -> {(rd + wr) / t:.2f} TB/s)", flush=True)


if __name__ == "__main__":
    main()
