"""MSELoss kernels alone at the config-2 shape (B = 256, F = 1024, T = 360): forward and backward time by device events after
warm-up, as effective TB/s over the bytes each must move (valid elements only).  Diagnostic; not part of the product.

    python tools/bench_mse.py [--iters 50] [--json out.json]

Cases: the training one (Z a bf16 row-layout buffer, Y plain fp32), the fp32 one (Z fp32 rows, Y plain fp32), both operands in
row layout (bf16), and a torch copy of the Y tensor as the chip's practical 1 read : 1 write ceiling on the same box."""
import argparse

import torch

from harness import emit, need_gpu, us, window
from speech_decoding_amd import lib as L, ops


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--json", default=None)
    a = ap.parse_args()
    need_gpu()
    dev = "cuda:0"
    B, F, T = 256, 1024, 360
    n = B * F * T
    Cp = L.pad_channels(F)
    g = torch.Generator(device=dev).manual_seed(0)
    Y = torch.randn(B, F, T, generator=g, device=dev)
    dloss = torch.ones(1, device=dev)
    rows = []
    cases = [("Z bf16 rows, Y fp32 plain", torch.bfloat16, False),
             ("Z fp32 rows, Y fp32 plain", torch.float32, False),
             ("Z bf16 rows, Y bf16 rows", torch.bfloat16, True)]
    for name, zdt, y_rows in cases:
        zbuf = ops.new_rows(B, T, Cp, zdt, dev)
        ops.pack_rows(torch.randn(B, F, T, generator=g, device=dev), zbuf)
        if y_rows:
            ybuf = ops.new_rows(B, T, Cp, zdt, dev)
            ops.pack_rows(Y, ybuf)
            yop, ybytes = ybuf, n * torch.finfo(zdt).bits // 8
        else:
            yop, ybytes = Y, n * 4
        zbytes = n * torch.finfo(zdt).bits // 8
        dz = ops.new_rows_uninit(B, T, Cp, zdt, dev)
        fwd_us = us(window(lambda: ops.mse_forward(zbuf, yop, B, F, T, B), a.iters, 5))
        bwd_us = us(window(lambda: ops.mse_backward(zbuf, yop, B, F, T, B, dloss, dz, None), a.iters, 5))
        for kind, t, nbytes in (("forward", fwd_us, zbytes + ybytes), ("backward", bwd_us, 2 * zbytes + ybytes)):
            rows.append(dict(case=name, kind=kind, us=round(t, 1), MB=round(nbytes / 1e6, 1), TBps=round(nbytes / t / 1e6, 3)))
        del zbuf, dz
    out = torch.empty_like(Y)
    t = us(window(lambda: out.copy_(Y), a.iters, 5))
    rows.append(dict(case="torch copy_ of Y (fp32)", kind="copy", us=round(t, 1), MB=round(2 * n * 4 / 1e6, 1),
                     TBps=round(2 * n * 4 / t / 1e6, 3)))
    for r in rows:
        print(f"{r['case']:28s} {r['kind']:9s} {r['us']:8.1f} us {r['MB']:7.1f} MB {r['TBps']:6.3f} TB/s", flush=True)
    if a.json:
        emit(rows, a.json)


if __name__ == "__main__":
    main()
