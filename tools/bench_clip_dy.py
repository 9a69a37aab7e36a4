"""CLIPLoss forward + backward with and without a gradient for the speech embeddings (x), and the speech-side gradient's parts
alone: the coefficient kernel (sda_clip_grad_y + its finisher), the dY GEMM beside the dZ GEMM it mirrors, and the typed
unpack.  Device events after warm-up.  Diagnostic; not part of the product.

    python tools/bench_clip_dy.py [--iters 30] [--json out.json]

Shapes: configs[1] (B = 256, F = 1024, T = 360) in bf16, fp16 and fp32, and 1024 speech rows in bf16.  Z is an encoder-style
row-layout buffer of the compute dtype, x a plain fp32 (B, F, T) tensor (the wav2vec 2.0 features or a speech module's output)."""
import argparse

import torch

from harness import emit, need_gpu, us, window
from speech_decoding_amd import clip, lib as L, ops
from speech_decoding_amd.config import Config


def one(B, F, T, dtype, iters, dev="cuda:0"):
    from speech_decoding.utils.loss import CLIPLoss
    timeit = lambda fn: us(window(fn, iters, 3))
    g = torch.Generator(device=dev).manual_seed(0)
    Cp = L.pad_channels(F)
    zbuf = ops.new_rows(B, T, Cp, dtype, dev)
    ops.pack_rows(torch.randn(B, F, T, generator=g, device=dev), zbuf)
    zbuf.requires_grad_(True)
    Z = ops.rows_view(zbuf, B, F, T)
    Y = torch.randn(B, F, T, generator=g, device=dev)
    Yg = Y.clone().requires_grad_(True)
    crit = CLIPLoss(Config(reduction="mean", init_temperature=2.0)).to(dev)

    def step(x):
        loss = crit(x, Z)
        loss.backward()
        zbuf.grad = None
        crit.temp.grad = None
        if x.requires_grad:
            x.grad = None

    r = {"B": B, "F": F, "T": T, "dtype": str(dtype).replace("torch.", "")}
    r["loss_fwd_bwd_us"] = timeit(lambda: step(Y))
    r["loss_fwd_bwd_with_dx_us"] = timeit(lambda: step(Yg))
    r["extra_us"] = r["loss_fwd_bwd_with_dx_us"] - r["loss_fwd_bwd_us"]
    # the parts alone, on the context of one forward
    Yt = ops.new_rows(B, T, Cp, dtype, dev)
    ops.pack_rows(Y, Yt)
    Zt = zbuf.detach()
    temp = crit.temp.detach()
    _, _, _, c = clip.clip_forward(Yt, Zt, temp, Bm=B, Bn=B, T=T)

    def coefs():
        Gy, part = ops.clip_grad_y(c.logits, c.row_lse, c.col_lse, c.zsq, c.zsq, 0, dtype)
        return Gy, ops.clip_grad_y_finish(part, c.ysq, c.zsq, temp, c.inv_norm, 0, B)

    r["coef_us"] = timeit(coefs)
    Gy, (rs, cs) = coefs()
    out = ops.new_rows_uninit(B, T, Cp, dtype, dev)
    r["dy_gemm_us"] = timeit(lambda: ops.clip_dz(Gy, Zt, Yt, out, rs, cs, Bm=B, Bn=B, row_elems=c.row_elems))
    r["dz_gemm_us"] = timeit(lambda: ops.clip_dz(c.G, Yt, Zt, out, c.rscale, c.cscale, Bm=B, Bn=B, row_elems=c.row_elems))
    r["dy_over_dz"] = r["dy_gemm_us"] / r["dz_gemm_us"]
    r["unpack_us"] = timeit(lambda: ops.unpack_rows(out, B, F, T))
    moved = B * F * T * (torch.finfo(dtype).bits // 8 + 4)             # read the valid stored elements, write fp32
    r["unpack_TBps"] = moved / (r["unpack_us"] * 1e-6) / 1e12
    crit.release_buffers()
    return r


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=30)
    ap.add_argument("--json", default=None)
    a = ap.parse_args()
    need_gpu()
    shapes = [(256, 1024, 360, dt) for dt in (torch.bfloat16, torch.float16, torch.float32)] + [(1024, 1024, 360, torch.bfloat16)]
    for shape in shapes:
        emit(one(*shape, a.iters), a.json, append=True, digits=3)


if __name__ == "__main__":
    main()
