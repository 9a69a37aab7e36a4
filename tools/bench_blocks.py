"""Times the standalone SpatialAttention, SubjectBlock and ConvBlock calls (forward alone, forward + backward) on the HIP path and
the same math in torch eager on the GPU (the reference's forwards, models.py:45-166, restated below with torch.nn.functional on
copies of the same parameters in the compute dtype), with device events after warm-up.

    python tools/bench_blocks.py [--dtypes bf16 fp32] [--B 256] [--T 360] [--iters 20] [--warmup 5]

Shapes default to config 2 (C = 208, S = 27, D1 = 270, D2 = 320).  Both sides run in training mode with every parameter and the
input requiring a gradient; the backward is driven by a fixed incoming gradient of the output's dtype.  Prints one JSON line per
(module, dtype) with milliseconds per call."""
import argparse

import torch
import torch.nn.functional as TF

from harness import emit, need_gpu, window
from speech_decoding_amd.config import Config

DT = {"fp32": torch.float32, "bf16": torch.bfloat16, "fp16": torch.float16}


def eager_sa(z, cos, sin, mask, X):
    """models.py:45-65 with SpatialDropout's mask (77-86)."""
    W = torch.softmax(z.real @ cos + z.imag @ sin, dim=-1)
    return torch.einsum("oi,bit->bot", W.to(X.dtype), X * mask.to(X.dtype)[None, :, None])


def eager_sb(p, X, subj, mask):
    """models.py:111-117, the per-sample loop as one batched matmul."""
    H = TF.conv1d(eager_sa(p["z"], p["cos"], p["sin"], mask, X), p["conv.weight"], p["conv.bias"])
    return torch.bmm(p["subject_layer"][subj.long().to(X.device), :, :, 0], H)


def eager_cb(p, X, k, dil):
    """models.py:152-166 in training mode."""
    def bn(h, j):
        pre = f"batchnorm{j}."
        return TF.batch_norm(h, p[pre + "running_mean"], p[pre + "running_var"], p[pre + "weight"], p[pre + "bias"], True, 0.1, 1e-5)
    h = TF.conv1d(X, p["conv0.weight"], p["conv0.bias"], padding=dil[0], dilation=dil[0])
    h = TF.gelu(bn(h if k == 0 else h + X, 0))
    h = TF.gelu(bn(TF.conv1d(h, p["conv1.weight"], p["conv1.bias"], padding=dil[1], dilation=dil[1]) + h, 1))
    return TF.glu(TF.conv1d(h, p["conv2.weight"], p["conv2.bias"], padding=dil[2], dilation=dil[2]), dim=-2)


def eager_params(module, dt):
    """Device copies of a module's parameters and buffers by name (prefix "spatial_attention." dropped; the per-subject weights
    as one (S, D1, D1, 1) tensor "subject_layer"), the parameters in the compute dtype and requiring a gradient; z and the
    Fourier tables stay fp32."""
    out = {}
    for k, v in module.state_dict().items():
        k = k.split("spatial_attention.")[-1]
        v = v.detach().clone()
        if k.startswith("subject_layer."):
            continue
        if "running" in k:
            out[k] = v.to(dt)                          # (torch's BatchNorm backward wants them in the input's dtype)
        elif "num_batches" in k or k in ("cos", "sin"):
            out[k] = v
        else:
            out[k] = (v if v.is_complex() else v.to(dt)).requires_grad_(True)
    if hasattr(module, "subject_layer"):
        out["subject_layer"] = module.subject_layer.weight.detach().to(dt).requires_grad_(True)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--dtypes", nargs="+", default=["bf16", "fp32"])
    ap.add_argument("--B", type=int, default=256)
    ap.add_argument("--T", type=int, default=360)
    ap.add_argument("--C", type=int, default=208)
    ap.add_argument("--S", type=int, default=27)
    ap.add_argument("--D1", type=int, default=270)
    ap.add_argument("--D2", type=int, default=320)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    a = ap.parse_args()
    need_gpu()
    from speech_decoding.models import ConvBlock, SubjectBlock
    from speech_decoding_amd.layout import synthetic_positions
    dev = "cuda:0"
    B, T, C, S, D1, D2, K = a.B, a.T, a.C, a.S, a.D1, a.D2, 32
    loc = synthetic_positions(C, seed=1)
    g = torch.Generator().manual_seed(3)
    subj = torch.randint(0, S, (B,), generator=g)
    for name in a.dtypes:
        dt = DT[name]
        torch.manual_seed(2)
        args = Config(num_subjects=S, D1=D1, D2=D2, F=8, K=K, dataset="Gwilliams2022", d_drop=0.1, root_dir=".",
                    preprocs={"last4layers": False}, sensor_positions=loc.numpy(), compute_dtype=name)
        sb = SubjectBlock(args).to(dev).train()
        sb.spatial_attention.set_drop_centre(5)
        mask = sb.spatial_attention.device_masks(dev)[5]
        cb = ConvBlock(1, D1, D2).set_compute_dtype(dt).to(dev).train()
        psb, pcb = eager_params(sb, dt), eager_params(cb, dt)
        X = torch.randn(B, C, T, generator=g).to(dev).to(dt).requires_grad_(True)
        H = torch.randn(B, D2, T, generator=g).to(dev).to(dt).requires_grad_(True)
        G1 = torch.randn(B, D1, T, generator=g).to(dev).to(dt)
        G2 = torch.randn(B, D2, T, generator=g).to(dev).to(dt)
        dil = (2 ** 2, 2 ** 3, 2)                           # block 1's dilations (models.py:133,141,149)
        cases = {
            "SpatialAttention": (lambda: sb.spatial_attention(X), lambda: eager_sa(psb["z"], psb["cos"], psb["sin"], mask, X), G1),
            "SubjectBlock": (lambda: sb(X, subj), lambda: eager_sb(psb, X, subj, mask), G1),
            "ConvBlock": (lambda: cb(H), lambda: eager_cb(pcb, H, 1, dil), G2),
        }
        for mod, (hip, eager, G) in cases.items():
            row = {"module": mod, "dtype": name, "B": B, "T": T, "C": C, "S": S, "D1": D1, "D2": D2}
            for side, fn in (("hip", hip), ("torch", eager)):
                with torch.no_grad():
                    row[f"{side}_fwd_ms"] = round(window(fn, a.iters, a.warmup), 4)
                row[f"{side}_fwd_bwd_ms"] = round(window(lambda: fn().backward(G), a.iters, a.warmup), 4)
            emit(row)


if __name__ == "__main__":
    main()
