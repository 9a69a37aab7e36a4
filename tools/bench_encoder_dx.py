"""BrainEncoder + CLIPLoss with and without a gradient for the brain input X, a frozen eval() attribution pass, and the dX kernel
alone.  Device events after warm-up, repeated rounds (median and spread).  Diagnostic; not part of the product.

    python tools/bench_encoder_dx.py [--iters 20] [--rounds 5] [--json out.json]
    python tools/bench_encoder_dx.py --kernel-only      # the dX kernel alone: run under rocprofv3 --kernel-trace --stats

Shapes: configs[1] (C=208, S=27, T=360, B=256) in bf16 and configs[0] (C=60, S=1, T=360, B=64) in fp32; D1=270, D2=320, F=1024.
  step / step_dx       forward + loss + backward of a training step, X without / with requires_grad
  fwd_bwd / attrib     forward + backward of a training step (all parameters trainable) against a frozen eval() encoder's
                       forward + backward into X (the saliency-map case)
  kernel               sda_input_grad alone on the step's shapes; bytes = G read + dX written, against 8 TB/s"""
import argparse

import numpy as np
import torch

import harness
from speech_decoding_amd import lib as L, ops
from speech_decoding_amd.config import Config

SHAPES = [dict(name="config2", C=208, S=27, T=360, B=256, dtype="bf16"), dict(name="config1", C=60, S=1, T=360, B=64, dtype="fp32")]
D1, D2, F, K = 270, 320, 1024, 32
DT = {"fp32": torch.float32, "bf16": torch.bfloat16}


def timeit(fn, iters, rounds):
    s = harness.summarize(harness.rounds(fn, iters, rounds, 3))
    return {"median_ms": s.median, "min_ms": s.min, "max_ms": s.max}


def setup(s, dev="cuda:0"):
    from speech_decoding.models import BrainEncoder
    from speech_decoding.utils.loss import CLIPLoss
    torch.manual_seed(0)
    loc = np.random.RandomState(0).uniform(0.1, 0.9, size=(s["C"], 2))     # sensor positions in the layout's unit square
    args = Config(num_subjects=s["S"], D1=D1, D2=D2, F=512, K=K, dataset="Gwilliams2022", d_drop=0.1, root_dir=".",
                preprocs={"last4layers": True}, reduction="mean", init_temperature=5.1, sensor_positions=loc,
                compute_dtype=s["dtype"])
    enc = BrainEncoder(args).to(dev).train()          # the reference's own initialisation
    crit = CLIPLoss(args).to(dev)
    X = torch.randn(s["B"], s["C"], s["T"])
    Y = torch.randn(s["B"], F, s["T"])
    subj = torch.randint(0, s["S"], (s["B"],))
    return enc, crit, X.to(dev), Y.to(dev), subj


def one(s, iters, rounds):
    enc, crit, X, Y, subj = setup(s)
    enc.set_drop_centre(4)
    params = list(enc.parameters()) + list(crit.parameters())
    Xg = X.clone().requires_grad_(True)

    def step(x):
        loss = crit(Y, enc(x, subj))
        loss.backward()
        for p in params:
            p.grad = None
        x.grad = None

    r = {"shape": s["name"], "dtype": s["dtype"], "B": s["B"], "C": s["C"]}
    r["step"] = timeit(lambda: step(X), iters, rounds)
    r["step_dx"] = timeit(lambda: step(Xg), iters, rounds)
    r["dx_extra_ms"] = r["step_dx"]["median_ms"] - r["step"]["median_ms"]

    # (b) forward + backward of the encoder alone (a fixed dZ): trainable vs a frozen eval() encoder into X
    dZ = torch.randn(s["B"], F, s["T"], device=X.device).to(DT[s["dtype"]])

    def fwd_bwd(x):
        Z = enc(x, subj)
        Z.backward(dZ)
        for p in params:
            p.grad = None
        x.grad = None

    r["fwd_bwd_train"] = timeit(lambda: fwd_bwd(X), iters, rounds)
    enc.eval()
    for p in enc.parameters():
        p.requires_grad_(False)
    r["attrib_frozen_eval"] = timeit(lambda: fwd_bwd(Xg), iters, rounds)
    r["attrib_over_train"] = r["attrib_frozen_eval"]["median_ms"] / r["fwd_bwd_train"]["median_ms"]
    for p in enc.parameters():
        p.requires_grad_(True)
    enc.train()

    # (c) the kernel alone
    r["kernel"] = kernel(s, iters, rounds)
    return r


def kernel(s, iters, rounds, dev="cuda:0"):
    dt = DT[s["dtype"]]
    D1p, Cp = L.pad_channels(D1), L.pad_channels(s["C"])
    G = ops.new_rows(s["B"], s["T"], D1p, dt, dev)
    ops.pack_rows(torch.randn(s["B"], D1, s["T"], device=dev), G)
    W = torch.randn((s["S"], 1, D1p, Cp), device=dev).to(dt)
    widx = torch.randint(0, s["S"], (s["B"],), device=dev, dtype=torch.int32)
    t = timeit(lambda: ops.input_grad(G, W, widx, s["B"], s["C"], s["T"], torch.float32), iters, rounds)
    moved = s["B"] * s["T"] * (D1p * G.element_size() + s["C"] * 4)
    t["bytes"] = moved
    t["TBps"] = moved / (t["median_ms"] * 1e-3) / 1e12
    t["byte_bound_us"] = moved / 8e12 * 1e6
    return t


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--kernel-only", action="store_true")
    ap.add_argument("--json", default=None)
    a = ap.parse_args()
    harness.need_gpu()
    rows = [kernel(s, a.iters, a.rounds) | {"shape": s["name"]} for s in SHAPES] if a.kernel_only else \
        [one(s, a.iters, a.rounds) for s in SHAPES]
    for r in rows:
        harness.emit(r, a.json, append=True)


if __name__ == "__main__":
    main()
