#!/usr/bin/env python3
"""Generate tests/golden/clip_grad.npz by RUNNING THE REFERENCE'S OWN CLIPLoss and torch autograd.

Runs only where a checkout of the reference is present (SD_REFERENCE, default /root/reference); the fixture it writes is
committed and travels, this script's dependency on the reference does not.

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_clip_grad_golden.py

For each of three odd shapes (B, F, T) — F not a multiple of 64, odd T, B = 2 included — x (speech) and y (brain) are seeded
N(0, 1) fp32 leaves, and temp is a leaf too.  For every (fast, reduction) in {True, False} x {"mean", "sum"} the fixture stores
the reference's loss = CLIPLoss(args)(x, y, fast=fast) and what autograd gives for loss.backward():
s<i>/x, s<i>/y, s<i>/temp, s<i>/<case>/loss, s<i>/<case>/dx, s<i>/<case>/dy, s<i>/<case>/dtemp with <case> = "fast-mean",
"fast-sum", "slow-mean", "slow-sum".  fast=False does not use temp: its dtemp is stored as 0 (the reference leaves
temp.grad None).
"""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
REF = os.environ.get("SD_REFERENCE", "/root/reference")
sys.dont_write_bytecode = True
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
sys.path.insert(0, REF)

from speech_decoding.utils.loss import CLIPLoss as RefCLIPLoss      # noqa: E402  (the reference)
from speech_decoding_amd.config import Config                        # noqa: E402

SHAPES = [(4, 72, 25), (2, 100, 9), (6, 64, 19)]
TEMPS = [2.3, 0.7, 1.5]
CASES = [("fast-mean", True, "mean"), ("fast-sum", True, "sum"), ("slow-mean", False, "mean"), ("slow-sum", False, "sum")]


def main():
    g = torch.Generator().manual_seed(20261016)
    out = {"shapes": np.array(SHAPES, dtype=np.int64), "temps": np.array(TEMPS, dtype=np.float32)}
    for i, ((B, F, T), t0) in enumerate(zip(SHAPES, TEMPS)):
        x = torch.randn(B, F, T, generator=g)
        y = torch.randn(B, F, T, generator=g)
        out[f"s{i}/x"], out[f"s{i}/y"] = x.numpy(), y.numpy()
        for name, fast, reduction in CASES:
            crit = RefCLIPLoss(Config(reduction=reduction, init_temperature=t0))
            xl, yl = x.clone().requires_grad_(True), y.clone().requires_grad_(True)
            loss = crit(xl, yl, fast=fast)
            loss.backward()
            key = f"s{i}/{name}"
            out[f"{key}/loss"] = loss.detach().numpy()
            out[f"{key}/dx"], out[f"{key}/dy"] = xl.grad.numpy(), yl.grad.numpy()
            dt = crit.temp.grad
            out[f"{key}/dtemp"] = (dt if dt is not None else torch.zeros(1)).detach().numpy()
    path = os.path.join(HERE, "clip_grad.npz")
    np.savez_compressed(path, **out)
    print(f"wrote {path} ({os.path.getsize(path)} bytes)")


if __name__ == "__main__":
    main()
