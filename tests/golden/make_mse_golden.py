#!/usr/bin/env python3
"""Generate tests/golden/mse.npz by RUNNING THE REFERENCE'S OWN MSELoss and torch autograd.

Runs only where a checkout of the reference is present (SD_REFERENCE, default /root/reference); the fixture it writes is
committed and travels, this script's dependency on the reference does not.

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_mse_golden.py

For each of three odd shapes (B, F, T) — T not a multiple of 8, F not a multiple of 64, B = 1 included — Y and Z are seeded
N(0, 1) fp32 leaves; the fixture stores them with the reference's loss = MSELoss()(Y, Z) and the gradients autograd gives
for loss.backward(): s<i>/Y, s<i>/Z, s<i>/loss, s<i>/dZ, s<i>/dY.
"""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
REF = os.environ.get("SD_REFERENCE", "/root/reference")
sys.dont_write_bytecode = True
sys.path.insert(0, REF)

from speech_decoding.utils.loss import MSELoss as RefMSELoss      # noqa: E402  (the reference)

SHAPES = [(3, 80, 37), (2, 1024, 17), (1, 64, 9)]


def main():
    g = torch.Generator().manual_seed(20261015)
    out = {"shapes": np.array(SHAPES, dtype=np.int64)}
    for i, (B, F, T) in enumerate(SHAPES):
        Y = torch.randn(B, F, T, generator=g).requires_grad_(True)
        Z = torch.randn(B, F, T, generator=g).requires_grad_(True)
        loss = RefMSELoss()(Y, Z)
        loss.backward()
        out[f"s{i}/Y"], out[f"s{i}/Z"] = Y.detach().numpy(), Z.detach().numpy()
        out[f"s{i}/loss"] = loss.detach().numpy()
        out[f"s{i}/dZ"], out[f"s{i}/dY"] = Z.grad.numpy(), Y.grad.numpy()
    path = os.path.join(HERE, "mse.npz")
    np.savez_compressed(path, **out)
    print(f"wrote {path} ({os.path.getsize(path)} bytes)")


if __name__ == "__main__":
    main()
