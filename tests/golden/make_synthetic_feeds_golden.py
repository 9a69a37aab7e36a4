#!/usr/bin/env python3
"""Writes tests/golden/synthetic_feeds.npz: the seeded stand-in datasets of speech_decoding_amd.data at the small cases of
tests/synthetic_feed_cases.py, as the commit this script is run on builds them.  The committed file was recorded on the commit
BEFORE the builders were folded into one (there data.py still imported WindowBank from retrieval inside the builder, hence the
second patch below); the same run on any later commit must give the same file.

    python tests/golden/make_synthetic_feeds_golden.py [--out FILE]

Per case `<case>/tol` is the tolerance for the arrays behind which a matrix product or a mean lies (the resident Y, the tracks, the
subject feed's Y), where another host CPU may sum in another order.  It is derived, not chosen:  4 * n * 2^-24 * A  with
  n   the number of terms behind one element: C, plus the baseline's nb where a baseline mean enters;
  A   the largest  sum_c |P[f, c]| * |operand[c, t]|  of the case, in float64 from the returned recordings (operand: the
      baseline-corrected scaled window, the scaled first recording, the scaled latent response);
  4   = 2 x 2: two fp32 evaluations each lie within n * 2^-24 * A of the exact sum, and the scale and the noise add that follow.
P (the only (F, C) draw) and the subject case's latent (the only (C, length) draw) are read by wrapping torch.randn while the
builder runs.  A wrong or missing draw moves elements by O(1)."""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))

from tests import synthetic_feed_cases as K       # noqa: E402

U = 2.0 ** -24


def amplitude(P, operands):
    return max(float((np.abs(P) @ np.abs(w)).max()) for w in operands)


def tolerance(name, out, draws):
    C, F = K.C, K.F
    P = (next(d for d in draws if tuple(d.shape) == (F, C)) / np.sqrt(C)).double().numpy()
    if name == "subject":
        length = K.CASES[name][1]["length"]
        latent = next(d for d in draws if tuple(d.shape) == (C, length)).double().numpy()
        return 4 * C * U * amplitude(P, [latent / 1.35])
    rec = out["recordings"].astype(np.float64)
    per = len(rec) // (int(out["rec_task"].max()) + 1)                     # recordings per task; a task's first one carries the speech
    if "tracks" in out:
        tasks = np.unique(out["seg_task"])
        return 4 * C * U * amplitude(P, [rec[per * t] / (2.0 * 1.35) for t in tasks])
    T, nb = (int(v) for v in out["segments_ctor"][:2])
    windows = []
    for t, j in zip(out["seg_task"], out["seg_in_task"]):
        o = int(out["onsets"][per * t][j])
        w = rec[per * t][:, o: o + T]
        windows.append((w - w[:, :nb].mean(axis=1, keepdims=True)) / (2.0 * 1.35))
    return 4 * (C + nb) * U * amplitude(P, windows)


def main(argv):
    out_path = argv[argv.index("--out") + 1] if "--out" in argv else os.path.join(HERE, "synthetic_feeds.npz")
    from speech_decoding_amd import retrieval
    K.patch_recorders(lambda mod, name, value: setattr(mod, name, value))
    retrieval.WindowBank = K.FakeBank
    real_randn, arrays = torch.randn, {}
    for name in K.CASES:
        draws = []

        def recording_randn(*a, **k):
            draws.append(real_randn(*a, **k))
            return draws[-1]
        torch.randn = recording_randn
        try:
            out = K.run_case(name)
        finally:
            torch.randn = real_randn
        out["tol"] = np.float64(tolerance(name, out, draws))
        print(f"{name}: tol {out['tol']:.4e}")
        arrays.update({f"{name}/{k}": np.asarray(v) for k, v in out.items()})
    np.savez_compressed(out_path, **arrays)
    print(f"{out_path}: {os.path.getsize(out_path)} bytes, {len(arrays)} arrays")


if __name__ == "__main__":
    main(sys.argv[1:])
