#!/usr/bin/env python3
"""The linear baseline beside train.py: a ridge regression from time-lagged sensors to speech features
(speech_decoding_amd.ridge.LaggedRidge, the backward mTRF) on the same config, the same data kinds and the same retrieval.

    python ridge_baseline.py                                  # configs/config.yaml, data=pool
    python ridge_baseline.py data=tracks compute_dtype=bf16 ridge.n_lags=60 ridge.alphas=[1,100,10000]
    python ridge_baseline.py dataset=Brennan2018 data=continuous

One pass of `partial_fit` over the training batches of one epoch (train.py's `build_data`: data=pool | resident | tracks |
continuous), `solve` for every `ridge.alphas` (default 1e0 ... 1e6 in decades), then alpha is picked on the test split by the
top-10 accuracy of `retrieve` — every test segment's prediction against the bank of the test split's speech segments — and
the line train.py prints for its test metrics is printed for the pick.  No subject indices are used: the baseline is one map
for all subjects.  `ridge.n_lags` defaults to 60 (half a second at 120 Hz).  Single process: fitting is not data parallel.
"""
from __future__ import annotations

import os
import sys
import time

import torch

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, ROOT)

from speech_decoding_amd import SpeechBank, load_config       # noqa: E402
from speech_decoding_amd import data as D                     # noqa: E402
from speech_decoding_amd.ridge import LaggedRidge             # noqa: E402
from train import build_data                                  # noqa: E402

DEFAULT_ALPHAS = tuple(10.0 ** e for e in range(7))


def run(args, train_batches=None, test_batch=None, log=print):
    """(row of metrics, the fitted LaggedRidge).  `train_batches` / `test_batch`: callables as train.run() takes them."""
    data_kind = str(args.get("data", "pool"))
    torch.cuda.set_device(0)
    device = torch.device("cuda", 0)
    if train_batches is None:
        _, train_batches, test_batch = build_data(args, data_kind, device, 0, 1)
    opts = args.get("ridge", None) or {}
    n_lags = int(opts.get("n_lags", 60))
    alphas = tuple(float(a) for a in opts.get("alphas", DEFAULT_ALPHAS))
    dims = D.segment_dims(args)
    ridge = LaggedRidge(dims.C, dims.F, n_lags=n_lags, device=device)
    n_batches = 0
    for X, Y, _ in train_batches():
        ridge.partial_fit(X, Y)
        n_batches += 1
    ridge.solve(alphas)
    X, Y, _ = test_batch()
    bank = SpeechBank.from_tensor(Y)
    labels = torch.arange(X.shape[0], device=device)
    results = ridge.score(X, bank, labels, k=min(10, X.shape[0]))
    best = ridge.best_alpha_
    Z = ridge.predict(X, alpha=best)
    row = {"alpha": alphas[best], "n_lags": n_lags, "train_segments": ridge.n // dims.T, "train_batches": n_batches,
           "test_loss": float(torch.nn.functional.mse_loss(Z, Y.float())), "testTop1acc": results[best].accuracy(1),
           "testTop10acc": results[best].accuracy(10), "solver": ridge.solver_,
           "testTop10acc_by_alpha": dict(zip(alphas, ridge.topk_))}
    log("Ridge | ", f"alpha: {row['alpha']:g} | ", f"lags: {n_lags} | ", f"test l: {row['test_loss']:.3f} | ",
        f"testTop1acc: {row['testTop1acc']:.3f} | ", f"testTop10acc: {row['testTop10acc']:.3f}")
    return row, ridge


def main(argv):
    overrides = [a for a in argv if "=" in a and not a.startswith("--")]
    path = next((a.split("=", 1)[1] for a in argv if a.startswith("--config=")), None)
    args = load_config(path, overrides)
    args.setdefault("root_dir", os.getcwd())
    args.setdefault("num_subjects", 27 if args.dataset == "Gwilliams2022" else 33)
    t0 = time.time()
    run(args)
    print(f"done in {time.time() - t0:.1f} s")


if __name__ == "__main__":
    main(sys.argv[1:])
