#!/usr/bin/env python3
"""Generate tests/golden/brennan.npz by RUNNING THE REFERENCE's Brennan2018 pipeline (dataclass/brennan2018.py:72-152).

Runs only where the reference checkout is present (SD_REFERENCE, needs sklearn and einops); the fixture it writes is
committed, this script's dependency on the reference is not.

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_brennan_golden.py

`brennan2018.py` imports packages that do no arithmetic on this path (mne, mne_bids, torchaudio, natsort, termcolor, and the
wav2vec helper's own imports): empty stand-in modules are registered in `sys.modules` of THIS process only, as
make_golden.py does.  The numbers come from the reference's own `shift_brain_signal`, `scaleAndClamp` (sklearn's
RobustScaler) and `baseline_correction`, called on an instance built without `__init__` (which only loads files); the
trim and split of lines 83-104 between them are restated here line by line.

Two cases, S = 3 subjects, C = 4 channels, F = 5 embedding channels:
  sw/   subject_wise=True;  the length is chosen so that trim_len // seq_len_samp == seq_len_samp: the reference's
        `split(num_segments)` then cuts chunks of seq_len_samp samples, the feed's default segmentation;
  pool/ subject_wise=False; trim_len // seq_len_samp = 11 != seq_len_samp = 24: the reference's chunks are 11 samples long,
        which the feed reproduces with an explicit segment_len.
Inputs: heavy-tailed values (Student t, 2 degrees of freedom) with a per-(subject, channel) gain over two decades and an
offset, artefact spikes (the clamp bites; under pooling the high-gain subjects are clamped wholesale), one constant row
(zero inter-quartile range) and one row with half its samples tied.
"""
import importlib
import os
import sys
import types

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
REF = os.environ.get("SD_REFERENCE", "/root/reference")
sys.dont_write_bytecode = True
sys.path.insert(0, REF)


def _stand_in(name, **attrs):
    try:
        importlib.import_module(name)
        return
    except Exception:
        pass
    m = types.ModuleType(name)
    m.__dict__.update(attrs)
    sys.modules[name] = m
    if "." in name:
        parent, child = name.rsplit(".", 1)
        setattr(sys.modules[parent], child, m)


_stand_in("termcolor", cprint=lambda *a, **k: None)
_stand_in("mne", set_log_level=lambda *a, **k: None)
_stand_in("mne_bids")
_stand_in("torchaudio")
_stand_in("torchaudio.functional")
_stand_in("natsort", natsorted=sorted)
_stand_in("pandas")
_stand_in("scipy")
_stand_in("scipy.io")
_stand_in("tqdm", tqdm=lambda x, *a, **k: x)
_stand_in("speech_decoding.utils.wav2vec_util", load_wav2vec_model=None, getW2VLastFourLayersAvg=None)

from speech_decoding.dataclass.brennan2018 import Brennan2018Dataset as Ref      # noqa: E402  (the reference)


def make_inputs(S, C, F, L, seed):
    rng = np.random.RandomState(seed)
    gain = 10.0 ** rng.uniform(-1.0, 1.0, size=(S, C, 1))
    X = (rng.standard_t(2, size=(S, C, L)) + rng.randn(S, C, 1)) * gain
    X[0, 0, L // 3] *= 300.0
    X[2, 3, L // 2] *= -300.0
    X[1, 2] = 0.25                                   # constant row: zero inter-quartile range
    X[2, 1, ::2] = 1.5                               # half the row tied (the median and a quartile sit inside the run)
    Y = rng.randn(F, L)
    return torch.from_numpy(X.astype(np.float32)), torch.from_numpy(Y.astype(np.float32))


def run_reference(X, Y, srate, seq_len_sec, baseline_len_sec, clamp_lim, subject_wise):
    ds = Ref.__new__(Ref)
    ds.clamp, ds.clamp_lim, ds.subject_wise = True, clamp_lim, subject_wise
    ds.X, ds.Y = Ref.shift_brain_signal(X, Y, srate=srate)                       # brennan2018.py:72
    shift = X.shape[-1] - ds.X.shape[-1]
    ds.seq_len_samp = int(seq_len_sec * srate)                                   # :83
    ds.baseline_len_samp = int(ds.seq_len_samp * baseline_len_sec / seq_len_sec)  # :86
    trim_len = (ds.X.shape[-1] // ds.seq_len_samp) * ds.seq_len_samp             # :89
    num_segments = trim_len // ds.seq_len_samp                                   # :92
    ds.X = ds.X[..., :trim_len]                                                  # :95
    ds.Y = ds.Y[..., :trim_len]                                                  # :96
    ds.X = ds.scaleAndClamp()                                                    # :99
    ds.X = ds.X.split(num_segments, dim=-1)                                      # :103
    ds.Y = ds.Y.split(num_segments, dim=-1)                                      # :104
    ds.X = ds.baseline_correction()                                              # :107
    assert len({x.shape[-1] for x in ds.X}) == 1
    lengths = np.array([shift, ds.seq_len_samp, ds.baseline_len_samp, trim_len, num_segments, ds.X[0].shape[-1], len(ds.X)])
    return torch.stack(list(ds.X)).numpy(), torch.stack(list(ds.Y)).numpy(), lengths


def main():
    out = {}
    cases = {"sw": dict(L=330, srate=9, seq_len_sec=2, baseline_len_sec=0.5, clamp_lim=20, subject_wise=True, seed=31),
             "pool": dict(L=275, srate=12, seq_len_sec=2, baseline_len_sec=0.5, clamp_lim=20, subject_wise=False, seed=32)}
    for tag, c in cases.items():
        X, Y = make_inputs(3, 4, 5, c["L"], c["seed"])
        expX, expY, lengths = run_reference(X.clone(), Y.clone(), c["srate"], c["seq_len_sec"], c["baseline_len_sec"], c["clamp_lim"],
                                            c["subject_wise"])
        out.update({f"{tag}/X": X.numpy(), f"{tag}/Y": Y.numpy(), f"{tag}/expX": expX.astype(np.float32), f"{tag}/expY": expY,
                    f"{tag}/lengths": lengths, f"{tag}/srate": np.float64(c["srate"]), f"{tag}/seq_len_sec": np.float64(c["seq_len_sec"]),
                    f"{tag}/baseline_len_sec": np.float64(c["baseline_len_sec"]), f"{tag}/clamp_lim": np.float64(c["clamp_lim"]),
                    f"{tag}/subject_wise": np.array(c["subject_wise"])})
        print(f"{tag}: lengths (shift, seq, baseline, trim, num_segments, chunk_len, chunks) = {lengths.tolist()}, "
              f"clamped {int((np.abs(expX) >= c['clamp_lim'] - 1e-3).sum())} values of {expX.size}, max |x| {np.abs(expX).max():.3f}")
    assert out["sw/lengths"][5] == out["sw/lengths"][1] and out["pool/lengths"][5] != out["pool/lengths"][1]
    path = os.path.join(HERE, "brennan.npz")
    np.savez_compressed(path, **out)
    print("wrote", path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
