"""GPU batch collate — drop-in for the reference's `Gwilliams2022Collator` (gwilliams2022.py:640-661):
baseline correction + per-(sample, channel) RobustScaler + clamp, run as ONE kernel on the device instead
of a Python loop over the batch with sklearn on DataLoader workers."""
from __future__ import annotations

from typing import List

import torch
import torch.nn as nn

from . import lib as L
from . import ops


def robust_scale_clamp(X: torch.Tensor, baseline_len_samp: int, clamp_lim: float, clamp: bool = True) -> torch.Tensor:
    """X: (B, C, T) float on the GPU -> same shape, fp32."""
    if not X.is_cuda:
        raise L.SdaError("collate needs device tensors (no CPU fallback)")
    B, C, T = X.shape
    src = X.contiguous().float()
    out = torch.empty_like(src)
    L.check(L.load().sda_collate_rows(src.data_ptr(), out.data_ptr(), B * C, T, int(baseline_len_samp), float(clamp_lim),
                                      int(bool(clamp)), torch.cuda.current_stream().cuda_stream), "collate_rows")
    return out


def _row_layout(X: torch.Tensor, pooled: bool):
    """(rows, row_stride, n_chunks, chunk_len, chunk_stride) of a contiguous (S, C, L) tensor: one row per (subject, channel),
    or — pooled — one row per channel made of the S subjects' pieces (brennan2018.py:114-134), with no rearranging copy."""
    if not X.is_cuda:
        raise L.SdaError("whole-recording scaling needs device tensors (no CPU fallback)")
    if X.dim() != 3 or X.dtype != torch.float32 or not X.is_contiguous():
        raise L.SdaError("whole-recording scaling: a contiguous fp32 (S, C, L) tensor")
    S, C, Ln = X.shape
    return (C, Ln, S, Ln, C * Ln) if pooled else (S * C, Ln, 1, Ln, Ln)


def robust_stats(X: torch.Tensor, pooled: bool = False):
    """RobustScaler.fit over whole recordings (brennan2018.py:117,130), sda_robust_stats: X (S, C, L) fp32 on the device ->
    (centre, scale), each (S, C) — or (C,) when `pooled` (every subject's samples of a channel in one row).  Median and
    inter-quartile range by exact selection, numpy's "linear" rule, zero scale -> 1.  X must hold no NaN."""
    rows, rstride, nch, clen, cstride = _row_layout(X, pooled)
    lib = L.load()
    out = torch.empty((2, rows), dtype=torch.float32, device=X.device)
    nbytes = int(lib.sda_robust_stats_scratch_bytes(rows))
    scratch = torch.empty(nbytes, dtype=torch.uint8, device=X.device)
    with torch.cuda.device(X.device):
        L.check(lib.sda_robust_stats(X.data_ptr(), rows, rstride, nch, clen, cstride, out[0].data_ptr(), out[1].data_ptr(),
                                     scratch.data_ptr(), nbytes, torch.cuda.current_stream().cuda_stream), "robust_stats")
    shape = (X.shape[1],) if pooled else tuple(X.shape[:2])
    return out[0].reshape(shape), out[1].reshape(shape)


def scale_clamp_rows(X: torch.Tensor, centre: torch.Tensor, scale: torch.Tensor, clamp_lim: float, clamp: bool = True,
                     pooled: bool = False, out: torch.Tensor = None) -> torch.Tensor:
    """RobustScaler.transform + clamp_ (brennan2018.py:120-124,130-133), sda_scale_clamp_rows: (X - centre) / scale per row of
    robust_stats' layout, limited to +-clamp_lim.  `out`: a contiguous tensor of X's shape; `out=X` works in place."""
    rows, rstride, nch, clen, cstride = _row_layout(X, pooled)
    out = torch.empty_like(X) if out is None else out
    if out.shape != X.shape or not out.is_cuda or out.dtype != torch.float32 or not out.is_contiguous():
        raise L.SdaError("scale_clamp_rows: out must be a contiguous fp32 device tensor of X's shape")
    centre, scale = centre.reshape(-1), scale.reshape(-1)
    for t in (centre, scale):
        if not t.is_cuda or t.dtype != torch.float32 or t.numel() != rows or not t.is_contiguous():
            raise L.SdaError("scale_clamp_rows: centre and scale must hold one fp32 device value per row")
    with torch.cuda.device(X.device):
        L.check(L.load().sda_scale_clamp_rows(X.data_ptr(), out.data_ptr(), rows, rstride, nch, clen, cstride, centre.data_ptr(),
                                              scale.data_ptr(), float(clamp_lim), int(bool(clamp)),
                                              torch.cuda.current_stream().cuda_stream), "scale_clamp_rows")
    return out


def gather_baseline_windows(X: torch.Tensor, subjects, starts, T: int, baseline_len_samp: int) -> torch.Tensor:
    """Segment gather + baseline_correction (brennan2018.py:136-152), sda_gather_baseline_windows: X (S, C, L) fp32 resident;
    window b = X[subjects[b], :, starts[b] : starts[b] + T] minus the mean of its first baseline_len_samp samples, per channel.
    subjects, starts: host integer sequences of length B -> (B, C, T) fp32."""
    if not X.is_cuda:
        raise L.SdaError("gather_baseline_windows needs device tensors (no CPU fallback)")
    if X.dim() != 3 or X.dtype != torch.float32 or not X.is_contiguous():
        raise L.SdaError("gather_baseline_windows: a contiguous fp32 (S, C, L) tensor")
    S, C, Ln = X.shape
    import numpy as np
    sub = np.asarray(subjects, dtype=np.int64).reshape(-1)
    on = np.asarray(starts, dtype=np.int64).reshape(-1)
    T, nb = int(T), int(baseline_len_samp)
    if len(sub) != len(on) or len(sub) < 1:
        raise L.SdaError("gather_baseline_windows: one subject and one start per window")
    if T < 1 or nb < 0 or nb > T:
        raise L.SdaError("gather_baseline_windows: 0 <= baseline_len_samp <= T")
    if bool(((sub < 0) | (sub >= S) | (on < 0) | (on + T > Ln)).any()):
        raise IndexError("segment window leaves its recording")
    dev = X.device
    out = torch.empty((len(sub), C, T), dtype=torch.float32, device=dev)
    with torch.cuda.device(dev):
        ptrs = ops.upload_small(X.data_ptr() + 4 * (sub * (C * Ln) + on), dev)
        cstr = ops.upload_small(np.full(len(sub), Ln, dtype=np.int64), dev)
        L.check(L.load().sda_gather_baseline_windows(ptrs.data_ptr(), cstr.data_ptr(), out.data_ptr(), len(sub), C, T, nb,
                                                     torch.cuda.current_stream().cuda_stream), "gather_baseline_windows")
    return out


class Gwilliams2022Collator(nn.Module):
    def __init__(self, args, device="cuda"):
        super().__init__()
        self.brain_resample_rate = args.preprocs["brain_resample_rate"]
        self.baseline_len_samp = int(self.brain_resample_rate * args.preprocs["baseline_len_sec"])
        self.clamp = args.preprocs["clamp"]
        self.clamp_lim = args.preprocs["clamp_lim"]
        self.device = device

    def forward(self, batch: List[tuple]):
        X = torch.stack([item[0] for item in batch]).to(self.device, non_blocking=True)
        Y = torch.stack([item[1] for item in batch])
        subject_idx = torch.IntTensor([item[2] for item in batch])
        X = robust_scale_clamp(X, self.baseline_len_samp, self.clamp_lim, self.clamp)
        return X, Y, subject_idx


class ResidentSegments:
    """Segment gather on the GPU (gwilliams2022.py:129-142): per-session recordings (C, L_s) stay resident in HBM;
    a batch is described by (session index, onset sample) per segment and materialised — window extraction,
    baseline correction, robust scaling, clamp — by one kernel, replacing `__getitem__` + the collator."""

    def __init__(self, sessions, seq_len_samp: int, baseline_len_samp: int, clamp_lim: float, clamp: bool = True):
        self.sessions = [s.contiguous().float() for s in sessions]
        if not all(s.is_cuda and s.dim() == 2 for s in self.sessions):
            raise L.SdaError("ResidentSegments needs (C, L) device tensors")
        self.C = self.sessions[0].shape[0]
        self.T, self.nb, self.lim, self.clamp = int(seq_len_samp), int(baseline_len_samp), float(clamp_lim), bool(clamp)
        self._base = torch.tensor([s.data_ptr() for s in self.sessions], dtype=torch.int64)
        self._len = torch.tensor([s.shape[1] for s in self.sessions], dtype=torch.int64)

    def batch(self, session_idx, onsets) -> torch.Tensor:
        """session_idx, onsets: integer sequences of length B (host) -> X (B, C, T) fp32 on the device."""
        sidx = torch.as_tensor(session_idx, dtype=torch.int64)
        on = torch.as_tensor(onsets, dtype=torch.int64)
        if bool(((on < 0) | (on + self.T > self._len[sidx])).any()):
            raise IndexError("segment window leaves its session recording")
        dev = self.sessions[0].device
        # the two index tables travel in kernel arguments (ops.upload_small): a copy from pageable host memory makes the host
        # wait for the stream it is queued on — with the step's loop two milliseconds ahead of the GPU that wait is the step's
        with torch.cuda.device(dev):
            ptrs = ops.upload_small((self._base[sidx] + 4 * on).numpy(), dev)
            cstr = ops.upload_small(self._len[sidx].numpy(), dev)
        out = torch.empty((len(sidx), self.C, self.T), dtype=torch.float32, device=dev)
        L.check(L.load().sda_collate_windows(ptrs.data_ptr(), cstr.data_ptr(), out.data_ptr(), len(sidx), self.C, self.T, self.nb,
                                             self.lim, int(self.clamp), torch.cuda.current_stream().cuda_stream), "collate_windows")
        return out
