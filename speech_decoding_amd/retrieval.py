"""Decoding: which of M speech segments did this brain segment hear?

The training path only ever ranks a square batch against itself (`Classifier.forward`, loss.retrieval_ranks).  This module
is its forward-only counterpart for a trained encoder: a resident bank of candidate segments (`SpeechBank`) and `retrieve`,
which scores N query segments against all M candidates and returns the k best of each, and, given the true candidates, their
ranks over the whole bank.  The score is the reference's similarity (models.py:223-232), <q, c> / max(|q| |c|, 1e-8).

Everything runs in libsdamd.so: the pack and the norms (ops.rows_of: one ops.pack_rows launch for fp32, bf16 or fp16 segments
with no widened copy, none for an encoder's row-layout view; sda_rows_sumsq), the similarity GEMM of the loss
(ops.matmul_nt_splitk's two kernels, rectangular) and one selection launch per block of queries (csrc/retrieval.hip).  The
N x M score matrix is never held whole: see plan_blocks.  Which side is "query" is the caller's choice — brain segments against
a speech bank (`Classifier.decode`) or the other way round; under torch.distributed every rank decodes its own queries
against its own bank and no collective is issued.  No gradients: both entry points run under no_grad.

A `WindowBank` holds candidates that are windows of continuous speech tracks (the reference cuts its segments at word onsets out
of one embedding track per audio file): each track is stored once as plain rows, a candidate is a row start, and the same pass
scores them with the windowed form of the similarity GEMM (sda_sim_gemm_windows) — 16-bit storage only, nothing is materialised.
The same bank is the speech side of the training feed (data.ResidentSegmentFeed with the bank as Y: ops.gather_windows), and
`WindowBank.select` hands a subset of its candidates — the test split — to the same decoding without copying the table.

Word-level decoding sits on the same blocked score matrix, filled by the same pass (`_ScorePass`: checks, pack, norms, scratch
and block loop, written once): a `ClassIndex` says which class (word) every candidate is an instance of, and `retrieve_classes`
pools each row's scores per class on the device (sda_retrieval_class_reduce: a segmented log-sum-exp at the loss's temperature,
each class with its own maximum), pools repeated queries (sda_retrieval_pool_rows) and selects over classes with the same kernel.
"""
from __future__ import annotations

from typing import NamedTuple, Optional

import numpy as np
import torch

from . import lib as L
from . import ops

MAX_K = 64          # the selection kernel keeps the 64 best candidates of a row


class Retrieval(NamedTuple):
    """indices (N, k) int64: bank rows of the k best candidates, best first (score descending, lower index first on equal
    scores); scores (N, k) fp32: their cosine similarities; ranks (N,) int32 or None: candidates that beat the labelled one
    over the whole bank (0 = top-1; -1 for a device label outside the bank).  All on the device."""
    indices: torch.Tensor
    scores: torch.Tensor
    ranks: Optional[torch.Tensor]

    def accuracy(self, k: int) -> float:
        """Share of queries whose true candidate is among the k best (reads the ranks back)."""
        if self.ranks is None:
            raise ValueError("Retrieval.accuracy: retrieve() was called without labels")
        return float((self.ranks < k).float().mean())


class SpeechBank:
    """M candidate segments, resident on the device in the loss's row layout: every candidate is one contiguous row of
    rows_tp(T) * pad_channels(F) elements of `dtype` (padding zero), with its fp32 squared norm beside it.  A bank filled by
    several add() calls holds the same bytes and norms as one filled at once."""

    def __init__(self, F: int, T: int, dtype=torch.bfloat16, device="cuda", capacity: Optional[int] = None):
        if int(F) < 1 or int(T) < 1:
            raise ValueError(f"SpeechBank: F and T must be positive, got F={F}, T={T}")
        if dtype not in ops.COMPUTE_DTYPES:
            raise ValueError(f"SpeechBank: dtype {dtype}; a bank holds float32, bfloat16 or float16")
        if capacity is not None and int(capacity) < 0:
            raise ValueError("SpeechBank: capacity must not be negative")
        self.F, self.T, self.dtype = int(F), int(T), dtype
        self.device = torch.device(device)
        if self.device.type != "cuda":
            raise L.SdaError("SpeechBank lives on the MI355X device (there is no CPU path)")
        self.row_elems = L.rows_tp(self.T) * L.pad_channels(self.F)
        self._size = 0
        self._capacity = 0
        self._rows = None               # (capacity * row_elems,) of dtype
        self._sq = None                 # (capacity,) fp32
        if capacity:
            self._reserve(int(capacity))

    @classmethod
    def from_tensor(cls, Y: torch.Tensor, dtype=torch.bfloat16) -> "SpeechBank":
        if not torch.is_tensor(Y) or Y.dim() != 3:
            raise ValueError("SpeechBank.from_tensor: Y must be an (M, F, T) tensor")
        if not Y.is_cuda:
            raise L.SdaError("SpeechBank.from_tensor: Y must live on the MI355X device (there is no CPU path)")
        bank = cls(Y.shape[1], Y.shape[2], dtype=dtype, device=Y.device, capacity=Y.shape[0])
        bank.add(Y)
        return bank

    def __len__(self) -> int:
        return self._size

    @property
    def rows(self) -> torch.Tensor:
        """(M, row_elems) view of the stored candidates."""
        return self._rows[: self._size * self.row_elems].view(self._size, self.row_elems)

    @property
    def norms_sq(self) -> torch.Tensor:
        """(M,) fp32 squared norms of the stored (rounded) candidates."""
        return self._sq[: self._size]

    def _reserve(self, capacity: int):
        if capacity <= self._capacity:
            return
        L.load()
        rows = torch.empty(capacity * self.row_elems, dtype=self.dtype, device=self.device)
        sq = torch.empty(capacity, dtype=torch.float32, device=self.device)
        if self._size:
            rows[: self._size * self.row_elems].copy_(self._rows[: self._size * self.row_elems])
            sq[: self._size].copy_(self._sq[: self._size])
        self._rows, self._sq, self._capacity = rows, sq, capacity

    @torch.no_grad()
    def add(self, Y: torch.Tensor) -> range:
        """Append the m candidates of Y (m, F, T) — fp32, bf16 or fp16, any strides, or the zero-copy view an encoder
        returns — and return the bank indices they received."""
        if not torch.is_tensor(Y) or Y.dim() != 3 or tuple(Y.shape[1:]) != (self.F, self.T):
            got = tuple(Y.shape) if torch.is_tensor(Y) else type(Y).__name__
            raise ValueError(f"SpeechBank.add: expected (m, {self.F}, {self.T}), got {got}")
        if not Y.is_cuda:
            raise L.SdaError("SpeechBank.add: Y must live on the MI355X device (there is no CPU path)")
        if Y.device != self.device and not (self.device.index is None and Y.device.index == torch.cuda.current_device()):
            raise L.SdaError(f"SpeechBank.add: Y is on {Y.device}, the bank on {self.device}")
        if Y.dtype not in ops.COMPUTE_DTYPES:
            raise L.SdaError(f"SpeechBank.add: Y of dtype {Y.dtype}; candidates are float32, bfloat16 or float16")
        m, first, re = Y.shape[0], self._size, self.row_elems
        if m == 0:
            return range(first, first)
        if first + m > self._capacity:
            self._reserve(max(first + m, 2 * self._capacity))
        packed, _ = ops.rows_of(Y, self.F, self.dtype)                    # pad rows and channels zero
        self._rows[first * re: (first + m) * re].copy_(packed.reshape(-1)[: m * re])
        self._sq[first: first + m].copy_(ops.rows_sumsq(packed, m, re, re))
        self._size = first + m
        return range(first, first + m)


MAX_TABLE_ROWS = 0x7FFF0000        # window starts are int32 table rows
_SUMSQ_ROWS = 32768                # table rows per sda_rows_sumsq launch (one grid row each)


class WindowBank:
    """M candidate segments that are WINDOWS of continuous speech tracks: candidate m is the T rows from row starts[m] on of one
    resident table of plain rows, (L_total, pad_channels(F)) of `dtype` with the tracks back to back and the channel padding
    zero — one audio file's embedding track is stored once however many word onsets cut windows from it, where a SpeechBank
    stores rows_tp(T) * pad_channels(F) elements per candidate.  Beside the table: the candidates' global row starts (int32, on
    the device and on the host), the fp32 sum of squares of every table row, and from those the candidates' fp32 squared norms.
    retrieve, retrieve_classes and Classifier.decode* take it in a SpeechBank's place (sda_sim_gemm_windows).  16-bit storage
    only: the windowed similarity GEMM has no fp32 form and nothing falls back to materialising the windows.  A bank filled by
    several add_track() calls holds the same bytes and norms as one filled at once."""

    def __init__(self, F: int, T: int, dtype=torch.bfloat16, device="cuda"):
        if int(F) < 1 or int(T) < 1:
            raise ValueError(f"WindowBank: F and T must be positive, got F={F}, T={T}")
        if dtype == torch.float32:
            raise ValueError("WindowBank: dtype float32; the windowed similarity GEMM serves 16-bit storage only (bfloat16 or "
                             "float16) and nothing materialises the windows instead: use a SpeechBank for fp32 candidates")
        if dtype not in (torch.bfloat16, torch.float16):
            raise ValueError(f"WindowBank: dtype {dtype}; a window bank holds bfloat16 or float16")
        self.F, self.T, self.dtype = int(F), int(T), dtype
        self.device = torch.device(device)
        if self.device.type != "cuda":
            raise L.SdaError("WindowBank lives on the MI355X device (there is no CPU path)")
        self.row_elems = L.pad_channels(self.F)             # of ONE table row; a candidate is T of them
        self._size, self._capacity = 0, 0                   # candidates
        self._L, self._row_capacity = 0, 0                  # table rows
        self._store = None              # row-layout buffer of one "sample" of _row_capacity rows: table row l is its row ROW_PAD + l
        self._row_sq = None             # (_row_capacity,) fp32
        self._starts = None             # (_capacity,) int32
        self._sq = None                 # (_capacity,) fp32
        self.starts_host = np.empty(0, dtype=np.int32)
        self._table_of = None           # the bank whose table this one shares (select); None: the table is its own

    def __len__(self) -> int:
        return self._size

    def select(self, indices) -> "WindowBank":
        """A new bank whose candidates are the candidates `indices` of this one (host or device integers, one-dimensional, any
        order, duplicates allowed), in that order — the test candidates of a train / test split of the same resident tracks.  The
        table and the per-row sums are SHARED, nothing is copied; starts, starts_host and norms_sq are the result's own, taken
        from this bank's values.  The result does not own the table: its add_track raises.  Tracks added to this bank afterwards
        are not seen by the result."""
        arr = indices.detach().cpu().numpy() if torch.is_tensor(indices) else np.asarray(indices)
        if arr.ndim != 1 or arr.dtype.kind not in "iu":
            raise ValueError("WindowBank.select: indices must be a one-dimensional array of integer candidates")
        if arr.size and (int(arr.min()) < 0 or int(arr.max()) >= self._size):
            raise IndexError(f"WindowBank.select: a candidate outside [0, {self._size})")
        arr = arr.astype(np.int64)
        sub = WindowBank(self.F, self.T, dtype=self.dtype, device=self.device)
        sub._table_of = self if self._table_of is None else self._table_of
        sub._store, sub._row_sq, sub._L, sub._row_capacity = self._store, self._row_sq, self._L, self._row_capacity
        sub.starts_host = self.starts_host[arr]
        sub._size = sub._capacity = int(arr.shape[0])
        if sub._size:
            sub._starts = torch.from_numpy(sub.starts_host).to(self._starts.device)
            sub._sq = self._sq.index_select(0, torch.from_numpy(arr).to(self._sq.device))
        else:
            sub._starts, sub._sq = self._starts[:0], self._sq[:0]
        return sub

    @property
    def table(self) -> torch.Tensor:
        """(L_total, pad_channels(F)) view of the stored tracks."""
        re = self.row_elems
        return self._store[L.ROW_PAD * re: (L.ROW_PAD + self._L) * re].view(self._L, re)

    @property
    def starts(self) -> torch.Tensor:
        """(M,) int32 device tensor: the table row every candidate starts at."""
        return self._starts[: self._size]

    @property
    def norms_sq(self) -> torch.Tensor:
        """(M,) fp32 squared norms of the stored (rounded) candidates."""
        return self._sq[: self._size]

    @property
    def row_norms_sq(self) -> torch.Tensor:
        """(L_total,) fp32 sums of squares of the table's rows."""
        return self._row_sq[: self._L]

    @property
    def nbytes(self) -> int:
        """Bytes the bank's contents take: the table, the starts and norms of the candidates, the per-row sums."""
        return self._L * self.row_elems * 2 + 8 * self._size + 4 * self._L

    def _reserve(self, rows: int, capacity: int):
        """Room for `rows` table rows and `capacity` candidates; what has to grow at least doubles (SpeechBank._reserve)."""
        L.load()
        re = self.row_elems
        if rows > self._row_capacity:
            rows = max(rows, 2 * self._row_capacity)
            store = torch.empty(L.rows_alloc(1, rows) * re, dtype=self.dtype, device=self.device)
            row_sq = torch.empty(rows, dtype=torch.float32, device=self.device)
            if self._L:
                a, b = L.ROW_PAD * re, (L.ROW_PAD + self._L) * re
                store[a:b].copy_(self._store[a:b])
                row_sq[: self._L].copy_(self._row_sq[: self._L])
            self._store, self._row_sq, self._row_capacity = store, row_sq, rows
        if capacity > self._capacity:
            capacity = max(capacity, 2 * self._capacity)
            starts = torch.empty(capacity, dtype=torch.int32, device=self.device)
            sq = torch.empty(capacity, dtype=torch.float32, device=self.device)
            if self._size:
                starts[: self._size].copy_(self._starts[: self._size])
                sq[: self._size].copy_(self._sq[: self._size])
            self._starts, self._sq, self._capacity = starts, sq, capacity

    @torch.no_grad()
    def add_track(self, E: torch.Tensor, starts) -> range:
        """Append one track E (F, L) — fp32, bf16 or fp16, any strides — and the windows of T rows that begin at its rows
        `starts` (host integers in [0, L - T], any order, duplicates allowed); returns the bank indices the windows received.
        Add tracks, and the windows of a track, in time order where you can: a chunk of neighbouring candidates then reads
        neighbouring table rows, which is what the caches can keep and what the 4 GB span of one GEMM launch is counted over."""
        if self._table_of is not None:
            raise L.SdaError("WindowBank.add_track: this bank was made by select() and shares another bank's table, which it does "
                             "not own; add the track to the bank the selection was made from and select again")
        if not torch.is_tensor(E) or E.dim() != 2 or E.shape[0] != self.F or E.shape[1] < self.T:
            got = tuple(E.shape) if torch.is_tensor(E) else type(E).__name__
            raise ValueError(f"WindowBank.add_track: expected an ({self.F}, L) track with L >= {self.T}, got {got}")
        arr = starts.detach().cpu().numpy() if torch.is_tensor(starts) else np.asarray(starts)
        if arr.ndim != 1 or (arr.size and arr.dtype.kind not in "iu"):
            raise ValueError("WindowBank.add_track: starts must be a one-dimensional array of integer rows")
        rows, m, first, row0 = int(E.shape[1]), int(arr.shape[0]), self._size, self._L
        if m and (int(arr.min()) < 0 or int(arr.max()) > rows - self.T):
            raise IndexError(f"WindowBank.add_track: a start outside [0, L - T = {rows - self.T}]")
        if row0 + rows > MAX_TABLE_ROWS or first + m > MAX_M:
            raise ValueError(f"WindowBank.add_track: more than {MAX_TABLE_ROWS:#x} table rows or candidates")
        if not E.is_cuda:
            raise L.SdaError("WindowBank.add_track: E must live on the MI355X device (there is no CPU path)")
        if E.device != self.device and not (self.device.index is None and E.device.index == torch.cuda.current_device()):
            raise L.SdaError(f"WindowBank.add_track: E is on {E.device}, the bank on {self.device}")
        if E.dtype not in ops.COMPUTE_DTYPES:
            raise L.SdaError(f"WindowBank.add_track: E of dtype {E.dtype}; tracks are float32, bfloat16 or float16")
        if m == 0:
            return range(first, first)
        self._reserve(row0 + rows, first + m)
        re = self.row_elems
        # the pack writes the track as the one sample of a row-layout buffer that begins ROW_PAD rows in front of its first table
        # row: exactly the rows [row0, row0 + rows) of the table, every channel of each, and nothing else
        ops.pack_rows(E.detach().unsqueeze(0), self._store[row0 * re:].view(-1, re))
        table = self._store[L.ROW_PAD * re:]
        for r0 in range(row0, row0 + rows, _SUMSQ_ROWS):
            n = min(_SUMSQ_ROWS, row0 + rows - r0)
            self._row_sq[r0: r0 + n].copy_(ops.rows_sumsq(table[r0 * re:], n, re, re))
        glob = (arr.astype(np.int64) + row0).astype(np.int32)
        self._starts[first: first + m].copy_(torch.from_numpy(glob).to(self._starts.device))
        ops.window_sumsq(self._row_sq, self._starts[first:], m, self.T, out=self._sq[first:])
        self.starts_host = np.concatenate([self.starts_host, glob])
        self._size, self._L = first + m, row0 + rows
        return range(first, first + m)


def plan_blocks(N: int, M: int, K: int, dtype, scratch_bytes: int):
    """(nb, mc, tiles256, ksplit): queries are decoded nb rows at a time; a block's raw scores over the WHOLE bank are held
    (nb x pad64(M) fp32, at most half of scratch_bytes), filled by one GEMM per chunk of mc bank rows, each in `ksplit` K slices
    whose partial sums (ksplit x nb x mc fp32, not needed when ksplit is 1) take the rest.  Every (block, chunk) pair is
    multiplied once, so the GEMM work does not depend on the blocking.  mc starts at the whole bank and is halved (in multiples
    of 256, the GEMM's tile) while the K slices the GEMM would like do not fit; what still does not fit is run in fewer slices.
    The plan depends only on its arguments and the device's CU count, so one call always computes the same bits."""
    return _plan(N, M, K, dtype, scratch_bytes, 0)


def plan_class_blocks(N: int, M: int, C: int, K: int, dtype, scratch_bytes: int):
    """plan_blocks for retrieve_classes: a block of nb queries holds, beside its nb x pad64(M) scores, its nb x pad64(C) class
    values; the two together take at most half of scratch_bytes and the K slices' partial sums the rest, so
    4 nb (pad64(M) + pad64(C)) + 4 ksplit nb mc (the last term only when ksplit > 1) <= scratch_bytes.  ValueError when one
    query row's scores and class values do not fit twice."""
    return _plan(N, M, K, dtype, scratch_bytes, L.pad_channels(C))


def _plan(N: int, M: int, K: int, dtype, scratch_bytes: int, class_cols: int):
    Mp = L.pad_channels(M)
    row = 4 * (Mp + class_cols)                  # bytes one query row holds between the GEMM and the selection
    if scratch_bytes < 2 * row:
        if class_cols:
            raise ValueError(f"retrieve_classes: scratch_bytes={scratch_bytes} does not hold one query's scores over the bank "
                             f"and its class values twice ({2 * row} bytes)")
        raise ValueError(f"retrieve: scratch_bytes={scratch_bytes} does not hold one query's scores over the bank twice ({8 * Mp} bytes)")
    nb = min(N, scratch_bytes // 2 // row)
    if nb >= 256:
        nb = nb // 256 * 256
    budget = scratch_bytes - nb * row
    mc = Mp
    if dtype == torch.float32:
        # fp32 storage runs on conv_gemm's matrix mode: a chunk's operand stays inside 2 GB, the spans that mode is run at
        mc = min(mc, max(64, ((1 << 31) // (4 * K)) // 64 * 64))
    while True:
        tiles256, ks = ops.splitk_plan(dtype, nb, min(mc, M), K, K)
        if ks == 1 or 4 * ks * nb * mc <= budget or mc <= 256:
            break
        mc = max(256, (mc // 2 + 255) // 256 * 256)
    ks = max(1, min(ks, budget // (4 * nb * mc)))
    return nb, mc, tiles256, ks


def _checked_k(who: str, k, what: str = "", size: int = MAX_K) -> int:
    if isinstance(k, bool) or int(k) != k or not 1 <= k <= min(MAX_K, size):
        raise ValueError(f"{who}: k={k} outside 1 ... " + (f"min({MAX_K}, {what}={size})" if what else f"{MAX_K}"))
    return int(k)


def _checked_labels(who: str, labels, N: int, size: int, noun: str, whose: str):
    """Device labels as an int64 device tensor; host labels, range-checked, as an int64 numpy array (uploaded later).  `noun`
    ("bank indices" / "class ids") and `whose` ("the bank's" / "the classes'") word the caller's messages."""
    if torch.is_tensor(labels) and labels.is_cuda:
        if labels.dim() != 1 or labels.shape[0] != N or labels.dtype.is_floating_point or labels.dtype == torch.bool:
            raise ValueError(f"{who}: labels must be {N} integer {noun}")
        return labels.to(torch.int64).contiguous()          # checked by the kernel: a value outside [0, size) gives rank -1
    arr = labels.detach().numpy() if torch.is_tensor(labels) else np.asarray(labels)
    if arr.shape != (N,) or arr.dtype.kind not in "iu":
        raise ValueError(f"{who}: labels must be {N} integer {noun}")
    if (arr < 0).any() or (arr >= size).any():
        raise IndexError(f"{who}: label outside {whose} [0, {size})")
    return arr.astype(np.int64)


class _ScorePass:
    """The blocked score pass under retrieve and retrieve_classes (`who`: the name in every message), in the order both keep:
    __init__ checks the shared arguments and the caller then its own and its plan (ValueError, nothing is touched); on_device
    refuses what the kernels cannot read (SdaError); start touches the device first: host labels go up, the queries are packed,
    their norms taken, the scratch allocated; blocks() fills S with one block of queries' scores after the other."""

    def __init__(self, who: str, queries: torch.Tensor, bank, k=None):
        if not isinstance(bank, (SpeechBank, WindowBank)):
            raise ValueError(f"{who}: bank must be a SpeechBank or a WindowBank")
        if not torch.is_tensor(queries) or queries.dim() != 3 or queries.shape[0] < 1:
            raise ValueError(f"{who}: queries must be an (N, F, T) tensor with N >= 1")
        N, F, T = queries.shape
        if (F, T) != (bank.F, bank.T):
            raise ValueError(f"{who}: queries are (N, {F}, {T}), the bank holds ({bank.F}, {bank.T}) segments")
        if k is not None:                                   # retrieve holds k to MAX_K before it looks at the bank's size
            self.k = _checked_k(who, k)
        if len(bank) == 0:
            raise ValueError(f"{who}: the bank is empty")
        self.who, self.queries, self.bank = who, queries, bank
        self.N, self.F, self.M = N, F, len(bank)
        # the packed queries are rows of rows_tp(T) * pad_channels(F) elements.  Against a SpeechBank, whose candidates are packed
        # the same way, the contraction runs over the whole row (pad rows are zero on both sides); against a WindowBank over the T
        # valid rows only, from the query's ROW_PAD-th row on: the rows in front of a window belong to other candidates.
        self.windows = isinstance(bank, WindowBank)
        self.q_pitch = L.rows_tp(T) * L.pad_channels(F)
        self.q_skip = L.ROW_PAD * L.pad_channels(F) if self.windows else 0
        self.K = self.q_pitch - self.q_skip

    def on_device(self) -> torch.device:
        who, queries = self.who, self.queries
        if not queries.is_cuda:
            raise L.SdaError(f"{who}: queries must live on the MI355X device (there is no CPU path)")
        held = self.bank.table if self.windows else self.bank.rows
        if queries.device != held.device:
            raise L.SdaError(f"{who}: queries are on {queries.device}, the bank on {held.device}")
        if queries.dtype not in ops.COMPUTE_DTYPES:
            raise L.SdaError(f"{who}: queries of dtype {queries.dtype}; segments are float32, bfloat16 or float16")
        return queries.device

    def start(self, plan, labels=None):
        """Takes the (nb, mc, tiles256, ksplit) of plan_blocks / plan_class_blocks; returns the labels as the kernels read them."""
        self.nb, self.mc, self.tiles256, self.ks = nb, mc, _, ks = plan
        N, bank, dev = self.N, self.bank, self.queries.device
        if self.windows and not self.tiles256:
            raise L.SdaError(f"{self.who}: the windowed similarity GEMM does not serve this shape (there is no other path)")
        if isinstance(labels, np.ndarray):
            labels = ops.upload_small(labels, dev)
        self.Qt = ops.rows_of(self.queries, self.F, bank.dtype)[0].reshape(-1)
        self.qsq = ops.rows_sumsq(self.Qt, N, self.q_pitch, self.q_pitch)
        self.Bt, self.csq = (bank.table if self.windows else bank.rows).reshape(-1), bank.norms_sq
        if self.windows:             # (smallest, largest) start of every chunk of mc candidates, from the host copy
            self.spans = [(int(c.min()), int(c.max())) for c in (bank.starts_host[c0: c0 + mc] for c0 in range(0, self.M, mc))]
        self.S = torch.empty(ops.retrieval_scores_floats(nb, self.M, mc), dtype=torch.float32, device=dev)
        self.partial = torch.empty(ks * nb * mc if ks > 1 else 0, dtype=torch.float32, device=dev)
        return labels

    def chunk(self, c0: int, n: int) -> torch.Tensor:
        """S from an n-row block's scores against bank row c0 (a multiple of mc) on.  S is chunk-major, one [n][pad64(m)] matrix
        per chunk of m bank rows: this offset and score_ptr in csrc/retrieval.hip are the two places that say so."""
        mc = self.mc
        return self.S[(c0 // mc) * n * mc:]

    def fill(self, i0: int = 0) -> int:
        """Fill S with the raw dot products of queries i0 ... i0 + n - 1 against the whole bank, one GEMM per chunk; returns n."""
        M, K, mc, Bt = self.M, self.K, self.mc, self.Bt
        Q = self.Qt[self.q_skip + i0 * self.q_pitch:]
        n = min(self.nb, self.N - i0)
        for c0 in range(0, M, mc):
            m = min(mc, M - c0)
            if self.windows:
                lo, hi = self.spans[c0 // mc]
                ops.sim_gemm_windows_into(Q, self.q_pitch, Bt, self.bank.starts[c0: c0 + m], lo, hi, self.bank.row_elems, n, m, K,
                                          self.ks, self.partial, self.chunk(c0, n))
            else:
                ops.matmul_nt_splitk_into(Q, Bt[c0 * K:], n, m, K, K, self.tiles256, self.ks, self.partial, self.chunk(c0, n))
        return n

    def blocks(self):
        """(i0, n) of every block of queries in turn, S filled for it."""
        for i0 in range(0, self.N, self.nb):
            yield i0, self.fill(i0)


@torch.no_grad()
def retrieve(queries: torch.Tensor, bank, k: int = 10, labels=None, scratch_bytes: int = 1 << 30) -> Retrieval:
    """Score the N segments of `queries` (N, F, T) against every candidate of `bank` (a SpeechBank or a WindowBank) and return the k best of each
    (Retrieval); with `labels` (N integer bank indices, host or device) also the rank of each query's true candidate over the
    whole bank.  Labels on the host are checked here (IndexError); labels on the device are checked by the kernel, which
    reports -1 for one outside the bank, because nothing is read back: the results are device tensors.  `scratch_bytes`
    bounds the temporary memory (plan_blocks); the same call with the same arguments returns the same bits."""
    sp = _ScorePass("retrieve", queries, bank, k)
    N, M = sp.N, sp.M
    k = _checked_k("retrieve", sp.k, "M", M)
    if labels is not None:
        labels = _checked_labels("retrieve", labels, N, M, "bank indices", "the bank's")
    plan = plan_blocks(N, M, sp.K, bank.dtype, int(scratch_bytes))
    dev = sp.on_device()
    labels = sp.start(plan, labels)
    indices = torch.empty((N, k), dtype=torch.int64, device=dev)
    scores = torch.empty((N, k), dtype=torch.float32, device=dev)
    ranks = torch.empty(N, dtype=torch.int32, device=dev) if labels is not None else None
    for i0, n in sp.blocks():
        ops.retrieval_select(sp.S, sp.qsq[i0:], sp.csq, n, M, k, sp.mc, labels=None if labels is None else labels[i0:],
                             indices=indices[i0:], scores=scores[i0:], ranks=None if ranks is None else ranks[i0:])
    return Retrieval(indices, scores, ranks)


# ---------------------------------------------------------------------------------------------------------------------------
# word-level decoding: the bank's candidates fall into classes; a class's score is the softmax mass of all its instances
# ---------------------------------------------------------------------------------------------------------------------------
MAX_M = 0x7FFF0000  # the selection kernel's column limit
REDUCE_MODES = ("sum", "mean", "max")


class ClassIndex:
    """Which class (word) each of a bank's M candidates belongs to, as the CSR index the class kernels read.  `classes`: M
    integer class ids in bank order (list, numpy array or tensor).  Built once on the host with a stable numpy sort:
    order (M,) int32, the bank rows sorted by class and ascending inside a class; offsets (C + 1,) int32; counts (C,) int64,
    with C = num_classes or max id + 1.  Classes without a member are allowed.  order and offsets are uploaded to `device` the
    first time a kernel asks for them (order_dev, offsets_dev) and stay there."""

    def __init__(self, classes, num_classes: Optional[int] = None, device="cuda"):
        arr = classes.detach().cpu().numpy() if torch.is_tensor(classes) else np.asarray(classes)
        if arr.ndim != 1 or arr.shape[0] < 1:
            raise ValueError("ClassIndex: classes must be M >= 1 class ids, one per bank row")
        if arr.dtype.kind not in "iu":
            raise ValueError(f"ClassIndex: class ids must be integers, got {arr.dtype}")
        if arr.shape[0] > MAX_M:
            raise ValueError(f"ClassIndex: M={arr.shape[0]} above {MAX_M:#x}")
        if num_classes is not None and (isinstance(num_classes, bool) or int(num_classes) != num_classes or num_classes < 1):
            raise ValueError(f"ClassIndex: num_classes={num_classes} must be a positive integer")
        if arr.dtype.kind == "i" and (arr < 0).any():
            raise ValueError("ClassIndex: negative class id")
        top = int(arr.max())
        C = top + 1 if num_classes is None else int(num_classes)
        if top >= C:
            raise ValueError(f"ClassIndex: class id {top} outside [0, num_classes={C})")
        if C > MAX_M:
            raise ValueError(f"ClassIndex: {C} classes above {MAX_M:#x}")
        arr = arr.astype(np.int64)
        self.M, self.C = int(arr.shape[0]), C
        self.classes = arr
        self.order = np.argsort(arr, kind="stable").astype(np.int32)
        self.counts = np.bincount(arr, minlength=C).astype(np.int64)
        self.offsets = np.concatenate([[0], np.cumsum(self.counts)]).astype(np.int32)
        self.device = torch.device(device)
        self._dev = None

    def __len__(self) -> int:
        return self.M

    def _upload(self):
        if self._dev is None:
            if self.device.type != "cuda":
                raise L.SdaError("ClassIndex: the class kernels run on the MI355X device (there is no CPU path)")
            self._dev = (torch.from_numpy(self.order).to(self.device), torch.from_numpy(self.offsets).to(self.device))
        return self._dev

    @property
    def order_dev(self) -> torch.Tensor:
        return self._upload()[0]

    @property
    def offsets_dev(self) -> torch.Tensor:
        return self._upload()[1]


class ClassRetrieval(NamedTuple):
    """classes (R, k) int64: the k best classes of every result row, best first (value descending, lower class id first on
    equal values; classes without a member carry -inf and come last); log_probs (R, k) fp32: their values (log-probabilities
    for reduce="sum"); ranks (R,) int32 or None: classes that beat the true one (0 = top-1; -1 for a device label outside
    [0, C)); matrix (R, C) fp32 or None: the whole value matrix (return_matrix=True).  R = N, or G with groups.  All on the
    device."""
    classes: torch.Tensor
    log_probs: torch.Tensor
    ranks: Optional[torch.Tensor]
    matrix: Optional[torch.Tensor]

    def accuracy(self, k: int) -> float:
        """Share of result rows whose true class is among the k best (reads the ranks back)."""
        if self.ranks is None:
            raise ValueError("ClassRetrieval.accuracy: retrieve_classes() was called without labels")
        return float(((self.ranks >= 0) & (self.ranks < k)).float().mean())


def _group_index(groups, N: int):
    """groups (N ids in [0, G), every group non-empty) -> (rows (N,) int32 sorted by group, ascending inside; offsets (G + 1,))."""
    arr = groups.detach().cpu().numpy() if torch.is_tensor(groups) else np.asarray(groups)
    if arr.shape != (N,) or arr.dtype.kind not in "iu":
        raise ValueError(f"retrieve_classes: groups must be {N} integer group ids")
    if (arr < 0).any():
        raise ValueError("retrieve_classes: negative group id")
    arr = arr.astype(np.int64)
    counts = np.bincount(arr)
    if (counts == 0).any():
        raise ValueError(f"retrieve_classes: group {int(np.argmin(counts))} has no query (groups are 0 ... G - 1, none empty)")
    return np.argsort(arr, kind="stable").astype(np.int32), np.concatenate([[0], np.cumsum(counts)]).astype(np.int32)


@torch.no_grad()
def retrieve_classes(queries: torch.Tensor, bank, classes, k: int = 10, scale: float = 1.0, reduce: str = "sum",
                     labels=None, groups=None, return_matrix: bool = False, scratch_bytes: int = 1 << 30) -> ClassRetrieval:
    """Word-level decoding: score the N segments of `queries` against every candidate of `bank` (a SpeechBank or a WindowBank), pool the scores of the
    candidates of one class, and return the k best CLASSES of each query (ClassRetrieval).  `classes`: a ClassIndex over the
    bank's M rows, or the M class ids themselves.  The logit of query i against candidate j is scale * cos(i, j), cos the
    similarity retrieve() uses and `scale` a positive finite float (a trained CLIPLoss: float(loss.temp.exp())); class c gets
        reduce="sum":  logsumexp of its members' logits (its probability mass)      "mean": that minus log n_c
        reduce="max":  its best member's logit                                     a class without members: -inf
    minus the log-sum-exp of the row's M logits, so "sum" returns log-probabilities that sum to one over the classes.
    `groups` (N integer ids in [0, G), none empty, or None): queries of one group are repetitions of one item — the same
    stimulus heard by several subjects or several times; their values are pooled as log mean exp per class and the result has
    G rows.  Groups may be interleaved.  `labels`: the true class per result row (N, or G with groups), host (range-checked
    here, IndexError) or device (checked by the kernel: rank -1), as in retrieve().
    Memory: `scratch_bytes` bounds a query block's scores, its class values and the GEMM's partial sums (plan_class_blocks).
    With `groups` or `return_matrix` the (N x pad64(C)) fp32 value matrix — and with groups the (G x pad64(C)) pooled one — is
    held whole: that is a result-sized allocation outside the bound.  No gradients, no collective; the same call returns the
    same bits."""
    sp = _ScorePass("retrieve_classes", queries, bank)
    N, M = sp.N, sp.M
    index = classes if isinstance(classes, ClassIndex) else ClassIndex(classes, device=bank.device)
    if index.M != M:
        raise ValueError(f"retrieve_classes: the class index covers {index.M} candidates, the bank holds {M}")
    C = index.C
    k = _checked_k("retrieve_classes", k, "C", C)
    if isinstance(scale, bool) or not isinstance(scale, (int, float, np.floating)) or not 0.0 < float(scale) <= float(np.finfo(np.float32).max) \
            or float(np.float32(scale)) == 0.0:
        raise ValueError(f"retrieve_classes: scale={scale!r} must be a positive finite float")
    if reduce not in REDUCE_MODES:
        raise ValueError(f"retrieve_classes: reduce={reduce!r}; one of {REDUCE_MODES}")
    gidx = None if groups is None else _group_index(groups, N)
    R = N if gidx is None else len(gidx[1]) - 1
    if labels is not None:
        labels = _checked_labels("retrieve_classes", labels, R, C, "class ids", "the classes'")
    plan = plan_class_blocks(N, M, C, sp.K, bank.dtype, int(scratch_bytes))
    dev = sp.on_device()
    order, offsets = index.order_dev, index.offsets_dev
    if order.device != dev:
        raise L.SdaError(f"retrieve_classes: the class index is on {order.device}, the queries on {dev}")
    labels = sp.start(plan, labels)
    nb, Cp = sp.nb, L.pad_channels(C)
    whole = gidx is not None or return_matrix                # the value matrix is kept: a result-sized allocation
    V = torch.empty((N if whole else nb, Cp), dtype=torch.float32, device=dev)
    row_lse = torch.empty(nb, dtype=torch.float32, device=dev)
    ones = torch.ones(max(R if whole else nb, C), dtype=torch.float32, device=dev)      # unit norms: the selection divides by 1
    top = torch.empty((R, k), dtype=torch.int64, device=dev)
    vals = torch.empty((R, k), dtype=torch.float32, device=dev)
    ranks = torch.empty(R, dtype=torch.int32, device=dev) if labels is not None else None
    for i0, n in sp.blocks():
        Vb = V[i0:] if whole else V
        ops.retrieval_class_reduce(sp.S, sp.qsq[i0:], sp.csq, order, offsets, n, M, C, float(scale), reduce, sp.mc, out=Vb, row_lse=row_lse)
        if not whole:
            ops.retrieval_select(V, ones, ones, n, C, k, Cp, labels=None if labels is None else labels[i0:],
                                 indices=top[i0:], scores=vals[i0:], ranks=None if ranks is None else ranks[i0:])
    if whole:
        if gidx is not None:
            V = ops.retrieval_pool_rows(V, torch.from_numpy(gidx[0]).to(dev), torch.from_numpy(gidx[1]).to(dev), N, R, C)
        ops.retrieval_select(V, ones, ones, R, C, k, Cp, labels=labels, indices=top, scores=vals, ranks=ranks)
    return ClassRetrieval(top, vals, ranks, V[:, :C] if return_matrix else None)
