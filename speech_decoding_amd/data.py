"""Per-rank data feed for the training step: the reference's sampler cut into rank shards, and the segment gather +
batch collate on the GPU in the loop.

What it mirrors (SeanNobel/speech-decoding):
  * utils/get_dataloaders.py:48-87 (`get_samplers`): `RandomSampler(train_set, replacement=True, num_samples=updates *
    batch_size, generator=g)` consumed in batches of `batch_size` — here the SAME index stream is generated on every rank
    from the same seeded generator and rank r keeps positions [r * B_local, (r + 1) * B_local) of each global batch
    (`ShardedRandomSampler`): no rank ever materialises another rank's samples, and the union over ranks is exactly the
    single-process batch;
  * dataclass/gwilliams2022.py:129-142 (`__getitem__`: a speech segment i -> a random recording of that task, the MEG
    window at the segment's onset, the subject index) and :640-661 (`Gwilliams2022Collator`: baseline correction, robust
    scaling, clamp) — here `ResidentSegmentFeed`: the recordings stay in HBM, a batch is (recording, onset) pairs turned
    into X (B, C, T) by ONE kernel (collate.ResidentSegments), Y rows are gathered from the resident embedding table — or, with
    a retrieval.WindowBank as Y, from the embedding TRACKS themselves: gwilliams2022.py embeds each audio file once and cuts a
    window per word onset; it materialises every window of the speech side (`self.Y[i]`), here sda_gather_windows writes a
    batch's windows straight into the loss's row layout and each track is stored once (`synthetic_track_dataset`);
  * dataclass/brennan2018.py:72-152 (shift, trim, RobustScaler + clamp over the WHOLE recording per subject and channel or
    per channel with the subjects pooled, split into chunks, baseline correction per chunk; `__getitem__`: chunk i of a
    random subject) — here `ResidentSubjectFeed`: the (S, C, L) array is scaled once on the device by exact order statistics
    (collate.robust_stats / scale_clamp_rows) and stays resident; a batch is (subject, chunk) pairs turned into X by one
    kernel (collate.gather_baseline_windows).

Written once: `segment_dims` (the sizes every stand-in and train.py read out of `args`), `_ResidentEmbeddings` (the speech side and
`batches()`, for both feeds: a feed says what it draws for a batch and under which keyword `batch()` takes it), and
`_synthetic_gwilliams` (the Gwilliams2022 stand-in: `synthetic_resident_dataset` and `synthetic_track_dataset` differ only in the
speech side they attach).
"""
from __future__ import annotations

from typing import Iterator, NamedTuple, Sequence, Tuple

import numpy as np
import torch

from . import collate as _collate
from . import lib as _lib
from . import ops
from .collate import ResidentSegments
from .lib import SdaError
from .retrieval import WindowBank


class ShardedRandomSampler:
    """Indices of `updates` global batches of `batch_size` drawn with replacement from range(n) (get_dataloaders.py:57-62),
    rank `rank` of `world` keeping its contiguous slice of every global batch.  Every rank runs the same generator, so the
    global batch is well defined without any communication."""

    def __init__(self, n: int, batch_size: int, updates: int, rank: int = 0, world: int = 1, seed: int = 0, replacement: bool = True):
        if batch_size % world:
            raise ValueError("the global batch must divide evenly over the ranks")
        self.n, self.batch_size, self.updates, self.rank, self.world = int(n), int(batch_size), int(updates), int(rank), int(world)
        self.replacement = bool(replacement)
        self.gen = torch.Generator().manual_seed(int(seed))

    def global_batches(self) -> Iterator[torch.Tensor]:
        for _ in range(self.updates):
            if self.replacement:
                yield torch.randint(0, self.n, (self.batch_size,), generator=self.gen)
            else:
                yield torch.randperm(self.n, generator=self.gen)[: self.batch_size]

    def __iter__(self) -> Iterator[torch.Tensor]:
        per = self.batch_size // self.world
        for idx in self.global_batches():
            yield idx[self.rank * per: (self.rank + 1) * per]

    def __len__(self) -> int:
        return self.updates


def check_track_dtype(who: str, dtype):
    """SdaError unless `dtype` is one a track-backed feed can hold (train.py data=tracks asks before it builds anything)."""
    if dtype not in (torch.bfloat16, torch.float16):
        raise _tracks_are_16bit(who, dtype)


def _tracks_are_16bit(who: str, dtype) -> Exception:
    return SdaError(f"{who}: dtype {dtype}; speech tracks are 16-bit (a WindowBank holds bfloat16 or float16 and nothing "
                    "materialises its windows instead): fp32 training uses materialised Y (N, F, T) segments")


class SegmentDims(NamedTuple):
    C: int        # M/EEG channels
    T: int        # samples per segment
    nb: int       # of them baseline
    F: int        # speech embedding channels
    S: int        # subjects


def segment_dims(args) -> SegmentDims:
    """(C, T, nb, F, S) as the stand-in datasets and train.py read them out of `args`."""
    rate = args.preprocs["brain_resample_rate"]
    return SegmentDims(C=int(args.get("num_channels", 208 if args.dataset == "Gwilliams2022" else 60)),
                       T=int(args.preprocs["seq_len_sec"] * rate), nb=int(args.preprocs["baseline_len_sec"] * rate),
                       F=1024 if args.preprocs["last4layers"] else int(args.F), S=int(args.num_subjects))


class _ResidentEmbeddings:
    """What the resident feeds share.  The speech side, one gather per batch: Y is (N, F, T) embeddings on the device, optionally
    kept as a row-layout table in the compute dtype (pack_embeddings), or a retrieval.WindowBank whose candidate i is segment i:
    the segments are then windows of resident tracks, each track stored once, and a batch is gathered from the bank's table
    (ops.gather_windows) — nothing materialises the windows.  And batches(): a feed names the keyword under which its batch()
    takes what it draws from `rng` per item (`drawn_as`) and draws it for any set of segments (`draw_for`)."""

    Y: torch.Tensor           # or a retrieval.WindowBank
    _Yt = None                # row-layout table in the compute dtype (set by pack_embeddings only)
    drawn_as: str             # "rec" / "subjects"; draw_for(ii) makes one such draw from the feed's generator per segment of ii

    def batches(self, sampler, index_map=None, with_ids: bool = False) -> Iterator[Tuple[torch.Tensor, ...]]:
        """One (X, Y, subject_idxs) per batch of `sampler`.  With a ShardedRandomSampler of more than one rank the draw (the
        recording of a segment, the subject of a chunk) is made for EVERY item of the global batch on every rank from the same
        generator state and the rank keeps its slice — the union over the ranks is exactly the batch a single process would have
        drawn, and no two ranks share a draw.  `index_map`: optional array mapping sampler indices to segment indices (a train
        split).  `with_ids`: yield the reference's 4-tuple (X, Y, subject_idxs, chunkIDs) instead (train.py:179-183), chunkIDs =
        speech_ids() of the batch's segments as a host int64 tensor — what CLIPLoss.forward takes as `labels`."""
        def item(ii, **drawn):
            out = self.batch(ii, **drawn)
            return (*out, torch.from_numpy(self.speech_ids(ii))) if with_ids else out

        if hasattr(sampler, "global_batches") and getattr(sampler, "world", 1) > 1:
            per = sampler.batch_size // sampler.world
            lo = sampler.rank * per
            for gidx in sampler.global_batches():
                g = gidx.numpy() if index_map is None else np.asarray(index_map)[gidx.numpy()]
                drawn = self.draw_for(g)
                yield item(g[lo: lo + per], **{self.drawn_as: drawn[lo: lo + per]})
            return
        for idx in sampler:
            i = idx.numpy() if isinstance(idx, torch.Tensor) else np.asarray(idx)
            yield item(i if index_map is None else np.asarray(index_map)[i])

    def speech_ids(self, idx) -> np.ndarray:
        """One int64 id per segment of `idx` that is equal for two segments exactly when they carry the same speech: the
        segment (chunk) index itself where Y holds materialised segments; for a WindowBank-backed feed the window's first row in
        the bank's table, so two candidates cut from the same track at the same start share an id."""
        ii = np.asarray(torch.as_tensor(idx, dtype=torch.int64).numpy(), dtype=np.int64).reshape(-1)
        bank = self._bank()
        if bank is None:
            return ii.copy()
        self._check_segments(ii)
        return bank.starts_host[ii].astype(np.int64)

    def _bank(self):
        """The WindowBank behind Y, or None when Y holds materialised segments."""
        return self.Y if isinstance(self.Y, WindowBank) else None

    def _check_segments(self, ii: np.ndarray):
        """Bank-backed feeds: every segment index is a candidate of the bank (checked on the host, before any launch)."""
        n = len(self.Y)
        if len(ii) and (int(ii.min()) < 0 or int(ii.max()) >= n):
            raise IndexError(f"segment index outside the bank's [0, {n})")

    def speech_bank(self, indices=None):
        """The WindowBank the feed's segments are windows of; with `indices` (segment indices, e.g. a test split) the bank of
        those candidates, in that order, sharing the same resident table (WindowBank.select) — what retrieve / retrieve_classes
        decode against."""
        bank = self._bank()
        if bank is None:
            raise SdaError("speech_bank: this feed holds materialised Y (N, F, T) segments, not a WindowBank")
        return bank if indices is None else bank.select(indices)

    negatives_seed = 0x6E6567     # of draw_negatives' own generator: the same on every rank
    _neg_rng = None

    def draw_negatives(self, n: int, batch_segments, pool) -> np.ndarray:
        """`n` distinct segment indices out of `pool` (the train split) none of which carries the speech id of any segment of
        `batch_segments` (the GLOBAL batch, on every rank alike) — what CLIPLoss.forward takes as `negatives` once speech_bank()
        has selected them.  Drawn without replacement from a generator of the feed's own that nothing else uses (seeded with
        `negatives_seed` at the first call: every rank makes the same draws; `rng` and NumPy's global generator stay reserved
        as described above, and a run that never asks consumes nothing).  ValueError when the pool cannot supply `n`."""
        bank = self._bank()
        if bank is None:
            raise SdaError("draw_negatives: this feed holds materialised Y (N, F, T) segments, not a WindowBank")
        n = int(n)
        if n < 1:
            raise ValueError(f"draw_negatives: n={n} must be at least 1")
        pool = np.unique(np.asarray(pool, dtype=np.int64).reshape(-1))
        batch = np.asarray(torch.as_tensor(batch_segments, dtype=torch.int64).numpy(), dtype=np.int64).reshape(-1)
        self._check_segments(pool)
        self._check_segments(batch)
        ids = bank.starts_host
        free = pool[~np.isin(ids[pool], ids[batch])]
        if len(free) < n:
            raise ValueError(f"draw_negatives: the pool holds {len(free)} segments whose speech is not in the batch, {n} were asked for")
        if self._neg_rng is None:
            self._neg_rng = np.random.RandomState(self.negatives_seed)
        return free[self._neg_rng.choice(len(free), size=n, replace=False)]

    def pack_embeddings(self, dtype: torch.dtype, chunk: int = 128):
        """Keep the speech embeddings resident as a row-layout table in `dtype` (the encoder's compute dtype): batch() then
        hands out Y as a zero-copy (B, F, T) view of ONE gather kernel's output, which CLIPLoss consumes as its packed operand —
        per step 0.4 GB of HBM traffic instead of the 1.3 GB of index_select + sda_pack_rows (batch 256, bf16).  Values: each
        embedding is rounded to `dtype` once here instead of once per step in the loss's pack — the same numbers."""
        bank = self._bank()
        if bank is not None:
            # windows of resident tracks are already the loss's operand in the bank's dtype: no copy is made, and none CAN be
            # made in another dtype without materialising every window
            if dtype == bank.dtype:
                return self
            if dtype == torch.float32:
                raise _tracks_are_16bit("pack_embeddings", dtype)
            raise SdaError(f"pack_embeddings: dtype {dtype}, but the feed's WindowBank holds {bank.dtype} tracks; build the bank "
                             "in the encoder's compute dtype")
        N, F, T = self.Y.shape
        Tp, Fp = _lib.rows_tp(T), _lib.pad_channels(F)
        table = torch.zeros((N * Tp + _lib.rows_alloc(1, T) - Tp, Fp), dtype=dtype, device=self.Y.device)
        for k in range(0, N, chunk):
            n = min(chunk, N - k)
            ops.pack_rows(self.Y[k: k + n], table[k * Tp:])
        self._Yt = table
        return self

    def _gather_Y(self, ii: np.ndarray) -> torch.Tensor:
        """Y of the segments `ii` (host int64 indices; duplicates allowed; a bank-backed feed's batch() has checked them)."""
        bank = self._bank()
        if bank is not None:
            # segments are windows of resident tracks: ONE kernel writes the whole row-layout batch (pad rows and slack included)
            # from the bank's table, and the view below is the loss's packed operand like the pack_embeddings form's
            ii = np.asarray(ii, dtype=np.int64)
            B = len(ii)
            with torch.cuda.device(bank.table.device):
                rows = ops.gather_windows(bank.table, bank.starts, ops.upload_small(ii, bank.table.device), B, bank.T)
            return ops.rows_view(rows, B, bank.F, bank.T)
        if self._Yt is not None:
            # embeddings resident in ROW LAYOUT in the compute dtype (pack_embeddings): the gathered batch IS the loss's packed
            # operand — CLIPLoss recognises the view and neither copies nor re-packs it
            B, (F, T) = len(ii), self.Y.shape[1:]
            with torch.cuda.device(self._Yt.device):
                return ops.rows_view(ops.gather_samples(self._Yt, ops.upload_small(ii, self._Yt.device), B, T), B, F, T)
        if self.Y.is_cuda:
            with torch.cuda.device(self.Y.device):
                return self.Y.index_select(0, ops.upload_small(ii, self.Y.device))    # (index table in kernel arguments: no host wait)
        return self.Y.index_select(0, torch.as_tensor(ii, dtype=torch.int64))


class ResidentSegmentFeed(_ResidentEmbeddings):
    """recordings: list of (C, L_r) device tensors, one per (subject, session) recording, each with the subject index
    `rec_subject[r]` and the task `rec_task[r]` it recorded; onsets[r][j] = first MEG sample of the j-th speech segment of
    that task; seg_task[i], seg_in_task[i] = (task, position) of global speech segment i (gwilliams2022.py: `segment_to_task`);
    Y (N, F, T) speech embeddings, resident — or a retrieval.WindowBank of N candidates, candidate i being segment i as a window
    of its task's embedding track (the reference embeds each audio file once and cuts a window per word onset; it materialises
    them, self.Y[i], here the tracks stay whole).  batch(idx) -> (X, Y, subject_idxs) with X collated on the device."""

    def __init__(self, recordings: Sequence[torch.Tensor], rec_subject: Sequence[int], rec_task: Sequence[int],
                 onsets: Sequence[np.ndarray], seg_task: np.ndarray, seg_in_task: np.ndarray, Y, *,
                 seq_len_samp: int, baseline_len_samp: int, clamp_lim: float, clamp: bool = True, seed: int = 0):
        self.rs = ResidentSegments(list(recordings), seq_len_samp, baseline_len_samp, clamp_lim, clamp)
        self.rec_subject = np.asarray(rec_subject, dtype=np.int32)
        self.rec_task = np.asarray(rec_task)
        self.onsets = [np.asarray(o, dtype=np.int64) for o in onsets]
        self.seg_task, self.seg_in_task = np.asarray(seg_task), np.asarray(seg_in_task)
        self.Y = Y
        if self._bank() is not None and len(Y) != len(self.seg_task):
            raise ValueError(f"the WindowBank holds {len(Y)} candidates for {len(self.seg_task)} segments (candidate i is segment i)")
        self.by_task = {int(t): np.nonzero(self.rec_task == t)[0] for t in np.unique(self.rec_task)}
        # (gwilliams2022.py:133 draws the recording from NumPy's GLOBAL generator inside DataLoader workers; the global
        # generator stays reserved for SpatialDropout's centre here — every rank must draw that one in lockstep)
        self.rng = np.random.RandomState(seed)
        # dense tables for the vectorised draw / onset lookup (None where the structure is ragged: the loops remain)
        self._task_keys = np.array(sorted(self.by_task), dtype=self.rec_task.dtype)
        counts = {len(v) for v in self.by_task.values()}
        self._rec_table = np.stack([self.by_task[int(t)] for t in self._task_keys]) if len(counts) == 1 else None
        lens = {len(o) for o in self.onsets}
        self._onset_table = np.stack(self.onsets) if len(lens) == 1 else None

    def __len__(self) -> int:
        return len(self.Y) if self._bank() is not None else int(self.Y.shape[0])

    def draw_recordings(self, idx) -> np.ndarray:
        """gwilliams2022.py:133: one random recording of each segment's task, drawn item by item from the feed's generator
        (`rng.choice(recordings of the task)`).  When every task has the same number of recordings the whole batch is ONE
        vectorised draw — the same stream of values as the item-by-item calls (checked in tests/test_host_cpu.py), without
        256 Python-level generator calls in front of a 7 ms step."""
        ii = np.asarray(idx, dtype=np.int64)
        tasks = self.seg_task[ii]
        if self._rec_table is not None:
            u = self.rng.randint(0, self._rec_table.shape[1], size=len(ii))
            return self._rec_table[np.searchsorted(self._task_keys, tasks), u].astype(np.int64)
        return np.array([self.rng.choice(self.by_task[int(t)]) for t in tasks], dtype=np.int64)

    drawn_as = "rec"

    def draw_for(self, ii: np.ndarray) -> np.ndarray:
        return self.draw_recordings(ii)

    def batch(self, idx, rec=None) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor]:
        """idx: this rank's global segment indices; rec: their recordings when the caller drew them (data parallelism: the
        draws are made for the GLOBAL batch on every rank alike and sliced, see batches())."""
        idx = torch.as_tensor(idx, dtype=torch.int64)
        ii = idx.numpy()
        if self._bank() is not None:
            self._check_segments(ii)
        rec = self.draw_recordings(ii) if rec is None else np.asarray(rec, dtype=np.int64)
        on = self._onset_of(rec, self.seg_in_task[ii])
        X = self.rs.batch(rec, on)
        Y = self._gather_Y(ii)
        return X, Y, torch.from_numpy(self.rec_subject[rec].astype(np.int32))

    def _onset_of(self, rec: np.ndarray, j: np.ndarray) -> np.ndarray:
        if self._onset_table is not None:
            return self._onset_table[rec, j]
        return np.array([self.onsets[r][k] for r, k in zip(rec, j)], dtype=np.int64)


def _synthetic_gwilliams(args, device, speech_side, *, n_segments: int, n_tasks: int, seed: int, recs_per_task: int,
                         hop: int = None) -> Tuple[ResidentSegmentFeed, np.ndarray, np.ndarray]:
    """The stand-in behind synthetic_resident_dataset and synthetic_track_dataset: recordings, subjects, tasks, onsets, segment
    tables, the read-out P, the feed and the split.  `speech_side(P, firsts, speech_onsets, seg_task, seg_in_task, g)` returns the
    feed's Y from the tasks' FIRST recordings (host copies) and their onsets — the speech onsets.  Every value comes from the one
    generator `g`, in this order: per task `base`, then per recording the drift's (C, 1) and the noise's (C, Lr); P; then whatever
    `speech_side` draws."""
    C, T, nb, F, S = segment_dims(args)
    g = torch.Generator().manual_seed(seed)
    per_task = (n_segments + n_tasks - 1) // n_tasks
    hop = max(1, T // 2) if hop is None else hop
    Lr = per_task * hop + T + 64
    recordings, rec_subject, rec_task, onsets, firsts = [], [], [], [], []
    for t in range(n_tasks):
        base = torch.randn(C, Lr, generator=g)
        for k in range(recs_per_task):
            drift = torch.linspace(0, float(k + 1), Lr)[None, :] * torch.randn(C, 1, generator=g)     # what the collate removes
            rec = (base + 0.3 * torch.randn(C, Lr, generator=g)) * (2.0 + k) + drift
            if k == 0:
                firsts.append(rec)
            recordings.append(rec.to(device))
            rec_subject.append((recs_per_task * t + k) % S)
            rec_task.append(t)
            onsets.append(np.arange(per_task, dtype=np.int64) * hop + 7 * k)
    seg_task = np.repeat(np.arange(n_tasks), per_task)[:n_segments]
    seg_in_task = np.concatenate([np.arange(per_task)] * n_tasks)[:n_segments]
    P = torch.randn(F, C, generator=g) / np.sqrt(C)
    Y = speech_side(P, firsts, onsets[::recs_per_task], seg_task, seg_in_task, g)
    feed = ResidentSegmentFeed(recordings, rec_subject, rec_task, onsets, seg_task, seg_in_task, Y, seq_len_samp=T,
                               baseline_len_samp=nb, clamp_lim=float(args.preprocs["clamp_lim"]), clamp=bool(args.preprocs["clamp"]),
                               seed=seed + 17)
    n_train = int(n_segments * float(args.split_ratio))
    perm = np.random.RandomState(seed).permutation(n_segments)
    return feed, perm[:n_train], perm[n_train:]


def synthetic_resident_dataset(args, device, *, n_segments: int, n_tasks: int = 4, seed: int = 1234,
                               recs_per_task: int = 2) -> Tuple[ResidentSegmentFeed, np.ndarray, np.ndarray]:
    """Seeded stand-in with the STRUCTURE of Gwilliams2022 (27 subjects x up to 2 sessions x 4 tasks of ~100 k samples are
    not needed to exercise the path): `n_tasks` tasks, `recs_per_task` recordings per task from different subjects (the real
    dataset has every subject hear every task: pass ceil(S / n_tasks) to see all S subjects in a batch), segments laid out
    back to back with an overlap; the speech embedding of a segment is a fixed linear read-out of the raw window of the
    task's FIRST recording plus noise, so retrieval is learnable.  Returns (feed, train indices, test indices)."""
    _, T, nb, F, _ = segment_dims(args)

    def segments(P, firsts, speech_onsets, seg_task, seg_in_task, g):
        Y = torch.empty((n_segments, F, T))
        for i, (t, j) in enumerate(zip(seg_task, seg_in_task)):
            o = int(speech_onsets[t][j])
            w = firsts[t][:, o: o + T].contiguous()
            w = (w - w[:, :nb].mean(dim=1, keepdim=True)) / (2.0 * 1.35)
            Y[i] = P @ w + 0.5 * torch.randn(F, T, generator=g)
        return Y.to(device)
    return _synthetic_gwilliams(args, device, segments, n_segments=n_segments, n_tasks=n_tasks, seed=seed, recs_per_task=recs_per_task)


def synthetic_track_dataset(args, device, *, n_segments: int, dtype, n_tasks: int = 4, seed: int = 1234, recs_per_task: int = 2,
                            hop: int = None) -> Tuple[ResidentSegmentFeed, np.ndarray, np.ndarray]:
    """synthetic_resident_dataset with the speech side the way the reference first holds it (gwilliams2022.py embeds each audio
    file once): the same recordings, onsets, tasks and split, and ONE (F, L) embedding track per task — a fixed linear read-out of
    the task's FIRST recording plus noise, so retrieval is learnable — added to a WindowBank of `dtype` (bfloat16 or float16) with
    the task's segment onsets as window starts, tasks and onsets in time order, so that candidate i is segment i.  Segments are
    `hop` samples apart (default T // 2; a word every third of a second is T // 9): neighbouring windows overlap and the track is
    stored once.  Returns (feed, train indices, test indices); the feed's Y is the bank."""
    check_track_dtype("synthetic_track_dataset", dtype)
    if hop is not None and int(hop) < 1:
        raise ValueError(f"synthetic_track_dataset: hop={int(hop)} must be at least one sample")
    _, T, _, F, _ = segment_dims(args)

    def tracks(P, firsts, speech_onsets, seg_task, seg_in_task, g):
        bank = WindowBank(F, T, dtype=dtype, device=device)
        for t, first in enumerate(firsts):
            n_t = int((seg_task == t).sum())
            if n_t == 0:                                    # (a task without segments: no track, and no draw)
                continue
            track = P @ (first / (2.0 * 1.35)) + 0.5 * torch.randn(F, first.shape[1], generator=g)
            bank.add_track(track.to(device), speech_onsets[t][:n_t])
        return bank
    return _synthetic_gwilliams(args, device, tracks, n_segments=n_segments, n_tasks=n_tasks, seed=seed, recs_per_task=recs_per_task,
                                hop=None if hop is None else int(hop))


def subject_feed_geometry(length: int, srate: float, seq_len_sec: float, baseline_len_sec: float, shift_ms: float = 150,
                          segment_len: int = None) -> dict:
    """The integer arithmetic of brennan2018.py:72-104 and :296 for a recording of `length` samples at `srate` Hz:
    shift (samples dropped from the front of X and the end of Y), seq_len_samp, baseline_len_samp, trim_len (the shifted length
    cut to a multiple of seq_len_samp), reference_segment_len (what the reference's `split(num_segments)` really cuts:
    trim_len // seq_len_samp samples per chunk), segment_len (the one used: `segment_len` or seq_len_samp) and n_segments."""
    shift = int(srate * (shift_ms / 1000))
    seq = int(seq_len_sec * srate)
    nb = int(seq * baseline_len_sec / seq_len_sec)
    if seq < 1:
        raise ValueError("seq_len_sec * srate is below one sample")
    shifted = int(length) - shift
    trim = (shifted // seq) * seq
    if shift < 0 or trim < seq:
        raise ValueError(f"a recording of {length} samples holds no segment of {seq} after a shift of {shift}")
    seg = seq if segment_len is None else int(segment_len)
    if seg < 1 or trim % seg:
        raise ValueError(f"segment_len={seg} does not divide the trimmed length {trim}")
    if nb > seg:
        raise ValueError(f"baseline of {nb} samples is longer than a segment of {seg}")
    return {"shift": shift, "seq_len_samp": seq, "baseline_len_samp": nb, "trim_len": trim, "reference_segment_len": trim // seq,
            "segment_len": seg, "n_segments": trim // seg}


class ResidentSubjectFeed(_ResidentEmbeddings):
    """Brennan2018's input path on the device (brennan2018.py:72-152).  X (S, C, L): every subject's recording of the SAME
    stimulus, Y (F, L): the speech embeddings of that stimulus, both on the device — the contents of the reference's
    `processed_X.pt` ("X", with "srate") and `embd_wav2vec.pt`.  Construction, on the feed's own copy of X:
      shift X forward by shift_ms (X[..., shift:], Y[:, :-shift]); trim to a multiple of seq_len_samp = int(seq_len_sec * srate);
      RobustScaler over the whole recording — per (subject, channel), or per channel with all subjects pooled when
      `subject_wise` is False — and clamp to +-clamp_lim (collate.robust_stats + scale_clamp_rows, in place);
      cut into segments; baseline correction (mean of the first baseline_len_samp samples) per segment at batch time.
    Segments of X are not materialised: segment i of subject s is columns [i * seg, (i + 1) * seg) of the scaled recording.

    segment_len: the default, seq_len_samp, is the documented intent (T = 360 at 120 Hz, 3 s).  The reference calls
    `split(num_segments)` and therefore really cuts chunks of trim_len // seq_len_samp samples (and seq_len_samp of them,
    up to a remainder): pass segment_len=subject_feed_geometry(...)["reference_segment_len"] to reproduce its files' chunks.
    A segment_len that does not divide the trimmed length raises ValueError.

    batch(idx) -> (X (B, C, seg) fp32, Y (B, F, seg), subject_idxs int32); the chunk ids are idx itself."""

    def __init__(self, X: torch.Tensor, Y: torch.Tensor, *, srate: float, seq_len_sec: float, baseline_len_sec: float,
                 clamp_lim: float, clamp: bool = True, subject_wise: bool = True, shift_ms: float = 150, segment_len: int = None,
                 seed: int = 0):
        if X.dim() != 3 or Y.dim() != 2 or X.shape[-1] != Y.shape[-1]:
            raise ValueError("X (S, C, L) and Y (F, L) of the same length")
        geo = subject_feed_geometry(X.shape[-1], srate, seq_len_sec, baseline_len_sec, shift_ms, segment_len)
        self.geometry = geo
        shift, trim, seg = geo["shift"], geo["trim_len"], geo["segment_len"]
        self.S, self.C = int(X.shape[0]), int(X.shape[1])
        self.seg, self.nb, self.subject_wise = seg, geo["baseline_len_samp"], bool(subject_wise)
        # the feed's own contiguous copy of the shifted, trimmed recording: scaled in place, the caller's X is left alone
        Xs = X[..., shift: shift + trim].float().contiguous()
        if Xs.data_ptr() == X.data_ptr():
            Xs = Xs.clone()
        self.centre, self.scale = _collate.robust_stats(Xs, pooled=not self.subject_wise)
        self.X = _collate.scale_clamp_rows(Xs, self.centre, self.scale, float(clamp_lim), bool(clamp), pooled=not self.subject_wise,
                                           out=Xs)
        n = geo["n_segments"]
        F = int(Y.shape[0])
        # (Y[:, :-shift] then [:trim_len]: the first trim_len samples; Y's segments ARE materialised, one embedding per item)
        self.Y = Y[:, :trim].reshape(F, n, seg).permute(1, 0, 2).contiguous()
        self.rng = np.random.RandomState(seed)       # (the global generator stays reserved for SpatialDropout, see above)

    def __len__(self) -> int:
        return int(self.geometry["n_segments"])

    def draw_subjects(self, n: int) -> np.ndarray:
        """brennan2018.py:148 draws `np.random.choice(num_subjects)` item by item; one vectorised randint(0, S, size=n) from the
        feed's own generator is the same stream of values."""
        return self.rng.randint(0, self.S, size=int(n)).astype(np.int64)

    drawn_as = "subjects"

    def draw_for(self, ii: np.ndarray) -> np.ndarray:
        return self.draw_subjects(len(ii))

    def batch(self, idx, subjects=None) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor]:
        """idx: this rank's segment indices (duplicates allowed); subjects: their subjects when the caller drew them (data
        parallelism: drawn for the GLOBAL batch on every rank alike and sliced, see batches())."""
        ii = np.asarray(torch.as_tensor(idx, dtype=torch.int64).numpy(), dtype=np.int64).reshape(-1)
        if len(ii) and (ii.min() < 0 or ii.max() >= len(self)):
            raise IndexError("segment index outside the feed")
        sub = self.draw_subjects(len(ii)) if subjects is None else np.asarray(subjects, dtype=np.int64).reshape(-1)
        X = _collate.gather_baseline_windows(self.X, sub, ii * self.seg, self.seg, self.nb)
        return X, self._gather_Y(ii), torch.from_numpy(sub.astype(np.int32))


def synthetic_subject_dataset(args, device, *, length: int, seed: int = 1234) -> Tuple[torch.Tensor, torch.Tensor]:
    """Seeded stand-in with the STRUCTURE of Brennan2018: S subjects hear one stimulus; a shared latent brain response
    (C, length) reaches subject s with a per-(subject, channel) gain spread over two decades, an offset and noise — what the
    whole-recording scaling removes (and what makes subject_wise matter) — plus rare artefact spikes for the clamp.  The
    speech embedding at sample t is a fixed linear read-out of the latent response `shift_len` ms LATER plus noise, so
    retrieval is learnable after the feed's shift.  Returns (X (S, C, length), Y (F, length)) on `device`."""
    C, _, _, F, S = segment_dims(args)
    shift = int(args.preprocs["brain_resample_rate"] * (args.preprocs.get("shift_len", 150) / 1000))
    g = torch.Generator().manual_seed(seed)
    latent = torch.randn(C, length, generator=g)
    gain = 10.0 ** (2.0 * torch.rand(S, C, 1, generator=g) - 1.0)
    offset = 3.0 * torch.randn(S, C, 1, generator=g)
    X = (latent[None] + 0.3 * torch.randn(S, C, length, generator=g)) * gain + offset * gain
    spikes = torch.rand(S, C, length, generator=g) < 1e-3
    X = torch.where(spikes, X * 60.0, X)
    P = torch.randn(F, C, generator=g) / np.sqrt(C)
    Y = torch.zeros(F, length)
    Y[:, : length - shift] = (P @ latent)[:, shift:] / 1.35
    Y = Y + 0.5 * torch.randn(F, length, generator=g)
    return X.to(device), Y.to(device)
