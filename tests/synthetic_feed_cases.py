"""The seeded stand-in datasets of speech_decoding_amd.data run on the CPU, for tests/test_synthetic_feeds_cpu.py and
tests/golden/make_synthetic_feeds_golden.py: the device kernel behind ResidentSegmentFeed and the WindowBank are replaced by
recorders (host logic only), and one case's builder is run into a flat dict of arrays — what tests/golden/synthetic_feeds.npz holds.

Every value of these datasets comes from one seeded generator whose order of draws decides all of them; bench.py's feed leg and the
train.py tests depend on the values."""
import numpy as np
import torch

from tests.builders import Config


C, F, S, RATE = 6, 5, 3, 8                      # T = 8 samples, 2 of them baseline; default hop 4
SEED = 1234


def args(dataset="Gwilliams2022"):
    return Config(dataset=dataset, num_channels=C, F=F, num_subjects=S, split_ratio=0.7,
                preprocs=dict(brain_resample_rate=RATE, seq_len_sec=1, baseline_len_sec=0.25, last4layers=False, clamp_lim=20.0,
                              clamp=True, shift_len=150))


# name -> (builder, keywords)
CASES = {
    "resident_short_last_task": ("synthetic_resident_dataset", dict(n_segments=10, n_tasks=3)),      # 4 + 4 + 2 segments
    "resident_three_recordings": ("synthetic_resident_dataset", dict(n_segments=10, n_tasks=3, recs_per_task=3)),
    "tracks_default_hop": ("synthetic_track_dataset", dict(n_segments=10, n_tasks=3, dtype=torch.bfloat16)),
    "tracks_hop_3": ("synthetic_track_dataset", dict(n_segments=10, n_tasks=3, dtype=torch.bfloat16, hop=3)),
    "tracks_empty_task": ("synthetic_track_dataset", dict(n_segments=3, n_tasks=4, dtype=torch.float16)),   # task 3: no segment, no track
    "subject": ("synthetic_subject_dataset", dict(length=8 * 8 + 1 + 2)),
}
# compared with the case's stored tolerance (a matrix product or a mean lies behind each element); everything else exactly
TOLERANT = ("Y", "tracks")


class FakeSegments:
    """collate.ResidentSegments: keeps the recordings and what it was constructed with."""

    def __init__(self, sessions, *a, **k):
        self.sessions, self.ctor = sessions, (a, k)


class FakeBank:
    """retrieval.WindowBank: keeps the tracks and the window starts handed to add_track."""

    def __init__(self, F, T, dtype=torch.bfloat16, device=None):
        self.F, self.T, self.dtype, self.tracks, self.track_starts = F, T, dtype, [], []

    def add_track(self, track, starts):
        self.tracks.append(track)
        self.track_starts.append(np.asarray(starts, dtype=np.int64).copy())

    def __len__(self):
        return sum(len(s) for s in self.track_starts)


def patch_recorders(setattr_):
    """setattr_: monkeypatch.setattr.  Each name is replaced where data.py looks it up."""
    from speech_decoding_amd import data as D
    setattr_(D, "ResidentSegments", FakeSegments)
    setattr_(D, "WindowBank", FakeBank)


def run_case(name):
    """The arrays of one case (patch_recorders first)."""
    from speech_decoding_amd import data as D
    builder, kw = CASES[name]
    if name == "subject":
        X, Y = getattr(D, builder)(args("Brennan2018"), "cpu", seed=SEED, **kw)
        return {"X": X.numpy(), "Y": Y.numpy()}
    feed, train_idx, test_idx = getattr(D, builder)(args(), "cpu", seed=SEED, **kw)
    (seq, nb, lim, clamp), rest = feed.rs.ctor
    assert not rest
    out = {"recordings": torch.stack(feed.rs.sessions).numpy(), "rec_subject": feed.rec_subject, "rec_task": feed.rec_task,
           "onsets": np.stack(feed.onsets), "seg_task": feed.seg_task, "seg_in_task": feed.seg_in_task,
           "train_idx": train_idx, "test_idx": test_idx, "segments_ctor": np.array([seq, nb, lim, clamp], dtype=np.float64),
           "rng": feed.rng.randint(0, 1000, 8)}
    if isinstance(feed.Y, FakeBank):
        out["tracks"] = torch.stack(feed.Y.tracks).numpy()
        out["starts"] = np.concatenate(feed.Y.track_starts)
        out["starts_per_track"] = np.array([len(s) for s in feed.Y.track_starts])
        out["bank_ctor"] = np.array([feed.Y.F, feed.Y.T, {torch.bfloat16: 16, torch.float16: 15}[feed.Y.dtype]])
    else:
        out["Y"] = feed.Y.numpy()
    return out
