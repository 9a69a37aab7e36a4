"""Brennan2018's input path, host side (no GPU): the NumPy restatement of the pipeline against the fixture the reference's own
functions produced (tests/golden/brennan.npz, made by tests/golden/make_brennan_golden.py), the segmentation arithmetic, the
subject draws of ResidentSubjectFeed and its refusal to run on CPU tensors.  The kernels are tested in
tests/test_subject_feed_gpu.py against the restatement pinned here."""
import numpy as np
import pytest
import torch

from tests import golden_io as G
from tests import subject_pipeline as P

CASES = {"sw": None, "pool": "reference"}        # case -> segment_len (None: the default; "reference": the fixture's chunk length)


def load_case(tag):
    g = G.load("brennan.npz")
    c = {k.split("/", 1)[1]: v for k, v in g.items() if k.startswith(tag + "/")}
    c["kw"] = dict(srate=float(c["srate"]), seq_len_sec=float(c["seq_len_sec"]), baseline_len_sec=float(c["baseline_len_sec"]),
                   clamp_lim=float(c["clamp_lim"]), subject_wise=bool(c["subject_wise"]))
    if CASES[tag] == "reference":
        c["kw"]["segment_len"] = int(c["lengths"][5])
    return c


@pytest.mark.parametrize("tag", list(CASES))
def test_restatement_reproduces_the_reference_fixture(tag):
    c = load_case(tag)
    segX, segY = P.pipeline(c["X"], c["Y"], clamp=True, **c["kw"])
    assert segX.shape == c["expX"].shape and segY.shape == c["expY"].shape
    np.testing.assert_allclose(segX, c["expX"], rtol=1e-5, atol=1e-5)
    assert np.array_equal(segY, c["expY"])
    # the fixture exercises what it is meant to: a constant row (scale 1 -> zeros), and the clamp under pooling
    assert float(np.abs(c["expX"][:, 1, 2]).max()) == 0.0
    if tag == "pool":
        Xs = c["X"][..., 1:265]
        ce, sc = P.robust_stats(Xs, False)
        assert float(np.abs(P.scale_clamp(Xs, ce, sc, 20.0, False)).max()) > 20.0


def test_fixture_cases_cover_both_segmentations():
    sw, pool = load_case("sw")["lengths"], load_case("pool")["lengths"]
    assert sw[5] == sw[1] and sw[4] == sw[1]           # trim_len // seq_len_samp == seq_len_samp: the default segmentation
    assert pool[5] != pool[1] and pool[5] == pool[4]   # the reference's chunks are num_segments samples long


@pytest.mark.parametrize("tag", list(CASES))
def test_segmentation_arithmetic_matches_the_fixture_lengths(tag):
    from speech_decoding_amd.data import subject_feed_geometry
    c = load_case(tag)
    shift, seq, nb, trim, nseg, chunk_len, chunks = [int(v) for v in c["lengths"]]
    L = c["X"].shape[-1]
    assert P.geometry(L, c["kw"]["srate"], c["kw"]["seq_len_sec"], c["kw"]["baseline_len_sec"]) == (shift, seq, nb, trim, nseg)
    geo = subject_feed_geometry(L, c["kw"]["srate"], c["kw"]["seq_len_sec"], c["kw"]["baseline_len_sec"])
    assert (geo["shift"], geo["seq_len_samp"], geo["baseline_len_samp"], geo["trim_len"]) == (shift, seq, nb, trim)
    assert geo["reference_segment_len"] == chunk_len and geo["segment_len"] == seq and geo["n_segments"] == trim // seq
    geo = subject_feed_geometry(L, c["kw"]["srate"], c["kw"]["seq_len_sec"], c["kw"]["baseline_len_sec"], segment_len=chunk_len)
    assert geo["segment_len"] == chunk_len and geo["n_segments"] == chunks


def test_segmentation_arithmetic_at_the_dataset_shapes():
    from speech_decoding_amd.data import subject_feed_geometry
    # (length, srate) -> shift, seq, baseline, trim: 120 Hz and 3 s give T = 360 and a shift of 18 samples; a fractional rate
    # (the reference resamples EEG to the embedding count: ~135.3 Hz) truncates every product separately
    for L, srate, want in [(86809, 120, (18, 360, 60, 86760)), (99712, 135.3, (20, 405, 67, 99630)), (361, 120, None), (378, 120, (18, 360, 60, 360))]:
        if want is None:
            with pytest.raises(ValueError):
                subject_feed_geometry(L, srate, 3, 0.5)
            continue
        geo = subject_feed_geometry(L, srate, 3, 0.5)
        assert (geo["shift"], geo["seq_len_samp"], geo["baseline_len_samp"], geo["trim_len"]) == want
        assert geo["n_segments"] == want[3] // want[1] == geo["reference_segment_len"]


def test_a_segment_len_that_does_not_divide_the_trimmed_length_raises():
    from speech_decoding_amd.data import ResidentSubjectFeed, subject_feed_geometry
    with pytest.raises(ValueError):
        subject_feed_geometry(330, 9, 2, 0.5, segment_len=17)
    with pytest.raises(ValueError):
        subject_feed_geometry(330, 9, 2, 0.5, segment_len=0)
    with pytest.raises(ValueError):          # raised before any kernel is asked for: CPU tensors get this far
        ResidentSubjectFeed(torch.zeros(3, 4, 330), torch.zeros(5, 330), srate=9, seq_len_sec=2, baseline_len_sec=0.5, clamp_lim=20,
                            segment_len=17)
    with pytest.raises(ValueError):
        ResidentSubjectFeed(torch.zeros(3, 4, 330), torch.zeros(5, 329), srate=9, seq_len_sec=2, baseline_len_sec=0.5, clamp_lim=20)


def test_cpu_tensors_raise_sda_error():
    from speech_decoding_amd import ResidentSubjectFeed, SdaError, collate
    X = torch.randn(3, 4, 330)
    with pytest.raises(SdaError):
        collate.robust_stats(X)
    with pytest.raises(SdaError):
        collate.robust_stats(X, pooled=True)
    with pytest.raises(SdaError):
        collate.scale_clamp_rows(X, torch.zeros(3, 4), torch.ones(3, 4), 20.0)
    with pytest.raises(SdaError):
        collate.gather_baseline_windows(X, [0], [0], 18, 4)
    with pytest.raises(SdaError):
        ResidentSubjectFeed(X, torch.randn(5, 330), srate=9, seq_len_sec=2, baseline_len_sec=0.5, clamp_lim=20)


def test_entry_points_are_declared_and_bound():
    from speech_decoding_amd import lib
    for name in ("sda_robust_stats", "sda_robust_stats_scratch_bytes", "sda_scale_clamp_rows", "sda_gather_baseline_windows"):
        assert name in lib.SIGNATURES
    assert lib.ABI_VERSION == 4


def host_feed(monkeypatch, X, Y, **kw):
    """ResidentSubjectFeed with the three kernels replaced by the NumPy restatement (host logic only)."""
    from speech_decoding_amd import collate
    from speech_decoding_amd.data import ResidentSubjectFeed

    def stats(Xt, pooled=False):
        c, s = P.robust_stats(Xt.numpy(), not pooled)
        return torch.from_numpy(c), torch.from_numpy(s)

    def scale(Xt, centre, sc, lim, clamp=True, pooled=False, out=None):
        res = torch.from_numpy(P.scale_clamp(Xt.numpy(), centre.numpy(), sc.numpy(), lim, clamp))
        return res if out is None else out.copy_(res)

    def gather(Xt, subjects, starts, T, nb):
        return torch.from_numpy(P.baseline_windows(Xt.numpy(), subjects, starts, T, nb))

    monkeypatch.setattr(collate, "robust_stats", stats)
    monkeypatch.setattr(collate, "scale_clamp_rows", scale)
    monkeypatch.setattr(collate, "gather_baseline_windows", gather)
    return ResidentSubjectFeed(torch.as_tensor(X), torch.as_tensor(Y), **kw)


@pytest.mark.parametrize("tag", list(CASES))
def test_feed_host_logic_reproduces_the_fixture(tag, monkeypatch):
    """Shift, trim, segmentation and the Y layout of the feed itself, with the kernels stood in by the restatement."""
    c = load_case(tag)
    X0 = c["X"].copy()
    feed = host_feed(monkeypatch, c["X"], c["Y"], seed=3, **c["kw"])
    assert np.array_equal(c["X"], X0)                                  # the caller's recording is left alone
    n, S = c["expX"].shape[:2]
    assert len(feed) == n and feed.S == S
    idx = np.array([0, n - 1, 2, 2, 1])
    sub = np.array([0, 2, 1, 1, 0])
    Xb, Yb, sb = feed.batch(idx, subjects=sub)
    np.testing.assert_allclose(Xb.numpy(), c["expX"][idx, sub], rtol=1e-5, atol=1e-5)
    assert np.array_equal(Yb.numpy(), c["expY"][idx]) and sb.dtype == torch.int32 and sb.tolist() == sub.tolist()
    with pytest.raises(IndexError):
        feed.batch([n])


def test_vectorised_subject_draw_is_the_item_by_item_choice_stream(monkeypatch):
    """brennan2018.py:148: `np.random.choice(num_subjects)` per item; the feed draws a whole batch at once from its own
    RandomState — the same values in the same order, batch after batch."""
    c = load_case("sw")
    feed = host_feed(monkeypatch, c["X"], c["Y"], seed=11, **c["kw"])
    twin = np.random.RandomState(11)
    state = np.random.get_state()[1].copy()
    for n in (1, 7, 64):
        want = [int(twin.choice(feed.S)) for _ in range(n)]
        assert feed.draw_subjects(n).tolist() == want
    _, _, sub = feed.batch(np.arange(5))
    assert sub.tolist() == [int(twin.choice(feed.S)) for _ in range(5)]
    assert np.array_equal(np.random.get_state()[1], state)             # NumPy's global generator is not touched


def test_rank_sliced_draws_union_to_the_single_process_batch(monkeypatch):
    from speech_decoding_amd.data import ShardedRandomSampler
    c = load_case("sw")
    n = len(c["expX"])
    index_map = np.random.RandomState(0).permutation(n)[:12]

    def run(rank, world):
        feed = host_feed(monkeypatch, c["X"], c["Y"], seed=9, **c["kw"])
        calls = []
        real = feed.batch
        feed.batch = lambda idx, subjects=None: calls.append((np.asarray(idx).copy(), None if subjects is None else np.asarray(subjects).copy())) or real(idx, subjects)
        out = list(feed.batches(ShardedRandomSampler(len(index_map), 8, 4, rank=rank, world=world, seed=3), index_map=index_map))
        return calls, out
    single_calls, single = run(0, 1)
    parts = [run(r, 2) for r in range(2)]
    twin = np.random.RandomState(9)
    for b in range(4):
        idx = np.concatenate([parts[r][0][b][0] for r in range(2)])
        sub = np.concatenate([parts[r][1][b][2].numpy() for r in range(2)])
        assert idx.tolist() == single_calls[b][0].tolist() and set(idx.tolist()) <= set(index_map.tolist())
        assert sub.tolist() == single[b][2].tolist() == twin.randint(0, 3, size=8).tolist()
        X = torch.cat([parts[r][1][b][0] for r in range(2)])
        assert torch.equal(X, single[b][0])
        assert all(len(parts[r][0][b][0]) == 4 for r in range(2))
