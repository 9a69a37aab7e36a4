"""Brennan2018's input path on the device: sda_robust_stats (exact order statistics of long rows), sda_scale_clamp_rows,
sda_gather_baseline_windows, ResidentSubjectFeed and train.py's data=continuous — against np.percentile, the NumPy restatement
of the pipeline (tests/subject_pipeline.py, pinned on the reference's fixture by tests/test_subject_feed_cpu.py) and the
fixture itself (tests/golden/brennan.npz)."""
import numpy as np
import pytest
import torch

from tests import golden_io as G
from tests import subject_pipeline as P
from tests.test_subject_feed_cpu import CASES, load_case

pytestmark = pytest.mark.gpu

DEV = "cuda:0"


def gpu_stats(rows: np.ndarray):
    """rows (R, N) float32 -> (centre, scale) numpy, one row per (subject 0, channel r)."""
    from speech_decoding_amd.collate import robust_stats
    c, s = robust_stats(torch.from_numpy(np.ascontiguousarray(rows, dtype=np.float32))[None].to(DEV))
    return c[0].cpu().numpy(), s[0].cpu().numpy()


def percentile32(rows: np.ndarray):
    """np.percentile on the float32 rows themselves: at integer positions the results are elements of the row, whatever the
    float type numpy computes in; their float32 difference is the correctly rounded one."""
    q = np.percentile(rows.astype(np.float32), [25, 50, 75], axis=1)
    assert np.array_equal(q.astype(np.float32), q)
    q = q.astype(np.float32)
    scale = (q[2] - q[0]).astype(np.float32)
    return q[1], np.where(scale == 0, np.float32(1), scale)


def integer_rows(N, seed, R=3):
    """Distinct integers of both signs stored as floats, shuffled, a different offset per row."""
    rng = np.random.RandomState(seed)
    return np.stack([rng.permutation(N).astype(np.float32) * 3 - np.float32(N + 7 * r) for r in range(R)])


# rows of 4k + 1 samples: the three positions q * (N - 1) are integers, the statistics are elements of the row (and one exact
# difference): equal to np.percentile on the float32 row, bit for bit (as numbers: a zero's sign is not compared).
# 5, 37, 257: inside one workgroup's share (4096 samples); 4097: two workgroups; 70001: a row cut over many workgroups
@pytest.mark.parametrize("N", [5, 37, 257, 4097, 70001])
def test_robust_stats_is_exact_at_integer_positions(N):
    rows = integer_rows(N, seed=N)
    centre, scale = gpu_stats(rows)
    wc, ws = percentile32(rows)
    assert np.array_equal(centre, wc) and np.array_equal(scale, ws), (centre, wc, scale, ws)


def graded_row(N, rng, zeros=False):
    """Both signs, magnitudes on a geometric grid: neighbours in the sorted row differ by at least 1e-3 relative, so a rank
    that is off by one misses by orders of magnitude more than the tolerance."""
    half = N // 2
    mags = 1e-3 * 1.0015 ** np.arange(max(half, N - half), dtype=np.float64)
    v = np.concatenate([-mags[:half], mags[:N - half]]).astype(np.float32)
    if zeros and N >= 6:
        v[0], v[half] = -0.0, 0.0                    # the two smallest magnitudes become -0.0 and +0.0
    return rng.permutation(v)


def interpolated_bounds(row):
    """float64 np.percentile of the float32 row, and the tolerance: 4 fp32 ulp of the larger bracketing element's magnitude
    (one lerp and one subtraction)."""
    s = np.sort(row.astype(np.float64))
    n = len(s)
    q = np.percentile(row.astype(np.float64), [25, 50, 75])

    def mag(p):
        i0 = int(np.floor(p * (n - 1)))
        return max(abs(s[i0]), abs(s[min(i0 + 1, n - 1)]))
    ulp = lambda m: float(np.spacing(np.float32(m)))      # noqa: E731
    return q[1], 4 * ulp(mag(0.5)), q[2] - q[0], 4 * ulp(max(mag(0.25), mag(0.75)))


@pytest.mark.parametrize("N", [2, 6, 100, 4099, 65536])
def test_robust_stats_interpolates_like_numpy(N):
    rng = np.random.RandomState(N)
    rows = np.stack([graded_row(N, rng), graded_row(N, rng, zeros=True), (graded_row(N, rng) * np.float32(37.0)).astype(np.float32)])
    centre, scale = gpu_stats(rows)
    for r, row in enumerate(rows):
        wc, tc, ws, ts = interpolated_bounds(row)
        print(f"N={N} row {r}: centre {centre[r]!r} vs {wc!r} (tol {tc:.3e}), scale {scale[r]!r} vs {ws!r} (tol {ts:.3e})")
        assert abs(float(centre[r]) - wc) <= tc, (N, r, centre[r], wc, tc)
        assert abs(float(scale[r]) - ws) <= ts, (N, r, scale[r], ws, ts)


def test_robust_stats_input_patterns():
    rng = np.random.RandomState(5)
    # values that differ only in the lowest mantissa byte: decided by the last radix pass alone (253 = 4 * 63 + 1 distinct values)
    low = (np.float32(1.5).view(np.uint32) + rng.permutation(253).astype(np.uint32)).view(np.float32)
    neg = -(np.float32(3.0).view(np.uint32) + rng.permutation(253).astype(np.uint32)).view(np.float32)
    rows = np.stack([low, neg])
    centre, scale = gpu_stats(rows)
    wc, ws = percentile32(rows)
    assert np.array_equal(centre, wc) and np.array_equal(scale, ws)
    # an all-equal row: centre is the value, the zero scale becomes 1
    for N in (2, 4097):
        centre, scale = gpu_stats(np.full((2, N), -2.75, dtype=np.float32))
        assert centre.tolist() == [-2.75, -2.75] and scale.tolist() == [1.0, 1.0]
    # half the row tied at the median, distinct integers below and above
    N = 4097
    row = np.concatenate([np.arange(1024, dtype=np.float32) - 3000, np.full(2049, 7.25, dtype=np.float32), np.arange(1024, dtype=np.float32) + 100])
    rows = np.stack([rng.permutation(row), rng.permutation(row[::-1] * -1)])
    centre, scale = gpu_stats(rows)
    wc, ws = percentile32(rows)
    assert np.array_equal(centre, wc) and np.array_equal(scale, ws) and centre.tolist() == [7.25, -7.25]
    # +-inf order like any value: a few at either end move the ranks, nothing else
    row = integer_rows(N, seed=1, R=1)[0]
    row[[3, 500, 4000]] = -np.inf
    row[[7, 8, 9, 2000, 4096]] = np.inf
    centre, scale = gpu_stats(row[None])
    wc, ws = percentile32(row[None])
    assert np.isfinite(wc).all() and np.array_equal(centre, wc) and np.array_equal(scale, ws)
    # mixed signs with both zeros, exact positions
    row = np.concatenate([-np.arange(1, 18, dtype=np.float32), [-0.0, 0.0], np.arange(1, 19, dtype=np.float32)]).astype(np.float32)
    assert len(row) == 37
    centre, scale = gpu_stats(rng.permutation(row)[None])
    wc, ws = percentile32(row[None])
    assert np.array_equal(centre, wc) and np.array_equal(scale, ws)


def test_robust_stats_chunked_rows_equal_contiguous_rows_and_repeat():
    """Pooled rows (3 chunks, chunk_stride = C * L > chunk_len) against the same samples made contiguous: the same bits; two
    calls: the same bits."""
    from speech_decoding_amd.collate import robust_stats
    g = torch.Generator().manual_seed(3)
    S, C, L = 3, 2, 4099
    X = (torch.randn(S, C, L, generator=g) * torch.tensor([0.1, 1.0, 30.0])[:, None, None] + torch.randn(S, C, 1, generator=g)).to(DEV)
    pc, ps = robust_stats(X, pooled=True)
    flat = X.permute(1, 0, 2).reshape(1, C, S * L).contiguous()
    fc, fs = robust_stats(flat)
    assert pc.shape == (C,) and torch.equal(pc, fc[0]) and torch.equal(ps, fs[0])
    pc2, ps2 = robust_stats(X, pooled=True)
    assert torch.equal(pc, pc2) and torch.equal(ps, ps2)
    wc, ws = P.robust_stats(X.cpu().numpy(), False)
    np.testing.assert_allclose(pc.cpu().numpy(), wc, rtol=1e-6, atol=0)
    np.testing.assert_allclose(ps.cpu().numpy(), ws, rtol=1e-6, atol=0)
    sc, ss = robust_stats(X)
    wc, ws = P.robust_stats(X.cpu().numpy(), True)
    assert sc.shape == (S, C)
    np.testing.assert_allclose(sc.cpu().numpy(), wc, rtol=1e-6, atol=0)
    np.testing.assert_allclose(ss.cpu().numpy(), ws, rtol=1e-6, atol=0)


def offset_view(n_before, shape, fill=float("nan")):
    """A contiguous tensor of `shape` whose first element sits n_before floats behind a 16-byte aligned address, NaN around it."""
    numel = int(np.prod(shape))
    buf = torch.full((numel + 8,), fill, dtype=torch.float32, device=DEV)
    assert buf.data_ptr() % 16 == 0
    return buf, buf[n_before: n_before + numel].view(shape)


@pytest.mark.parametrize("L", [1, 7, 4099, 8197, 20000])
@pytest.mark.parametrize("pooled", [False, True])
def test_scale_clamp_rows(L, pooled):
    """Against the restatement: clamp on and off, in place and out of place, bases on and off 16-byte alignment (the same and
    different misalignment of source and destination), lengths that are no multiple of 4 and longer than one workgroup's piece."""
    from speech_decoding_amd.collate import scale_clamp_rows
    g = torch.Generator().manual_seed(L)
    S, C = 3, 4
    X = torch.randn(S, C, L, generator=g) * 40 + 3
    shape = (C,) if pooled else (S, C)
    centre = torch.randn(shape, generator=g) * 5
    scale = torch.rand(shape, generator=g) * 3 + 0.05
    for clamp in (True, False):
        want = P.scale_clamp(X.numpy(), centre.numpy(), scale.numpy(), 20.0, clamp)
        for off_in, off_out in [(0, 0), (1, 1), (3, 2), (0, None)]:
            sbuf, src = offset_view(off_in, (S, C, L))
            src.copy_(X)
            if off_out is None:                                  # in place
                dbuf, dst = sbuf, src
            else:
                dbuf, dst = offset_view(off_out, (S, C, L))
            got = scale_clamp_rows(src, centre.to(DEV), scale.to(DEV), 20.0, clamp, pooled=pooled, out=dst)
            assert got.data_ptr() == dst.data_ptr()
            np.testing.assert_allclose(got.cpu().numpy(), want, rtol=1e-5, atol=1e-5)
            o = off_in if off_out is None else off_out
            guard = torch.cat([dbuf[:o], dbuf[o + S * C * L:]])
            assert bool(torch.isnan(guard).all())                # nothing written outside the tensor
        got = scale_clamp_rows(X.to(DEV), centre.to(DEV), scale.to(DEV), 20.0, clamp, pooled=pooled)
        np.testing.assert_allclose(got.cpu().numpy(), want, rtol=1e-5, atol=1e-5)


@pytest.mark.parametrize("T", [7, 241, 360, 1500])
def test_gather_baseline_windows(T):
    """Windows starting at any sample (first, last and an odd one), duplicates in the batch, baseline lengths 0, 1 and T, T
    beyond the 1024 samples of the per-window collate; the samples just outside every window are NaN and must not be read."""
    from speech_decoding_amd.collate import gather_baseline_windows
    g = torch.Generator().manual_seed(T)
    S, C, L = 3, 5, 1707
    X = torch.randn(S, C, L, generator=g) * 4 + torch.randn(S, C, 1, generator=g) * 10
    starts_of = [0, 77, L - T]
    Xn = X.clone()
    for s, a in enumerate(starts_of):
        if a > 0:
            Xn[s, :, a - 1] = float("nan")
        if a + T < L:
            Xn[s, :, a + T] = float("nan")
    sub = [0, 1, 2, 1, 0]
    starts = [starts_of[s] for s in sub]
    Xd = Xn.to(DEV)
    for nb in (0, 1, T):
        want = P.baseline_windows(X.numpy(), sub, starts, T, nb)
        got = gather_baseline_windows(Xd, sub, starts, T, nb).cpu().numpy()
        assert got.shape == (5, C, T) and np.isfinite(got).all()
        np.testing.assert_allclose(got, want, rtol=1e-5, atol=2e-5)
        if nb == 0:
            assert np.array_equal(got, want)                     # a copy
    again = gather_baseline_windows(Xd, sub, starts, T, T).cpu().numpy()
    assert np.array_equal(again, got)
    with pytest.raises(IndexError):
        gather_baseline_windows(Xd, [0], [L - T + 1], T, 1)


def fixture_feed(tag, **extra):
    from speech_decoding_amd import ResidentSubjectFeed
    c = load_case(tag)
    feed = ResidentSubjectFeed(torch.from_numpy(c["X"]).to(DEV), torch.from_numpy(c["Y"]).to(DEV), **c["kw"], **extra)
    return c, feed


@pytest.mark.parametrize("tag", list(CASES))
def test_feed_reproduces_the_reference_fixture(tag):
    c, feed = fixture_feed(tag, seed=5)
    n, S = c["expX"].shape[:2]
    assert len(feed) == n
    idx = np.concatenate([np.repeat(np.arange(n), S), [2, 2, 0]])          # every (segment, subject) pair, then duplicates
    sub = np.concatenate([np.tile(np.arange(S), n), [1, 1, 2]])
    X, Y, sidx = feed.batch(idx, subjects=sub)
    assert X.dtype == torch.float32 and tuple(X.shape) == (len(idx),) + c["expX"].shape[2:]
    np.testing.assert_allclose(X.cpu().numpy(), c["expX"][idx, sub], rtol=1e-5, atol=2e-5)
    assert np.array_equal(Y.cpu().numpy(), c["expY"][idx]) and sidx.dtype == torch.int32 and sidx.tolist() == sub.tolist()
    # subjects drawn by the feed: its own RandomState, replayed
    twin = np.random.RandomState(5)
    X2, _, s2 = feed.batch(idx[:7])
    want = [int(twin.choice(S)) for _ in range(7)]
    assert s2.tolist() == want
    np.testing.assert_allclose(X2.cpu().numpy(), c["expX"][idx[:7], want], rtol=1e-5, atol=2e-5)
    # built twice: identical bits
    _, twin_feed = fixture_feed(tag, seed=5)
    assert torch.equal(feed.X, twin_feed.X) and torch.equal(feed.centre, twin_feed.centre) and torch.equal(feed.scale, twin_feed.scale)
    assert torch.equal(twin_feed.batch(idx, subjects=sub)[0], X)


@pytest.mark.parametrize("subject_wise", [True, False])
@pytest.mark.parametrize("clamp", [True, False])
def test_feed_against_the_restatement_at_a_longer_recording(subject_wise, clamp):
    from speech_decoding_amd import ResidentSubjectFeed
    rng = np.random.RandomState(17)
    S, C, F, L = 3, 5, 4, 4099 + 15
    X = ((rng.standard_t(2, size=(S, C, L)) + rng.randn(S, C, 1)) * 10.0 ** rng.uniform(-1, 1, size=(S, C, 1))).astype(np.float32)
    Y = rng.randn(F, L).astype(np.float32)
    kw = dict(srate=100, seq_len_sec=0.5, baseline_len_sec=0.1, clamp_lim=20.0, clamp=clamp, subject_wise=subject_wise)
    segX, segY = P.pipeline(X, Y, **kw)
    feed = ResidentSubjectFeed(torch.from_numpy(X).to(DEV), torch.from_numpy(Y).to(DEV), **kw)
    n = len(feed)
    assert n == len(segX) == 81 and feed.seg == 50 and feed.nb == 10
    idx = rng.randint(0, n, size=40)
    sub = rng.randint(0, S, size=40)
    Xb, Yb, _ = feed.batch(idx, subjects=sub)
    np.testing.assert_allclose(Xb.cpu().numpy(), segX[idx, sub], rtol=1e-5, atol=2e-5)
    assert np.array_equal(Yb.cpu().numpy(), segY[idx])


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float32])
def test_feed_with_packed_embeddings_hands_out_the_loss_operand(dtype):
    from speech_decoding_amd import ops
    _, plain = fixture_feed("sw", seed=2)
    _, feed = fixture_feed("sw", seed=2)
    assert feed.pack_embeddings(dtype) is feed
    idx = np.array([3, 17, 17, 0, 5, 9])
    X, Y, sub = feed.batch(idx)
    X0, Y0, sub0 = plain.batch(idx)
    assert torch.equal(X, X0) and torch.equal(sub, sub0) and Y.dtype == dtype and tuple(Y.shape) == tuple(Y0.shape)
    assert torch.equal(Y.float().cpu(), Y0.to(dtype).float().cpu())
    B, F, T = Y.shape
    assert ops.rows_base(Y, B, F, T, dtype) is not None              # a row-layout view: CLIPLoss consumes it in place


def tiny_args(**over):
    from oracle import brain_oracle as O
    from speech_decoding_amd import load_config
    loc = O.synthetic_positions(12, seed=7)
    args = load_config(overrides=["dataset=Brennan2018", "data=continuous", "num_subjects=3", "D1=16", "D2=24", "F=32", "K=4", "batch_size=12",
                                  "epochs=10", "num_channels=12", "preprocs.last4layers=False", "preprocs.seq_len_sec=1",
                                  "preprocs.brain_resample_rate=40", "preprocs.baseline_len_sec=0.25", "lr=3e-3",
                                  "synthetic_segments=40", "updates_per_epoch=2", "split_ratio=0.7"] + [f"{k}={v}" for k, v in over.items()])
    args["sensor_positions"] = loc.numpy()
    return args


def recording_feeds(monkeypatch):
    """train.py builds its feed inside run(): keep a handle on it."""
    from speech_decoding_amd import data as D
    made = []

    class Recorded(D.ResidentSubjectFeed):
        def __init__(self, *a, **k):
            super().__init__(*a, **k)
            made.append(self)
    monkeypatch.setattr(D, "ResidentSubjectFeed", Recorded)
    return made


def test_training_driver_on_the_continuous_feed(tmp_path, monkeypatch):
    """train.py dataset=Brennan2018 data=continuous: whole-recording scaling -> segment gather -> the training step, at the
    once-per-epoch update cadence of this dataset; the loss comes down and the held-out split is ranked."""
    import train as T
    monkeypatch.chdir(tmp_path)
    made = recording_feeds(monkeypatch)
    args = tiny_args()
    torch.manual_seed(0)
    np.random.seed(0)
    hist, enc, lossf = T.run(args, log=lambda *a: None)
    print([round(float(h["train_loss"]), 4) for h in hist], [round(float(h["test_loss"]), 4) for h in hist])
    assert len(hist) == 10 and all(np.isfinite(h["train_loss"]) and np.isfinite(h["test_loss"]) for h in hist)
    assert hist[-1]["train_loss"] < hist[0]["train_loss"]
    assert 0.0 <= hist[-1]["testTop10acc"] <= 1.0
    feed, = made
    assert feed.subject_wise and len(feed) == 40 and feed.seg == 40 and feed.nb == 10 and feed.geometry["shift"] == 6
    assert tuple(feed.X.shape) == (3, 12, 1600) and feed._Yt is not None
    with pytest.raises(ValueError):
        T.run(tiny_args(dataset="Gwilliams2022"), log=lambda *a: None)


def test_training_driver_reads_subject_wise(tmp_path, monkeypatch):
    """preprocs.subject_wise=False reaches the feed: on the stand-in (per-subject gains over two decades) pooling every
    subject per channel gives a different scaled recording than scaling each subject on its own."""
    import train as T
    from speech_decoding_amd.data import ResidentSubjectFeed, synthetic_subject_dataset
    monkeypatch.chdir(tmp_path)
    made = recording_feeds(monkeypatch)
    args = tiny_args(**{"preprocs.subject_wise": False, "epochs": 2})
    torch.manual_seed(0)
    np.random.seed(0)
    hist, _, _ = T.run(args, log=lambda *a: None)
    assert len(hist) == 2 and all(np.isfinite(h["train_loss"]) and np.isfinite(h["test_loss"]) for h in hist)
    pooled, = made
    assert not pooled.subject_wise and tuple(pooled.centre.shape) == (12,)
    Xc, Yc = synthetic_subject_dataset(args, DEV, length=40 * 40 + 6 + 13, seed=1234)
    own = ResidentSubjectFeed(Xc, Yc, srate=40, seq_len_sec=1, baseline_len_sec=0.25, clamp_lim=20.0, subject_wise=True)
    assert tuple(own.centre.shape) == (3, 12) and own.X.shape == pooled.X.shape
    assert float((own.X - pooled.X).abs().max()) > 1.0
    # per subject every row has unit inter-quartile range; pooled, the subjects keep their relative gains
    iqr = lambda X: (torch.quantile(X, 0.75, dim=-1) - torch.quantile(X, 0.25, dim=-1)).cpu()      # noqa: E731
    assert float((iqr(own.X) - 1).abs().max()) < 1e-3
    assert float(iqr(pooled.X).max() / iqr(pooled.X).min()) > 3.0
