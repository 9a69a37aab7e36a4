"""Training batches gathered from resident speech tracks on the MI355X: sda_gather_windows / ops.gather_windows, WindowBank.select,
ResidentSegmentFeed with a WindowBank as Y, train.py data=tracks.

Yardsticks.  The kernel moves bytes, so everything about it is exact: the numpy restatement of tests/track_feed_cases.py (whose
planted bugs tests/test_track_feed_cpu.py tells apart) over the WHOLE destination buffer, pad rows and slack included, into a
destination pre-filled with a NaN pattern.  The feed is compared bit for bit with the existing feed given the same windows
materialised on the host from the bank's rounded table and packed with pack_embeddings; the loss and its gradients on the two
feeds' Y are compared bit for bit as well (same bytes in, same kernels, same order)."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from oracle import brain_oracle as O          # noqa: E402  (sensor positions of the toy encoder, as tests/test_train_gpu.py)
from tests import track_feed_cases as K       # noqa: E402

DEV = "cuda:0"
DT = {"bf16": torch.bfloat16, "fp16": torch.float16}
INT = {np.dtype(np.uint16): (np.int16, torch.int16), np.dtype(np.uint32): (np.int32, torch.int32)}

_refs = {}


def ref(name, utype):
    """(case, restated destination), computed once and shared (never written to)."""
    key = (name, np.dtype(utype))
    if key not in _refs:
        c = K.case(name, utype)
        _refs[key] = (c, K.gather_windows_ref(c["table"], c["starts"], c["idx"], c["T"]))
    return _refs[key]


def to_dev(u, dtype=None):
    """An unsigned-integer array as a device tensor of the same bits: int16 / int32, or viewed as `dtype`."""
    t = torch.from_numpy(np.ascontiguousarray(u).view(INT[u.dtype][0])).to(DEV)
    return t if dtype is None else t.view(dtype)


def bits(t, utype):
    return t.contiguous().view(INT[np.dtype(utype)][1]).cpu().numpy().view(utype)


def check_zero_regions(got, c):
    B, T, F, Tp = c["B"], c["T"], c["F"], c["T"] + 16
    for b in range(B):
        assert not got[b * Tp: b * Tp + 16].any(), f"pad rows of sample {b}"
    assert got.shape[0] == B * Tp + 176 and not got[B * Tp:].any(), "slack"
    assert not got[:, F:].any(), "channel padding"


@pytest.mark.parametrize("dtype", ["bf16", "fp16"])
@pytest.mark.parametrize("name", K.CASES)
def test_ops_gather_windows_is_the_restatement(name, dtype):
    from speech_decoding_amd import lib as L, ops
    c, want = ref(name, np.uint16)
    table = to_dev(c["table"], DT[dtype])
    out = ops.gather_windows(table, torch.from_numpy(c["starts"]).to(DEV), torch.from_numpy(c["idx"]).to(DEV), c["B"], c["T"])
    assert out.dtype == DT[dtype] and tuple(out.shape) == (L.rows_alloc(c["B"], c["T"]), c["Cp"]) == want.shape
    assert torch.equal(out.view(torch.int16), to_dev(want))
    check_zero_regions(bits(out, np.uint16), c)


def call_c_entry(c, utype, idx=None, starts=None, table_rows=None):
    """sda_gather_windows called directly into a destination full of NaN patterns; returns (rc, destination bits)."""
    from speech_decoding_amd import lib as L
    table = to_dev(c["table"])
    idx = torch.from_numpy(c["idx"] if idx is None else idx).to(DEV)
    starts = torch.from_numpy(c["starts"] if starts is None else starts).to(DEV)
    B, T, Cp = len(idx), c["T"], c["Cp"]
    dst = torch.full((L.rows_alloc(B, T), Cp), K.FILL[np.dtype(utype)], dtype=INT[np.dtype(utype)][1], device=DEV)
    rc = L.load().sda_gather_windows(table.data_ptr(), table.shape[0] if table_rows is None else table_rows, starts.data_ptr(),
                                     starts.numel(), idx.data_ptr(), dst.data_ptr(), B, T, Cp * table.element_size(),
                                     torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    return rc, bits(dst, utype)


@pytest.mark.parametrize("width", ["16-bit", "fp32 bytes"])
@pytest.mark.parametrize("name", K.CASES)
def test_c_entry_writes_every_byte_of_an_uninitialised_destination(name, width):
    utype = {"16-bit": np.uint16, "fp32 bytes": np.uint32}[width]
    c, want = ref(name, utype)
    rc, got = call_c_entry(c, utype)
    assert rc == 0
    assert np.array_equal(got, want)                    # every element: none keeps the NaN pattern it arrived with
    check_zero_regions(got, c)


@pytest.mark.parametrize("width", ["16-bit", "fp32 bytes"])
def test_candidates_and_starts_outside_the_table_come_back_as_zeros(width):
    """Defined behaviour, not a provoked fault: the kernel's guard means no read leaves the table."""
    utype = {"16-bit": np.uint16, "fp32 bytes": np.uint32}[width]
    c, _ = ref("a7", utype)
    M, Tp = len(c["starts"]), c["T"] + 16
    idx = c["idx"].copy()
    idx[2], idx[5] = M, -1
    rc, got = call_c_entry(c, utype, idx=idx)
    assert rc == 0 and np.array_equal(got, K.gather_windows_ref(c["table"], c["starts"], idx, c["T"]))
    want_valid = ref("a7", utype)[1]
    for b in range(7):
        rows = slice(b * Tp, (b + 1) * Tp)
        assert (not got[rows].any()) if b in (2, 5) else np.array_equal(got[rows], want_valid[rows])
    # a start in front of the table, and one whose window would leave a table declared two rows shorter than it is
    starts = c["starts"].copy()
    starts[1] = -2
    rc, got = call_c_entry(c, utype, starts=starts, table_rows=30)
    assert rc == 0 and np.array_equal(got, K.gather_windows_ref(c["table"][:30], starts, c["idx"], c["T"]))
    zeroed = [b for b in range(7) if not got[b * Tp: (b + 1) * Tp].any()]
    assert zeroed == [b for b, m in enumerate(c["idx"]) if m in (1, 4)]              # start -2; start 27: 27 + 5 > 30


# ---------------------------------------------------------------------------------------------------------------------------
# the feed
# ---------------------------------------------------------------------------------------------------------------------------
def tiny_args(**more):
    from speech_decoding_amd import load_config
    loc = O.synthetic_positions(12, seed=7)
    args = load_config(overrides=["dataset=Gwilliams2022", "num_subjects=3", "D1=16", "D2=24", "F=32", "K=4", "batch_size=12",
                                  "epochs=2", "num_channels=12", "preprocs.last4layers=False", "preprocs.seq_len_sec=1",
                                  "preprocs.brain_resample_rate=40", "preprocs.baseline_len_sec=0.25", "lr=3e-4",
                                  "synthetic_segments=40", "updates_per_epoch=2", "split_ratio=0.7"] + [f"{k}={v}" for k, v in more.items()])
    args["sensor_positions"] = loc.numpy()
    return args


def twin(feed, Y, seed=1234 + 17):
    """A feed over the same recordings, onsets and segments as `feed` with `Y` as its speech side and a fresh generator."""
    from speech_decoding_amd.data import ResidentSegmentFeed
    rs = feed.rs
    return ResidentSegmentFeed(rs.sessions, feed.rec_subject, feed.rec_task, feed.onsets, feed.seg_task, feed.seg_in_task, Y,
                               seq_len_samp=rs.T, baseline_len_samp=rs.nb, clamp_lim=rs.lim, clamp=rs.clamp, seed=seed)


def track_feed(dtype, hop=7):
    from speech_decoding_amd.data import synthetic_track_dataset
    return synthetic_track_dataset(tiny_args(), DEV, n_segments=40, dtype=DT[dtype], seed=1234, hop=hop)


def materialised(feed, dtype):
    """The same windows cut out of the bank's rounded table on the host, as (N, F, T) fp32, in a feed packed the existing way."""
    bank = feed.Y
    tab = bank.table.float().cpu().numpy()
    Y = np.stack([tab[s: s + bank.T, : bank.F].T for s in bank.starts_host])
    return twin(feed, torch.from_numpy(np.ascontiguousarray(Y)).to(DEV)).pack_embeddings(DT[dtype])


IDX = np.array([3, 17, 17, 39, 0, 21, 8, 30, 11, 2, 5, 6])


@pytest.mark.parametrize("dtype", ["bf16", "fp16"])
def test_feed_equals_the_feed_of_materialised_windows_and_so_does_the_loss(dtype):
    from speech_decoding_amd import CLIPLoss, WindowBank, ops
    feed, train_idx, test_idx = track_feed(dtype)
    bank = feed.Y
    assert isinstance(bank, WindowBank) and len(feed) == len(bank) == 40 and bank.dtype == DT[dtype]
    assert len(train_idx) == 28 and len(test_idx) == 12 and not set(train_idx) & set(test_idx)
    assert np.diff(bank.starts_host[:10]).max() < bank.T                        # neighbouring segments overlap
    assert bank.table.shape[0] * 2 < 40 * (bank.T + 16)                         # ... so the tracks are smaller than the packed table
    mat = materialised(feed, dtype)
    X, Y, subj = feed.batch(IDX)
    X0, Y0, subj0 = mat.batch(IDX)
    B, F, T = Y.shape
    assert (B, F, T) == (12, 32, 40) and Y.dtype == DT[dtype]
    assert torch.equal(X, X0) and torch.equal(subj, subj0) and subj.dtype == torch.int32
    assert torch.equal(Y, Y0)
    base, base0 = ops.rows_base(Y, B, F, T, DT[dtype]), ops.rows_base(Y0, B, F, T, DT[dtype])
    assert base is not None and base0 is not None                               # the loss's packed operand, consumed in place
    assert torch.equal(base.view(torch.int16), base0.view(torch.int16))         # the whole rows buffer: pad rows, padding, slack
    # the loss, its gradient for Z and for the temperature: the same bits from the two feeds' Y
    args = tiny_args()
    Zsrc = torch.randn(B, F, T, generator=torch.Generator().manual_seed(3)).to(DEV).to(DT[dtype])
    got = []
    for y in (Y, Y0):
        lossf = CLIPLoss(args).to(DEV)
        Z = Zsrc.clone().requires_grad_(True)
        loss = lossf(y, Z)
        loss.backward()
        assert bool(torch.isfinite(loss)) and Z.grad is not None and lossf.temp.grad is not None
        got.append((loss.detach().float().reshape(1), Z.grad.float(), lossf.temp.grad.float().reshape(-1)))
    for a, b in zip(*got):
        assert torch.equal(a.view(torch.int32), b.view(torch.int32))
    assert float(got[0][1].abs().max()) > 0


def test_sharded_batches_of_two_ranks_concatenate_to_the_one_rank_batch():
    from speech_decoding_amd.data import ShardedRandomSampler
    feed, train_idx, _ = track_feed("bf16")
    one = list(twin(feed, feed.Y).batches(ShardedRandomSampler(len(train_idx), 12, 3, 0, 1, seed=9), index_map=train_idx))
    ranks = [list(twin(feed, feed.Y).batches(ShardedRandomSampler(len(train_idx), 12, 3, r, 2, seed=9), index_map=train_idx))
             for r in range(2)]
    assert len(one) == 3
    for whole, a, b in zip(one, *ranks):
        assert a[1].shape[0] == b[1].shape[0] == 6
        for k in range(3):
            assert torch.equal(torch.cat([a[k], b[k]]), whole[k])


def same_bits(a, b):
    assert len(a) == len(b)
    for x, y in zip(a, b):
        assert (x is None) == (y is None)
        if x is not None:
            assert x.dtype == y.dtype and x.shape == y.shape
            assert torch.equal(x.view(torch.int32) if x.dtype == torch.float32 else x, y.view(torch.int32) if y.dtype == torch.float32 else y)


def test_select_shares_the_table_and_decodes_like_a_fresh_bank():
    from speech_decoding_amd import SdaError, WindowBank, retrieve
    from tests import window_bank_cases as W
    c = W.case("a", exact=False)
    dev = lambda x: torch.from_numpy(np.ascontiguousarray(x)).to(DEV)         # noqa: E731
    bank = WindowBank(c["F"], c["T"], device=DEV)
    for t, s in zip(c["tracks"], c["local"]):
        bank.add_track(dev(t), s)
    sel = np.random.RandomState(8).permutation(c["M"])[:300]
    sel[7] = sel[100]                                                           # a duplicate; the order is shuffled
    sub = bank.select(sel)
    assert len(sub) == 300 and sub.table.data_ptr() == bank.table.data_ptr() and sub.row_norms_sq.data_ptr() == bank.row_norms_sq.data_ptr()
    assert sub.starts.data_ptr() != bank.starts.data_ptr() and sub.norms_sq.data_ptr() != bank.norms_sq.data_ptr()
    assert np.array_equal(sub.starts_host, bank.starts_host[sel]) and sub.starts_host.dtype == np.int32
    assert torch.equal(sub.starts.cpu(), torch.from_numpy(bank.starts_host[sel]))
    assert torch.equal(sub.norms_sq.view(torch.int32).cpu(), bank.norms_sq.view(torch.int32).cpu()[torch.from_numpy(sel)])
    assert torch.equal(bank.select(torch.from_numpy(sel).to(DEV)).starts, sub.starts)         # device indices too
    fresh = WindowBank(c["F"], c["T"], device=DEV)                              # the same rows as ONE track, only those windows
    fresh.add_track(dev(np.concatenate(c["tracks"], axis=1)), bank.starts_host[sel])
    assert torch.equal(fresh.table.view(torch.int16), sub.table.view(torch.int16))
    assert torch.equal(fresh.norms_sq.view(torch.int32), sub.norms_sq.view(torch.int32))
    Q = dev(c["queries"])
    labels = (np.arange(c["N"]) * 53) % 300
    same_bits(retrieve(Q, sub, k=10, labels=labels), retrieve(Q, fresh, k=10, labels=labels))
    again = sub.select(np.arange(299, -1, -1))                                  # a selection of a selection still shares the table
    assert again.table.data_ptr() == bank.table.data_ptr() and np.array_equal(again.starts_host, sub.starts_host[::-1])
    with pytest.raises(SdaError, match="select"):
        sub.add_track(dev(c["tracks"][0]), [0])
    assert len(bank.add_track(dev(c["tracks"][0]), [0])) == 1                   # the owner still grows
    for bad in ([c["M"] + 1], [-1]):
        with pytest.raises(IndexError):
            bank.select(bad)
    for bad in ([[0, 1]], [0.5, 1.0], 3):
        with pytest.raises(ValueError):
            bank.select(np.asarray(bad))


def test_refusals_of_the_bank_backed_feed():
    import train as T
    from speech_decoding_amd import SdaError
    from speech_decoding_amd.data import synthetic_track_dataset
    feed, _, test_idx = track_feed("bf16")
    assert feed.pack_embeddings(torch.bfloat16) is feed and feed._Yt is None     # no copy
    with pytest.raises(SdaError, match="16-bit.*materialised"):
        feed.pack_embeddings(torch.float32)
    with pytest.raises(SdaError, match="bfloat16"):
        feed.pack_embeddings(torch.float16)
    for bad in ([40], [3, -1]):
        with pytest.raises(IndexError):
            feed.batch(np.array(bad))
    with pytest.raises(SdaError, match="16-bit"):
        synthetic_track_dataset(tiny_args(), DEV, n_segments=40, dtype=torch.float32)
    assert feed.speech_bank() is feed.Y
    held_out = feed.speech_bank(test_idx)
    assert len(held_out) == len(test_idx) and held_out.table.data_ptr() == feed.Y.table.data_ptr()
    assert np.array_equal(held_out.starts_host, feed.Y.starts_host[test_idx])
    args = tiny_args()                                                          # compute_dtype fp32, the default
    args["data"] = "tracks"
    with pytest.raises(SdaError, match="16-bit"):
        T.run(args, log=lambda *a: None)


def test_training_driver_on_tracks_end_to_end(tmp_path, monkeypatch):
    import train as T
    monkeypatch.chdir(tmp_path)
    runs = []
    for _ in range(2):
        args = tiny_args(compute_dtype="bf16")
        args["data"] = "tracks"
        torch.manual_seed(0)
        np.random.seed(0)
        lines = []
        hist, enc, lossf = T.run(args, log=lambda *a: lines.append(" ".join(a)))
        assert len(hist) == 2 and len(lines) == 2 and lines[0].startswith("Ep 0/2 | ") and "testTop10acc" in lines[1]
        assert all(np.isfinite(h["train_loss"]) and np.isfinite(h["test_loss"]) for h in hist)
        assert all(0.0 <= h["testTop10acc"] <= 1.0 for h in hist)
        runs.append(lines)
    assert runs[0] == runs[1]
