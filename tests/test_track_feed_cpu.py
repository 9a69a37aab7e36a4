"""Training batches gathered from resident speech tracks, the part that needs no GPU: the numpy restatement of
sda_gather_windows (tests/track_feed_cases.py) against slicing and stacking written here, the planted bugs it tells apart, the C
entry's refusals (no kernel is launched: the library loads without a device, as in tests/test_capi_cpu.py), train.py's refusal of
data=tracks for another dataset, and the sampler's rank slices."""
import ctypes
import os

import numpy as np
import pytest
import torch

from tests import track_feed_cases as K

UTYPES = {"16-bit": np.uint16, "fp32 bytes": np.uint32}


@pytest.fixture(scope="module")
def lib():
    from speech_decoding_amd import lib as L
    if not os.path.exists(L.LIB_PATH):
        import __graft_entry__ as g
        g.build()
    return L


def stacked(c):
    """The expected destination written without the restatement's loop: windows stacked, 16 zero rows in front of each, zero slack."""
    T, Cp = c["T"], c["Cp"]
    wins = np.stack([c["table"][s: s + T] for s in c["starts"][c["idx"]]])                  # (B, T, Cp)
    body = np.concatenate([np.zeros((c["B"], 16, Cp), dtype=wins.dtype), wins], axis=1).reshape(c["B"] * (T + 16), Cp)
    return np.concatenate([body, np.zeros((16 + 128 + 32, Cp), dtype=wins.dtype)])


@pytest.mark.parametrize("width", list(UTYPES))
@pytest.mark.parametrize("name", K.CASES)
def test_restatement_equals_slicing_and_stacking(name, width):
    c = K.case(name, UTYPES[width])
    table, F = c["table"], c["F"]
    assert table.shape == (sum(c["lens"]), c["Cp"]) and not table[:, F:].any() and table[:, :F].all()
    if name != "c" or width == "fp32 bytes":
        assert len(np.unique(table[:, :F])) == table[:, :F].size                # distinct in every element
    else:
        assert all(len(np.unique(r)) == F for r in table[:, :F])                # 16-bit, 780 x 1024 elements: distinct inside a row ...
        assert not (table[1:, :F] == table[:-1, :F]).any()                      # ... and against the neighbouring row
    got = K.gather_windows_ref(table, c["starts"], c["idx"], c["T"])
    assert got.shape == (K.rows_alloc(c["B"], c["T"]), c["Cp"]) and got.dtype == table.dtype
    assert np.array_equal(got, stacked(c))                                      # (every element written: none keeps the fill)


def test_cases_cover_what_they_claim():
    a1, a7, b, c = (K.case(n) for n in K.CASES)
    assert a1["Cp"] * 2 == 128 and a1["B"] == 1 and a7["B"] == 7 and b["B"] == 9 and c["B"] == 3 and b["Cp"] == 128
    assert len(set(a7["idx"])) < 7 and list(a7["idx"]) != sorted(a7["idx"]) and len(set(b["idx"])) < 9
    for x in (a7, b, c):                                                        # each track's first and last legal start
        row0 = 0
        for n in x["lens"]:
            assert row0 in x["starts"] and row0 + n - x["T"] in x["starts"]
            row0 += n
    assert a1["starts"][a1["idx"][0]] + a1["T"] == 32                           # B = 1 reads the table's final rows
    assert np.diff(np.sort(b["starts"])).min() <= 3 < b["T"]                    # heavy overlap
    # case c against the launch rule of sda_gather_windows (ceil(vectors / 2048) workgroups of 256 lanes per sample): the four-fold
    # unrolled loop runs and leaves a tail, and a sample is shared by several workgroups
    vecs = c["T"] * c["Cp"] * 2 // 16
    bx = -(-vecs // 2048)
    assert bx > 1 and vecs // (bx * 256) >= 4 and vecs % (4 * bx * 256) != 0


@pytest.mark.parametrize("bug", K.BUGS)
def test_planted_bugs_are_told_apart(bug):
    seen = 0
    for width in UTYPES.values():
        for name in K.CASES:
            c = K.case(name, width)
            good = K.gather_windows_ref(c["table"], c["starts"], c["idx"], c["T"])
            bad = K.gather_windows_bugged(c["table"], c["starts"], c["idx"], c["T"], c["F"], bug)
            if (bug == "sample stride T" and c["B"] == 1) or (bug == "channel padding not carried" and c["F"] == c["Cp"]):
                continue                                        # one sample has no stride; case c has no padding channel
            assert not np.array_equal(good, bad), (bug, name)
            seen += 1
    assert seen >= 6


def test_out_of_range_candidates_restate_to_zero_samples():
    c = K.case("a7")
    idx = c["idx"].copy()
    idx[2], idx[5] = len(c["starts"]), -1
    got = K.gather_windows_ref(c["table"], c["starts"], idx, c["T"])
    want = K.gather_windows_ref(c["table"], c["starts"], c["idx"], c["T"])
    Tp = c["T"] + 16
    for b in range(7):
        rows = slice(b * Tp, (b + 1) * Tp)
        assert (not got[rows].any()) if b in (2, 5) else np.array_equal(got[rows], want[rows])


def test_c_entry_refuses_bad_arguments_without_a_launch(lib):
    """Every refusal named in sd_amd.h, each with its own message; the pointers are never dereferenced (nothing is launched)."""
    L = lib.load()
    ok = dict(table=4096, table_rows=32, starts=8192, M=6, idx=12288, dst=16384, B=7, T=5, row_bytes=128)

    def call(**kw):
        a = dict(ok, **kw)
        rc = L.sda_gather_windows(a["table"], a["table_rows"], a["starts"], a["M"], a["idx"], a["dst"], a["B"], a["T"], a["row_bytes"], None)
        return rc, L.sda_last_error().decode()

    for name in ("table", "starts", "idx", "dst"):
        rc, msg = call(**{name: None})
        assert rc == -1 and "gather_windows" in msg and "null" in msg, (name, msg)
    for name in ("B", "T", "M"):
        for v in (0, -3):
            rc, msg = call(**{name: v})
            assert rc == -1 and "at least 1" in msg and f"{name}={v}" in msg, (name, msg)
    rc, msg = call(table_rows=4)
    assert rc == -1 and "holds no window" in msg and "4 rows" in msg
    for rb in (0, 64, 192, 136, -128):
        rc, msg = call(row_bytes=rb)
        assert rc == -1 and "multiple of 128" in msg, (rb, msg)
    for name in ("table", "dst"):
        rc, msg = call(**{name: ok[name] + 8})
        assert rc == -1 and "16-byte aligned" in msg, (name, msg)


def test_signature_is_bound(lib):
    assert "sda_gather_windows" in lib.SIGNATURES
    assert hasattr(ctypes.CDLL(lib.LIB_PATH), "sda_gather_windows")
    header = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "sd_amd.h")).read()
    assert "sda_gather_windows" in header.split("#define SDA_ROW_PAD")[0]      # named in the "still 4, additions only" list


def test_train_refuses_tracks_for_another_dataset_before_touching_a_device(monkeypatch):
    import train as T
    from speech_decoding_amd import load_config
    args = load_config(overrides=["dataset=Brennan2018", "num_subjects=3"])
    args["data"] = "tracks"

    def no_device(*a, **k):
        raise AssertionError("a device was touched before the refusal")
    monkeypatch.setattr(torch.cuda, "set_device", no_device)
    with pytest.raises(ValueError, match="data=tracks"):
        T.run(args, log=lambda *a: None)


def test_two_rank_slices_concatenate_to_the_one_rank_batch():
    from speech_decoding_amd.data import ShardedRandomSampler
    one = list(ShardedRandomSampler(57, 12, 5, 0, 1, seed=4321))
    ranks = [list(ShardedRandomSampler(57, 12, 5, r, 2, seed=4321)) for r in range(2)]
    assert len(one) == 5 and all(len(r) == 5 for r in ranks)
    for whole, a, b in zip(one, *ranks):
        assert len(a) == len(b) == 6 and torch.equal(torch.cat([a, b]), whole)
