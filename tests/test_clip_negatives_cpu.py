"""tests/clip_negative_cases.py on the CPU: the cases reach their edges, the fp32 emulations of the kernels pass their own
check_*() functions, the one new constant is 4 .. 5 x what the emulation measures, every planted bug misses a tolerance by 10 x or
more on some case; draw_negatives (the same draw on every rank, disjoint from the batch, its own generator), its error paths, the
refusal of a tensor in a bank's place, and the new header entries.  No GPU."""
import numpy as np
import pytest
import torch

from tests import clip_negative_cases as NC

MISS = 10.0


def worst(checks):
    return max(checks.values())


def stats_cases():
    for shape in NC.STATS_SHAPES:
        for regime in NC.STATS_REGIMES:
            yield NC.stats_case(*shape, regime)


def test_cases_reach_their_edges():
    ns = {s[1] for s in NC.STATS_SHAPES} | {s[1] for s in NC.DZ_SHAPES}
    assert {1, 31, 32, 33, 255, 256, 257, 289} <= ns                         # both sides of a K-step and of a 256 tile, a second pass
    assert {s[2] * NC.DZ_FP for s in NC.DZ_SHAPES} == {256, 320, 576}        # one whole tile, a partial one, more than two
    assert {2, 64, 65, 257} <= {s[0] for s in NC.DZ_SHAPES}
    dom, neg = NC.stats_case(5, 32, "dominant"), NC.stats_case(5, 32, "negligible")
    assert bool((dom["col_lse_merged"] > dom["col_lse"] + 5).all())          # the negatives carry the column soft-max
    assert torch.equal(neg["col_lse_merged"], neg["col_lse"])                # or vanish in it
    L, T = NC.DZ_TABLE_ROWS, 5
    for pattern in NC.START_PATTERNS:
        s = NC.starts_of(33, L, T, pattern)
        assert s.dtype == np.int32 and s.min() >= 0 and s.max() <= L - T
    e = NC.starts_of(33, L, T, "edges")
    assert e[0] == 0 and e[-1] == L - T                                      # a window at table row 0, one ending at the last row
    assert len(set(NC.starts_of(33, L, T, "same").tolist())) <= 17           # two negatives with the same start
    assert bool((np.diff(NC.starts_of(33, L, T, "overlap")) == 1).all())     # overlapping windows
    d = NC.starts_of(33, L, T, "descending")
    assert bool((np.diff(d) <= 0).all()) and d[0] == L - T and d[-1] == 0


@pytest.mark.parametrize("shape", NC.STATS_SHAPES, ids=str)
def test_emulated_stats_and_grad_pass(shape):
    for regime in NC.STATS_REGIMES:
        c = NC.stats_case(*shape, regime)
        Bn, N = shape
        for hw in NC.HW:
            m, cl = NC.emul_neg_stats(c, hw)
            mbuf, cbuf = torch.full((Bn + 1, N), NC.SENT), torch.full((Bn + 1,), NC.SENT)
            mbuf[:Bn], cbuf[:Bn] = m, cl
            checks = NC.check_neg_stats(c, mbuf, cbuf)
            assert worst(checks) <= 1.0, (c["name"], hw, checks)
            for dtype in NC.DTYPES16:
                checks = NC.check_neg_grad(c, dtype, *NC.emul_neg_grad(c, dtype, hw))
                assert worst(checks) <= 1.0, (c["name"], hw, dtype, checks)


def test_tolerance_table_matches_the_emulation():
    m = NC.measure_constants(list(stats_cases()))
    print(m)
    assert 4.0 * m["C_MERGE"] <= NC.C_MERGE <= 5.0 * m["C_MERGE"], m


@pytest.mark.parametrize("mutant", ["col_lse_not_merged", "merge_replaces_col_lse"])
def test_planted_stats_bugs_are_caught(mutant):
    seen = 0.0
    for c in stats_cases():
        Bn, N = c["Bn"], c["N"]
        m, cl = NC.emul_neg_stats(c, 0, mutant)
        mbuf, cbuf = torch.full((Bn + 1, N), NC.SENT), torch.full((Bn + 1,), NC.SENT)
        mbuf[:Bn], cbuf[:Bn] = m, cl
        seen = max(seen, worst(NC.check_neg_stats(c, mbuf, cbuf)))
    assert seen >= MISS, (mutant, seen)


@pytest.mark.parametrize("mutant", ["gn_wrong_norm", "rscale_share_missing", "dtemp_share_missing"])
def test_planted_grad_bugs_are_caught(mutant):
    seen = 0.0
    for c in stats_cases():
        seen = max(seen, worst(NC.check_neg_grad(c, torch.bfloat16, *NC.emul_neg_grad(c, torch.bfloat16, 0, mutant))))
    assert seen >= MISS, (mutant, seen)


@pytest.mark.parametrize("dtype", NC.DTYPES16, ids=str)
def test_emulated_dz_windows_passes(dtype):
    for shape in NC.DZ_SHAPES:
        for k, pattern in enumerate(NC.START_PATTERNS):
            for ints in (False, True):
                c = NC.dz_case(*shape, pattern, dtype, exact_ints=ints)
                checks = NC.check_dz_windows(c, dtype, NC.emul_dz_windows(c, dtype))
                assert worst(checks) <= 1.0, (c["name"], ints, checks)


def test_exact_cases_are_exact_in_fp32():
    """every partial sum of an exact_ints case stays an integer multiple of 2^-3 below 2^24 * 2^-3: fp32 holds it exactly"""
    for shape in NC.DZ_SHAPES:
        c = NC.dz_case(*shape, "edges", torch.bfloat16, exact_ints=True)
        absum = c["Gn"].abs().sum(0).max() * c["table"].abs().max()
        assert float(absum) * 8 + 8 * 8 < 2 ** 24
        ref, _ = NC.dz_windows_ref(c, torch.bfloat16)
        assert torch.equal(ref * 8, (ref * 8).round())
        assert not torch.equal(ref.to(torch.bfloat16).double(), ref) or shape[1] < 255     # the rounding is exercised


@pytest.mark.parametrize("mutant", ["window_row_early", "window_row_late", "last_partial_kstep_dropped", "pad_rows_written"])
def test_planted_dz_windows_bugs_are_caught(mutant):
    seen = 0.0
    for shape in NC.DZ_SHAPES:
        for pattern in NC.START_PATTERNS:
            c = NC.dz_case(*shape, pattern, torch.bfloat16)
            seen = max(seen, worst(NC.check_dz_windows(c, torch.bfloat16, NC.emul_dz_windows(c, torch.bfloat16, mutant))))
    assert seen >= MISS, (mutant, seen)


# ---------------------------------------------------------------------------------------------------------------
# the whole pipeline
# ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("reduction", ["mean", "sum"])
def test_emulated_pipeline_matches_float64_autograd(reduction):
    for case in NC.PIPE_CASES:
        c = NC.pipe_case(*case)
        figs = NC.pipeline_figures(c, None, reduction)
        print(c["name"], reduction, figs)
        assert worst(figs) <= 1.0, (c["name"], figs)


@pytest.mark.parametrize("mutant", NC.PIPE_MUTANTS)
def test_planted_pipeline_bugs_are_caught(mutant):
    seen = 0.0
    for case in NC.PIPE_CASES:
        seen = max(seen, worst(NC.pipeline_figures(NC.pipe_case(*case), mutant)))
    print(mutant, seen)
    assert seen >= MISS, (mutant, seen)


def test_reference_without_negatives_is_the_plain_loss():
    """N -> the negatives' logits at -inf: the two-line form is tests/clip_label_cases.loss_ref, labelled or not"""
    from tests import clip_label_cases as LC
    g = torch.Generator().manual_seed(3)
    l = torch.randn(6, 6, generator=g, dtype=torch.float64)
    m = torch.full((4, 6), -1e30, dtype=torch.float64)
    lab = torch.tensor([1, 2, 1, 3, 4, 4])
    for labels, mode in ((None, "positive"), (lab, "positive"), (lab, "mask")):
        for red in ("mean", "sum"):
            assert abs(float(NC.loss_ref(l, m, labels, mode, red)) - float(LC.loss_ref(l, labels, mode, red))) < 1e-12
    m2 = torch.randn(4, 6, generator=g, dtype=torch.float64)
    assert float(NC.loss_ref(l, m2)) > float(LC.loss_ref(l, None, "positive")) + 1e-3      # a real negative raises the loss


# ---------------------------------------------------------------------------------------------------------------
# draw_negatives
# ---------------------------------------------------------------------------------------------------------------
class _Bank:
    def __init__(self, starts):
        self.starts_host = np.asarray(starts, dtype=np.int32)

    def __len__(self):
        return len(self.starts_host)


def fake_feed(starts, seed=5):
    """a feed whose speech side is a bank of windows at `starts` (host side only: draw_negatives never touches the device)"""
    from speech_decoding_amd import data as D

    class Feed(D._ResidentEmbeddings):
        def __init__(self):
            self.Y = _Bank(starts)
            self.rng = np.random.RandomState(seed)

        def _bank(self):
            return self.Y
    return Feed()


def test_draw_negatives_is_the_same_on_every_rank_and_avoids_the_batch():
    starts = np.arange(60) // 2 * 3                         # every speech id twice: two segments share a window
    pool = np.arange(0, 50)
    batch = np.array([0, 7, 7, 20, 41, 55])
    a, b = fake_feed(starts), fake_feed(starts)
    np.random.seed(11)
    g0, r0 = np.random.get_state()[1].copy(), a.rng.get_state()[1].copy()
    for step in range(3):
        da, db = a.draw_negatives(16, batch, pool), b.draw_negatives(16, batch, pool)
        assert np.array_equal(da, db)                       # two simulated ranks
        assert len(set(da.tolist())) == 16 and set(da.tolist()) <= set(pool.tolist())
        assert not set(starts[da].tolist()) & set(starts[batch].tolist())     # no id of the batch, the partner segment included
    assert not np.array_equal(a.draw_negatives(16, batch, pool), da)          # the stream moves on
    assert np.array_equal(np.random.get_state()[1], g0) and np.array_equal(a.rng.get_state()[1], r0)
    assert fake_feed(starts)._neg_rng is None               # a run that never asks has made no generator and no draw


def test_draw_negatives_error_paths():
    from speech_decoding_amd import data as D
    from speech_decoding_amd.lib import SdaError
    starts = np.arange(20)
    f = fake_feed(starts)
    with pytest.raises(ValueError, match="the pool holds 6 segments"):
        f.draw_negatives(7, np.arange(4), np.arange(10))
    assert len(f.draw_negatives(6, np.arange(4), np.arange(10))) == 6
    with pytest.raises(ValueError, match="at least 1"):
        f.draw_negatives(0, np.arange(4), np.arange(10))
    with pytest.raises(IndexError):
        f.draw_negatives(2, np.arange(4), np.array([3, 20]))

    class Materialised(D._ResidentEmbeddings):
        Y = torch.zeros(4, 3, 5)
    with pytest.raises(SdaError, match="materialised Y"):
        Materialised().draw_negatives(1, [0], [1, 2])


def test_a_tensor_in_a_banks_place_is_refused():
    from speech_decoding_amd.lib import SdaError
    from speech_decoding_amd.loss import speech_negatives
    with pytest.raises(SdaError, match="must be a WindowBank"):
        speech_negatives(torch.zeros(4, 3, 5), 3, 5, torch.bfloat16, "cpu")
    assert speech_negatives(None, 3, 5, torch.bfloat16, "cpu") is None


def test_train_refuses_clip_negatives_without_tracks_or_clip():
    import train
    from tests.builders import Config
    for over in (dict(data="resident"), dict(data="tracks", loss="sigmoid"), dict(data="tracks", loss="mse"), dict()):
        with pytest.raises(ValueError, match="clip_negatives=8 needs data=tracks"):
            train.run(Config(clip_negatives=8, **over))
    with pytest.raises(ValueError, match="clip_negatives=-1"):
        train.run(Config(clip_negatives=-1, data="tracks"))


def test_header_declares_the_new_entries_at_abi_4():
    from speech_decoding_amd import lib as L
    assert L.ABI_VERSION == 4
    protos = L.PROTOTYPES
    assert protos["sda_clip_neg_stats"] == ("int", ["const float*", "long", "const float*", "const float*", "const float*", "float*", "float*",
                                                    "int", "int", "void*"])
    assert protos["sda_clip_neg_rows"] == ("int", ["int"])
    assert protos["sda_clip_neg_grad"][1][5:8] == ["float", "void*", "long"] and len(protos["sda_clip_neg_grad"][1]) == 16
    assert protos["sda_clip_dz_windows_span"] == ("long", ["long"])
    assert protos["sda_clip_dz_windows"] == ("int", ["const void*", "long", "const void*", "const int32_t*", "int", "long", "long", "void*", "long",
                                                     "const float*", "const float*", "int", "int", "long", "int", "void*"])
