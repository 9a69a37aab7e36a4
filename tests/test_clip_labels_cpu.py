"""tests/clip_label_cases.py on the CPU: the label patterns reach the edges they are named for; the fp32 emulation of every kernel
of csrc/clip_labels.hip passes its check_*() against float64 (with every exp moved by -1, 0, +1 ulp); the two new tolerance
constants are 4 .. 5 x what the emulation measures; seven planted bugs miss the tolerances by 10 x or more; and the float64
reference itself has the properties the loss is built on (all-distinct labels give the unlabelled loss, one class under `mask`
gives zero loss and zero D, the kernels' D formula is autograd's gradient of the two-line loss)."""
import math

import pytest
import torch

from tests import clip_label_cases as LC
from tests import sa_loss_cases as S

_BASE, _CASES = {}, {}


def case(shape, regime, pattern):
    """one case per key, shared and left unchanged"""
    key = (*shape, regime, pattern)
    if key not in _CASES:
        if key[:4] not in _BASE:
            _BASE[key[:4]] = S.clip_case(*shape, regime)
        _CASES[key] = LC.label_case(*shape, regime, pattern, base=_BASE[key[:4]])
    return _CASES[key]


def all_cases(shapes=LC.LABEL_SHAPES, regimes=LC.CLIP_REGIMES, patterns=LC.LABEL_PATTERNS):
    return [case(s, r, p) for s in shapes for r in regimes for p in patterns]


def worst(checks):
    return max(checks.values())


def test_patterns_reach_their_edges():
    for Bm, Bn, col0 in LC.LABEL_SHAPES:
        lab = {p: LC.labels_of(Bm, Bn, col0, p).to(torch.int64) for p in LC.LABEL_PATTERNS}
        inb = lambda i: col0 <= i < col0 + Bn
        assert lab["distinct"].unique().numel() == Bm
        assert lab["pair"].unique().numel() == Bm - 1 and lab["pair"][col0] == lab["pair"][col0 + Bn - 1]
        m3 = (lab["straddle3"] == 7).nonzero().flatten().tolist()
        assert len(m3) == 3 and any(inb(i) for i in m3)
        if Bm > Bn:
            assert sum(not inb(i) for i in m3) >= 1
            mo = (lab["partners_outside"] == 7).nonzero().flatten().tolist()
            assert len(mo) == 3 and sum(inb(i) for i in mo) == 1
        sizes = torch.bincount(lab["sizes"].unique(return_inverse=True)[1])
        assert int(sizes.max()) >= max(Bm // 2, 2) and (Bm < 8 or (int((sizes == 2).sum()) == 1 and int((sizes == 1).sum()) > 0))
        assert lab["one_class"].unique().numel() == 1
        ex = lab["extremes"]
        assert int(ex.min()) == -2 ** 31 and int(ex.max()) == 2 ** 31 - 1 and int((ex == ex.max()).sum()) == 2
        assert Bm < 4 or int((ex == ex.min()).sum()) == 2
        # ties + pair: row col0's repeat (the block's last column) has exactly the positive's logit, and beats it by neither rule
        c = case((Bm, Bn, col0), "ties", "pair")
        assert float(c["logits"][col0, Bn - 1]) == float(c["logits"][col0, 0]) == float(c["diag"][col0])
        assert int(S.ranks_ref(c)[col0 + Bn - 1]) >= 1 and int(LC.ranks_labels_ref(c)[col0 + Bn - 1]) == int(S.ranks_ref(c)[col0 + Bn - 1]) - 1
        # one class on a column block: the rows outside it keep nothing
        if Bm > Bn:
            assert int(LC.masked_stats_ref(case((Bm, Bn, col0), "flat", "one_class"))["empty"].sum()) == Bm - Bn


@pytest.mark.parametrize("shape", LC.LABEL_SHAPES, ids=str)
def test_emulations_pass_their_checks(shape):
    Bm, Bn, col0 = shape
    for c in all_cases([shape]):
        assert torch.equal(LC.emul_counts(c), c["counts"]), c["name"]
        assert torch.equal(LC.emul_ranks_labels(c), LC.ranks_labels_ref(c)), c["name"]
        for hw in LC.HW:
            r = worst(LC.check_masked_stats(c, *LC.emul_masked_stats(c, hw)))
            assert r <= 1.0, (c["name"], "masked stats", hw, r)
        for mode in LC.MODES:
            for dtype in LC.DTYPES:
                for hw in (LC.HW if dtype == LC.F32 else (0,)):
                    G, rs, cs, sc = LC.emul_grad_labels(c, mode, dtype, hw)
                    chk = LC.check_grad_labels(c, mode, dtype, G, rs, cs, sc)
                    assert worst(chk) <= 1.0, (c["name"], mode, dtype, hw, chk)
                    Gy, part = LC.emul_grad_y_labels(c, mode, dtype, hw)
                    chk = LC.check_grad_y_labels(c, mode, dtype, Gy, part)
                    assert worst(chk) <= 1.0, (c["name"], mode, dtype, hw, chk)


def test_tolerance_table_matches_the_emulation():
    m = LC.measure_constants(all_cases())
    chosen = dict(C_MLSE=LC.C_MLSE, C_PBAR=LC.C_PBAR)
    print({k: (v if k == "C_MLSE" else v / LC.U32) for k, v in m.items()})
    for k, v in m.items():
        assert 4.0 * v <= chosen[k] <= 5.0 * v, (k, v, chosen[k])


# planted bug -> (the cases it must show on, how it is run); each must miss a tolerance by 10 x or more on at least one case
def _grad(mode, mutant):
    def run(c):
        G, rs, cs, sc = LC.emul_grad_labels(c, mode, LC.F32, 0, mutant)
        Gy, part = LC.emul_grad_y_labels(c, mode, LC.F32, 0, mutant)
        return max(worst(LC.check_grad_labels(c, mode, LC.F32, G, rs, cs, sc)), worst(LC.check_grad_y_labels(c, mode, LC.F32, Gy, part)))
    return run


def _stats(mutant):
    return lambda c: worst(LC.check_masked_stats(c, *LC.emul_masked_stats(c, 0, mutant)))


def _ranks(mutant):
    return lambda c: S.exact(torch.equal(LC.emul_ranks_labels(c, mutant), LC.ranks_labels_ref(c)))


COL_BLOCKS = [s for s in LC.LABEL_SHAPES if s[2] != 0]
BUGS = {
    "T normalised by the block-local count": (COL_BLOCKS, ("partners_outside", "straddle3"), _grad("positive", "T_by_the_block_local_count")),
    "-2 delta kept in positive mode": (LC.LABEL_SHAPES, ("distinct", "pair"), _grad("positive", "delta_kept_in_positive_mode")),
    "the mask applied to the diagonal too": (LC.LABEL_SHAPES, ("pair", "sizes"), _stats("mask_on_the_diagonal_too")),
    "the mask applied to rows but not columns": (LC.LABEL_SHAPES, ("pair", "sizes"), _stats("mask_rows_not_columns")),
    "a masked entry leaking into dtemp or rscale": (LC.LABEL_SHAPES, ("pair", "sizes"), _grad("mask", "masked_entry_leaks_into_sums")),
    "label-blind ranks": (LC.LABEL_SHAPES, ("pair",), _ranks("label_blind_ranks")),
    "labels indexed without col0 (statistics)": (COL_BLOCKS, ("pair", "straddle3"), _stats("labels_without_col0")),
    "labels indexed without col0 (D, positive)": (COL_BLOCKS, ("pair", "straddle3"), _grad("positive", "labels_without_col0")),
    "labels indexed without col0 (D, mask)": (COL_BLOCKS, ("pair", "straddle3"), _grad("mask", "labels_without_col0")),
    "labels indexed without col0 (ranks)": (COL_BLOCKS, ("sizes", "one_class"), _ranks("labels_without_col0")),
}


@pytest.mark.parametrize("bug", list(BUGS), ids=str)
def test_planted_bugs_miss_the_tolerances(bug):
    shapes, patterns, run = BUGS[bug]
    miss = {c["name"]: run(c) for c in all_cases(shapes, ("flat", "trained", "ties"), patterns)}
    print(bug, "largest error / tolerance per case:", {k: f"{v:.3g}" for k, v in miss.items()})
    assert max(miss.values()) >= 10.0, (bug, miss)
    # and on every shape it is meant for, not on one lucky case
    for s in shapes:
        assert max(v for k, v in miss.items() if f"Bm={s[0]} Bn={s[1]} col0={s[2]} " in k) >= 10.0, (bug, s)


def test_counts_over_the_block_is_caught():
    assert any(not torch.equal(LC.emul_counts(c, "counts_over_the_block"), c["counts"]) for c in all_cases(COL_BLOCKS, ("flat",), ("partners_outside",)))


# ---- the float64 reference alone
@pytest.mark.parametrize("reduction", ["mean", "sum"])
def test_all_distinct_labels_give_the_unlabelled_loss(reduction):
    for shape in ((3, 3, 0), (64, 64, 0)):
        for regime in ("flat", "trained"):
            c = case(shape, regime, "distinct")
            l = c["Lg32"].double()
            lab = c["labels"].to(torch.int64)
            plain = float(LC.loss_ref(l, None, None, reduction))
            for mode in LC.MODES:
                assert abs(float(LC.loss_ref(l, lab, mode, reduction)) - plain) <= 1e-12 * abs(plain), (c["name"], mode)


def test_one_class_under_mask_gives_zero_loss_and_zero_D():
    for shape in ((3, 3, 0), (64, 64, 0), (140, 70, 70)):
        c = case(shape, "trained", "one_class")
        assert float(LC.loss_ref(c["Lg32"].double(), c["labels"].to(torch.int64), "mask")) == 0.0
        assert float(LC.global_D_ref(c, "mask").abs().max()) == 0.0
        assert float(LC.label_D(c, "mask")[0].abs().max()) == 0.0


@pytest.mark.parametrize("mode", LC.MODES)
def test_D_formula_is_autograds_gradient_of_the_two_line_loss(mode):
    """D of the kernels' formula (on the fp32-rounded lse they are handed) against d loss / d logits of the autograd form"""
    for shape in ((3, 3, 0), (64, 64, 0), (15, 5, 10), (140, 70, 70)):
        for pattern in LC.LABEL_PATTERNS:
            c = case(shape, "trained", pattern)
            D = LC.label_D(c, mode)[0]
            ref = LC.global_D_ref(c, mode)[:, c["col0"]:c["col0"] + c["Bn"]]
            assert float((D - ref).abs().max()) <= 1e-5, (c["name"], float((D - ref).abs().max()))


@pytest.mark.parametrize("mode", LC.MODES)
def test_loss_share_formula_sums_to_the_two_line_loss(mode):
    """the per-column shares of every block, summed over the blocks of the global batch, are the loss"""
    for shape, pattern in (((15, 5, 10), "straddle3"), ((140, 70, 70), "sizes"), ((64, 64, 0), "pair")):
        Bm, Bn, _ = shape
        base = case(shape, "trained", pattern)
        total = sum(float(LC.grad_labels_ref(LC.block_of(base, b0), mode, torch.float32)["scalars"][0]) for b0 in range(0, Bm, Bn))
        want = float(LC.loss_ref(base["Lg32"].double(), base["labels"].to(torch.int64), mode))
        assert abs(total - want) <= 1e-5 * abs(want), (shape, pattern, total, want)
