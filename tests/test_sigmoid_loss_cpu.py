"""CPU side of the pairwise sigmoid loss's tests: the cases of tests/sigmoid_loss_cases.py reach their edges, its tolerance table
is the one its emulation measures, the emulation (plain torch, fp32, the kernels' summation order) passes every check the HIP
kernels are held to in tests/test_sigmoid_loss_gpu.py, each planted bug misses one of them by 10 x or more, the float64 references
agree with autograd, and malformed arguments are refused before anything is launched."""
import math

import numpy as np
import pytest
import torch

from speech_decoding_amd import SigmoidLoss  # noqa: F401  (the feature under test: without it this file does not import)
from tests import builders as TB
from tests import sigmoid_loss_cases as SC

F32 = torch.float32
_CASES = {}


def case(shape, regime):
    key = (*shape, regime)
    if key not in _CASES:
        _CASES[key] = SC.sig_case(*shape, regime)
    return _CASES[key]


def labelled(shape, regime, pattern):
    return SC.with_labels(case(shape, regime), pattern)


def run_all(c, mode, dtype, hw=0, mutant=None):
    """every check of the three kernels on the emulation -> {name: error / tolerance}"""
    a, diag, G, part = SC.emul_pairs(c, mode, dtype, hw, mutant)
    out = {"pairs " + k: v for k, v in SC.check_pairs(c, mode, dtype, a, diag, G, part).items()}
    clean_part = SC.emul_pairs(c, mode, dtype, hw)[3][:-1]                   # the finisher is handed correct partials
    out.update({"finish " + k: v for k, v in SC.check_finish(c, clean_part, *SC.emul_finish(c, clean_part, hw, mutant)).items()})
    out.update({"grad_y " + k: v for k, v in SC.check_grad_y(c, mode, dtype, *SC.emul_grad_y(c, mode, dtype, hw, mutant)).items()})
    return out


# ---------------------------------------------------------------------------------------------------------------
# the cases and the table
# ---------------------------------------------------------------------------------------------------------------
def test_tolerance_table_matches_the_emulation():
    m = SC.measure_constants((lc, mode) for shape in SC.SHAPES for regime in SC.REGIMES for lc, mode in SC.variants(case(shape, regime)))
    print(m)
    for name, measured in m.items():
        chosen = getattr(SC, name)
        assert 4.0 * measured <= chosen <= 5.0 * measured, (name, measured, chosen)
    doc = SC.__doc__
    assert f"C_SIGD     {m['C_SIGD']:.2f}" in doc and f"C_SP       {m['C_SP']:.2f}" in doc


@pytest.mark.parametrize("shape", SC.SHAPES, ids=str)
def test_the_regimes_reach_their_edges(shape):
    hot, init = case(shape, "hot"), case(shape, "init")
    l = hot["a64"] + float(hot["bias"])
    assert float((l.abs() > 104).double().mean()) >= 0.10          # fp32 sigma is exactly 0 or 1 there
    assert float(l.abs().max()) > 1000                             # a loss term in the thousands
    li = init["a64"] + float(init["bias"])
    assert float(li.abs().max()) < 15
    assert float(init["temp"]) == pytest.approx(math.log(10.0)) and float(init["bias"]) == -10.0
    assert float(case(shape, "bias3")["bias"]) == 3.0


@pytest.mark.parametrize("shape", SC.LABEL_SHAPES, ids=str)
def test_every_label_pattern_has_a_repeat_inside_the_block(shape):
    for pattern in SC.LABEL_PATTERNS:
        c = labelled(shape, "trained", pattern)
        n = int((c["same"] & ~c["pos"]).sum())
        assert (n == 0) if pattern == "distinct" else (n >= 1), (pattern, n)
        assert int(c["labels"].numel()) == shape[0] and c["labels"].dtype == torch.int32
    assert set(SC.LABEL_SHAPES) <= set(SC.SHAPES)


def test_the_float64_references_agree_with_autograd():
    """D of the kernel reference = d loss_ref / d l / inv_norm on the global problem, in both modes and without labels"""
    for shape, pattern, mode in (((64, 64, 0), None, "positive"), ((64, 64, 0), "sizes", "positive"), ((64, 64, 0), "sizes", "mask"),
                                 ((3, 3, 0), "one_class", "mask")):
        c = case(shape, "bias3") if pattern is None else labelled(shape, "bias3", pattern)
        l = (c["a64"] + float(c["bias"])).clone().requires_grad_(True)
        lab = None if pattern is None else c["labels"].to(torch.int64)
        loss = SC.loss_ref(l, lab, mode, "mean")
        (g,) = torch.autograd.grad(loss, [l])
        t = SC.terms64(c["a64"], c["bias"], SC.signs(c, mode))
        assert float((g * shape[0] - t["D"]).abs().max()) <= 1e-14
        assert abs(float(loss.detach()) - float(t["sp"].sum()) / shape[0]) <= 1e-12 * max(1.0, abs(float(loss.detach())))


# ---------------------------------------------------------------------------------------------------------------
# the emulation passes; the planted bugs do not
# ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", SC.SHAPES, ids=str)
def test_the_emulation_passes_every_check(shape):
    worst = {}
    for regime in SC.REGIMES:
        for k, (lc, mode) in enumerate(SC.variants(case(shape, regime))):
            # every variant in fp32; the 16-bit stores and the moved exp / log1p on the unlabelled block and one labelled pattern
            runs = [(F32, 0)] + ([(torch.bfloat16, 1), (torch.float16, -1)] if lc["pattern"] in (None, "sizes") else [])
            for dtype, hw in runs:
                for name, r in run_all(lc, mode, dtype, hw).items():
                    worst[name] = max(worst.get(name, 0.0), r)
                    assert r <= 1.0, (lc["name"], mode, dtype, hw, name, r)
    print(shape, {k: round(v, 3) for k, v in worst.items()})


def _hits(c, mode, mutant, dtype=F32):
    clean, bad = run_all(c, mode, dtype), run_all(c, mode, dtype, mutant=mutant)
    assert all(r <= 1.0 for r in clean.values()), clean
    return {k: r for k, r in bad.items() if r >= 10.0}


BUGS = {   # mutant -> (shape, regime, label pattern, mode, the check that must miss by 10 x)
    "bias_left_out": ((64, 64, 0), "trained", None, "positive", "pairs G"),
    "sum_Dl_not_Da": ((64, 64, 0), "bias3", None, "positive", "pairs part"),
    "naive_log1pexp": ((64, 64, 0), "hot", None, "positive", "pairs part"),
    "ymax_local_rows": ((15, 5, 10), "trained", None, "positive", "pairs G"),
    "diag_without_col0": ((15, 5, 10), "trained", None, "positive", "pairs diag exactly zero outside the block"),
    "inv_norm_2B": ((64, 64, 0), "trained", None, "positive", "finish scalars[0] loss"),
    "dbias_without_inv_norm": ((64, 64, 0), "trained", None, "positive", "finish scalars[2] dbias"),
    "zero_row_unwritten": ((3, 3, 0), "trained", None, "positive", "pairs G zero row and pad columns exactly zero"),
    "pad_column_unwritten": ((3, 3, 0), "trained", None, "positive", "pairs G zero row and pad columns exactly zero"),
}


@pytest.mark.parametrize("mutant", sorted(BUGS))
def test_a_planted_bug_misses_by_ten_times(mutant):
    shape, regime, pattern, mode, check = BUGS[mutant]
    c = case(shape, regime) if pattern is None else labelled(shape, regime, pattern)
    hits = _hits(c, mode, mutant)
    print(mutant, hits)
    assert check in hits, (mutant, hits)


def test_sum_Dl_in_the_speech_side_partials_is_caught_too():
    assert "grad_y part" in _hits(case((64, 64, 0), "bias3"), "positive", "sum_Dl_not_Da")
    assert "grad_y Gy" in _hits(case((64, 64, 0), "trained"), "positive", "bias_left_out")


@pytest.mark.parametrize("mutant", ["zero_row_unwritten", "pad_column_unwritten"])
def test_unwritten_zeros_of_Gy_are_caught(mutant):
    hits = _hits(case((15, 5, 10), "trained"), "positive", mutant)
    assert ("grad_y Gy zero row exactly zero" if mutant == "zero_row_unwritten" else "grad_y Gy columns without a row exactly zero") in hits


@pytest.mark.parametrize("mode", SC.MODES)
def test_a_same_label_pair_counted_as_a_negative_is_caught(mode):
    hits = _hits(labelled((64, 64, 0), "trained", "pair"), mode, "same_label_as_negative")
    assert "pairs G" in hits or "pairs G of a dropped pair exactly zero" in hits, hits
    assert "grad_y Gy" in hits or "grad_y Gy of a dropped pair exactly zero" in hits, hits
    assert "pairs part" in hits, hits


def test_one_minus_sigma_is_caught():
    """a positive pair at l = 15: sigma(-l) = 3e-7, where 1 - sigma(l) has two bits left"""
    c = dict(case((64, 64, 0), "trained"), bias=torch.tensor([12.0]))
    hits = _hits(c, "positive", "one_minus_sigma")
    assert "pairs G" in hits and "grad_y Gy" in hits, hits


def test_a_masked_pair_multiplied_by_zero_is_caught():
    c = labelled((64, 64, 0), "trained", "pair")
    p, ij = SC.dropped_pair_case(c)
    clean = SC.emul_pairs(c, "mask", F32)
    good = SC.check_dropped_nan(ij, *SC.emul_pairs(p, "mask", F32)[2:], *clean[2:])
    bad = SC.check_dropped_nan(ij, *SC.emul_pairs(p, "mask", F32, mutant="masked_times_zero")[2:], *clean[2:])
    assert all(r == 0.0 for r in good.values()), good
    assert bad["G of the dropped NaN pair exactly zero"] == math.inf and bad["the sums keep the clean run's bits"] == math.inf


@pytest.mark.parametrize("value", [math.nan, math.inf])
@pytest.mark.parametrize("where", ["S", "ysq", "bias"])
def test_nonfinite_inputs_propagate_in_the_emulation(where, value):
    c = case((15, 5, 10), "trained")
    p = SC.poisoned(c, where, value)
    clean = SC.emul_pairs(c, "positive", F32)

    def run(mutant=None):
        a, diag, G, part = SC.emul_pairs(p, "positive", F32, mutant=mutant)
        return SC.check_nonfinite(c, p, where, "positive", F32, G, SC.emul_finish(p, part[:-1])[2], clean[2])

    good = run()
    assert all(r == 0.0 for r in good.values()), good
    if where == "ysq" and value != value:          # fmaxf drops the NaN: ymax stays finite and so does the rest of G
        assert run("fmaxf_ymax")["G non-finite exactly where the formulas say"] == math.inf


# ---------------------------------------------------------------------------------------------------------------
# refusals, before any launch
# ---------------------------------------------------------------------------------------------------------------
def test_arguments_are_refused_before_any_launch(monkeypatch):
    from speech_decoding_amd import SdaError, SigmoidLoss, lib, ops

    def boom(*a, **k):
        raise AssertionError("the library was reached before the arguments were refused")

    monkeypatch.setattr(lib, "load", boom)
    Bm, Bn = 6, 3
    S, ysq, zsq, one = torch.zeros(Bm, 64), torch.ones(Bm), torch.ones(Bn), torch.zeros(1)
    a = torch.zeros(Bm, Bn)
    with pytest.raises(SdaError, match="device tensors"):                                   # host tensors
        ops.sigmoid_pairs(S, ysq, zsq, one, one, Bm, Bn, 0, F32)
    with pytest.raises(SdaError, match="device tensors"):
        ops.sigmoid_grad_y(a, one, zsq, zsq, 0, F32)
    with pytest.raises(SdaError, match="device tensors"):
        ops.sigmoid_finish(torch.zeros(1, Bn, 3), ysq, zsq, one, 0.5)
    for bad in ("ignore", "negative", ""):                                                  # an unknown duplicates mode
        with pytest.raises(ValueError, match="duplicates"):
            ops.sigmoid_pairs(S, ysq, zsq, one, one, Bm, Bn, 0, F32, torch.zeros(Bm, dtype=torch.int32), bad)
        with pytest.raises(ValueError, match="duplicates"):
            ops.sigmoid_grad_y(a, one, zsq, zsq, 0, F32, None, bad)
    for lab in (torch.zeros(Bm - 1, dtype=torch.int32), torch.zeros(Bm + 1, dtype=torch.int32)):    # labels of the wrong length
        with pytest.raises(SdaError, match=f"int32 tensor of {Bm} values"):
            ops.sigmoid_pairs(S, ysq, zsq, one, one, Bm, Bn, 0, F32, lab, "mask")
        with pytest.raises(SdaError, match=f"int32 tensor of {Bm} values"):
            ops.sigmoid_grad_y(a, one, zsq, zsq, 0, F32, lab, "mask")
    for col0 in (4, -1):                                                                    # col0 + Bn > Bm
        with pytest.raises(SdaError, match="col0"):
            ops.sigmoid_pairs(S, ysq, zsq, one, one, Bm, Bn, col0, F32)
        with pytest.raises(SdaError, match="col0"):
            ops.sigmoid_grad_y(a, one, zsq, zsq, col0, F32)


def test_the_loss_refuses_bad_arguments(monkeypatch):
    from speech_decoding_amd import SdaError, SigmoidLoss, ops
    from speech_decoding.utils.loss import SigmoidLoss as shim
    assert shim is SigmoidLoss
    crit = SigmoidLoss(TB.Config(reduction="mean"))
    assert crit.temp.item() == pytest.approx(math.log(10.0)) and crit.bias.item() == -10.0 and crit.duplicates == "positive"
    crit = SigmoidLoss(TB.Config(reduction="sum", sigmoid_init_temperature=1.5, sigmoid_init_bias=-4.0, clip_duplicates="mask"))
    assert crit.temp.item() == 1.5 and crit.bias.item() == -4.0 and crit.duplicates == "mask" and crit.reduction == "sum"
    assert [n for n, _ in crit.named_parameters()] == ["temp", "bias"]
    with pytest.raises(ValueError, match="reduction"):
        SigmoidLoss(TB.Config(reduction="none"))
    for bad in ("ignore", "negative", ""):
        with pytest.raises(ValueError, match="duplicates"):
            SigmoidLoss(TB.Config(reduction="mean", clip_duplicates=bad))

    def boom(*a, **k):
        raise AssertionError("a kernel was launched before the arguments were refused")

    for name in ("pack_rows", "rows_sumsq", "matmul_nt_splitk", "upload_small", "sigmoid_pairs"):
        monkeypatch.setattr(ops, name, boom)
    x, y = torch.zeros(4, 8, 5), torch.zeros(4, 8, 5)
    with pytest.raises(SdaError, match="must live on the MI355X device"):
        crit(x, y)
    with pytest.raises(ValueError, match="expected 4 speech ids"):
        crit(x, y, labels=np.arange(5))
