"""CPU-side proof for tests/test_exact_gpu.py: every case it imports from tests/exact_cases.py meets the conditions of its
regime (so none can silently stop exercising the rounding), the correct emulation equals the integer reference, and every
mutant of the reference differs from it on at least one case of each 16-bit type — with torch.equal as the only comparison."""
import pytest
import torch

from tests import exact_cases as X

ALL = [(r, d) for r in X.REGIMES for d in X.DTYPES]
ALL16 = [(r, d) for r in X.REGIMES for d in X.DTYPES16]


def test_stores_on_hand_picked_values():
    y = torch.tensor([257.0, 258.0, 259.0, -257.0, -259.0, 261.0, 256.0, 0.0, 3.0])       # bf16 step above 256 is 2
    assert X.store(y, torch.bfloat16).tolist() == [256.0, 258.0, 260.0, -256.0, -260.0, 260.0, 256.0, 0.0, 3.0]
    assert X.store(y, torch.bfloat16, "trunc").tolist() == [256.0, 258.0, 258.0, -256.0, -258.0, 260.0, 256.0, 0.0, 3.0]
    assert X.store(y, torch.bfloat16, "half_away").tolist() == [258.0, 258.0, 260.0, -258.0, -260.0, 262.0, 256.0, 0.0, 3.0]
    assert X.is_tie(y, torch.bfloat16).tolist() == [True, False, True, True, True, True, False, False, False]
    h = torch.tensor([2049.0, 2051.0, 4098.0, 4099.0, -4097.0, 2048.0, 0.5])                # fp16 step above 2048 is 2, above 4096 is 4
    assert X.store(h, torch.float16).tolist() == [2048.0, 2052.0, 4096.0, 4100.0, -4096.0, 2048.0, 0.5]
    assert X.store(h, torch.float16, "trunc").tolist() == [2048.0, 2050.0, 4096.0, 4096.0, -4096.0, 2048.0, 0.5]
    assert X.store(h, torch.float16, "half_away").tolist() == [2050.0, 2052.0, 4100.0, 4100.0, -4096.0, 2048.0, 0.5]
    assert X.is_tie(h, torch.float16).tolist() == [True, True, True, False, False, False, False]
    r = X.ints((4000,), 20000, 1)
    r = r[r != 0]
    for d in X.DTYPES16:                                # every mode returns a neighbour of y in d; rne is torch's cast
        lo, hi = X._trunc_next(r, d)
        assert bool(X.representable(lo, d).all()) and bool(X.representable(hi, d).all())
        assert bool(((lo.abs() <= r.abs()) & (r.abs() < hi.abs())).all())
        assert torch.equal(X.store(r, d), r.float().to(d).double())
    with pytest.raises(AssertionError):
        X.operand(torch.tensor([257.0]), torch.bfloat16)


def test_failure_helper_names_count_and_first_index():
    a = torch.zeros(2, 3, 200)
    b = a.clone()
    assert X.mismatch(a, b) is None
    b[1, 2, 128] = 4.0
    b[1, 2, 129] = 5.0
    msg = X.mismatch(a, b)
    assert "2 of 1200 differ" in msg and "(b, c, t) = (1, 2, 128)" in msg and "got 0.0 expected 4.0" in msg
    with pytest.raises(AssertionError, match="conv: 2 of 1200"):
        X.assert_same(a, b, "conv")


@pytest.mark.parametrize("regime,dtype", ALL)
def test_every_case_meets_the_conditions_of_its_regime(regime, dtype):
    """max |reference| < 2^24; exact regime: representable in all three types; rounding regime, 16-bit: |reference| <= 2^15 in
    fp16, >= 10 % of the outputs not representable in the stored type, >= 1 % exact ties — for every reference the GPU file
    compares a stored value with."""
    for i, s in enumerate(X.CONV3_SHAPES):
        case = X.conv3_case(i, regime, dtype)
        for epi in X.EPILOGUES:
            if epi == "bias_res" and case.res is None:
                continue
            X.check_regime(X.conv_expected(case, epi), regime, dtype, f"conv3 {tuple(s)} {epi}")
        X.operand(case.x, dtype), X.operand(case.w, dtype)
    g = X.glu_case(regime, dtype)
    X.check_regime(g.ref[:, X.GLU_HALF:], regime, dtype, "glu gate")
    for name in X.CONV1_SHAPES:
        if dtype == torch.float32 and name.startswith("wide"):
            continue
        c = X.conv1_case(name, regime, dtype)
        X.check_regime(c.ref, regime, dtype, f"conv1 {name}")
        if regime == "exact" and c.shape.cout % 128 == 0:
            assert float(X.row_sumsq_ref(c.ref).max()) < 2 ** 24
    for i in range(len(X.DGRAD_SHAPES)):
        X.check_regime(X.dgrad_case(i, regime, dtype).ref, regime, dtype, f"dgrad {i}")
    for i in range(len(X.TYPED_SHAPES)):
        X.check_regime(X.typed_case(i, regime, dtype).ref, regime, dtype, f"typed {i}")
    for i in range(len(X.IG_SHAPES)):
        X.check_regime(X.ig_case(i, regime, dtype).ref, regime, dtype, f"input_grad {i}")
    if dtype != torch.float32:
        for i in range(len(X.CLIP_SHAPES)):
            c = X.clip_case(i, regime, dtype)
            X.check_regime(c.ref, regime, dtype, f"clip_dz {i}")
            for t in (c.G, c.Y, c.Z):
                X.operand(t, dtype)


def test_fp32_result_cases_stay_below_2_24():
    for i, s in enumerate(X.WGRAD_SHAPES):
        c = X.wgrad_case(i)
        for seg, nseg in ((None, 1), (s.subjects, X.WGRAD_NSUBJ)):
            assert float(X.wgrad_ref(c.dy, c.x, s.KS, s.dil, seg, nseg).abs().max()) < 2 ** 24
        for d in X.DTYPES:
            X.operand(c.dy, d), X.operand(c.x, d)
    for i in range(len(X.SIM_SHAPES)):
        assert float(X.sim_case(i)[2].abs().max()) < 2 ** 24
    for form in X.PGEMM_FORMS:
        A, B = X.pgemm_operands(form)
        assert X.PGEMM_R ** 2 * 270 < 2 ** 24
    A, B = X.pgemm_operands("typed_out_into_view")
    X.check_regime(A @ B[:, :209], "rounding", torch.bfloat16, "param_gemm typed output")


def test_exact_regime_is_one_operand_set_for_all_types():
    """the cross-dtype equality check: the three storage types read the same integers and must store the same values"""
    for i in range(len(X.CONV3_SHAPES)):
        a, b, c = (X.conv3_case(i, "exact", d) for d in X.DTYPES)
        for o in (b, c):
            assert o.R == a.R and torch.equal(o.x, a.x) and torch.equal(o.w, a.w) and torch.equal(o.ref, a.ref)


@pytest.mark.parametrize("regime,dtype", ALL)
def test_correct_emulation_equals_the_reference(regime, dtype):
    for i in range(len(X.CONV3_SHAPES)):
        case = X.conv3_case(i, regime, dtype)
        X.assert_same(X.conv_emulation(case, dtype), X.store(case.ref, dtype), f"conv3 case {i}")


@pytest.mark.parametrize("mutant", X.CONV_MUTANTS)
def test_every_mutant_is_caught_in_each_16_bit_type(mutant):
    """counts of (shape, regime) cases out of 12 per type on which the mutant's stored values differ from the reference's"""
    caught = {}
    for dtype in X.DTYPES16:
        n = 0
        for regime in X.REGIMES:
            for i in range(len(X.CONV3_SHAPES)):
                case = X.conv3_case(i, regime, dtype)
                n += X.mismatch(X.conv_emulation(case, dtype, mutant), X.store(case.ref, dtype)) is not None
        caught[dtype] = n
    print(f"{mutant}: caught on {caught[torch.bfloat16]} (bf16) and {caught[torch.float16]} (fp16) of {2 * len(X.CONV3_SHAPES)} cases")
    assert all(n >= 1 for n in caught.values()), caught
