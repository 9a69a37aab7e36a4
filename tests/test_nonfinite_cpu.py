"""CPU proof that the propagation and containment checks of tests/nonfinite_cases.py have teeth: each of the four ways a kernel
swallows or leaks a non-finite value, planted into the plain-torch restatement of the construct, is caught, and every unmutated
restatement passes.  Without this file tests/test_nonfinite_gpu.py proves nothing.

The same for the cases of tests/test_nonfinite_losses_gpu.py (the labelled, sigmoid and negatives loss kernels): every case it
runs reaches an output and leaves something for the bit check, and the mutants planted in the case modules' emul_* functions —
a masked lse whose maximum skips NaN, a label mask applied by multiplication, a logaddexp on fmaxf / fminf, a saturating 16-bit
store, a partial sum that skips non-finite terms, a windows product that reads a row outside the window against a zero
coefficient — fail N.check where their restatements pass."""
import pytest
import torch

from tests import nonfinite_cases as N

# which check has to catch which mutant
CAUGHT_BY = {"softmax_skips_nan": "propagation", "saturating_store": "propagation", "mask_by_multiply": "containment",
             "colsum_skips_nonfinite": "propagation"}


def failures(name, mutant):
    """{what: {output: check -> message}} of the cases the (mutated) restatement fails; the reference is the restatement"""
    clean, ref_clean = N.restatement(name, N.cpu_operands(), mutant), N.restatement(name, N.cpu_operands())
    out = {}
    for what, o in N.cpu_cases():
        ref, got = N.restatement(name, o), N.restatement(name, o, mutant)
        bad = {k: r for k in ref for r in [N.check(ref[k], got[k], clean[k], ref_clean[k])] if r}
        if bad:
            out[what] = bad
    return out


@pytest.mark.parametrize("name", N.MUTANTS)
def test_every_restatement_passes_both_checks(name):
    assert failures(name, None) == {}


@pytest.mark.parametrize("name", N.MUTANTS)
def test_every_mutant_is_caught(name):
    bad = failures(name, name)
    kinds = {k for per_case in bad.values() for per_out in per_case.values() for k in per_out}
    assert CAUGHT_BY[name] in kinds, (name, bad)


def test_each_poison_value_catches_the_saturating_store_in_the_type_it_overflows():
    """+-inf in both types, 1e5 in fp16 only (bf16 holds it), 3.4e38 in both: each must be stored as inf"""
    x = torch.zeros(1, 4)
    for v, types in ((N.INF, ("fp16", "bf16")), (-N.INF, ("fp16", "bf16")), (1e5, ("fp16",)), (3.4e38, ("fp16", "bf16"))):
        o = dict(x=N.poisoned(x, (0, 1), v))
        ref, got = N.restatement("saturating_store", o), N.restatement("saturating_store", o, "saturating_store")
        clean = N.restatement("saturating_store", dict(x=x), "saturating_store")
        caught = {k.split()[1] for k in ref if "propagation" in N.check(ref[k], got[k], clean[k], clean[k])}
        assert caught == set(types), (v, caught)
    assert torch.isinf(N.stored(torch.tensor([1e5], dtype=torch.float64), torch.float16)).all()
    assert torch.isinf(N.stored(torch.tensor([3.4e38], dtype=torch.float64), torch.bfloat16)).all()
    assert torch.isfinite(N.stored(torch.tensor([65504.0, 65519.0]), torch.float16)).all()


def test_the_checks_themselves():
    """propagation: a swallowed NaN; containment: a leaked inf, and a finite element whose bits moved (a -0 for a +0 included);
    an inf where the reference has NaN, or of the other sign, is no failure"""
    ref = torch.tensor([1.0, N.NAN, N.INF, 0.0])
    clean = torch.tensor([1.0, 2.0, 3.0, 0.0])
    chk = lambda got: set(N.check(ref, torch.tensor(got), clean, clean))
    assert chk([1.0, N.INF, -N.INF, 0.0]) == set() and chk([1.0, N.NAN, N.NAN, 0.0]) == set()
    assert chk([1.0, 2.0, N.INF, 0.0]) == {"propagation"}
    assert chk([N.INF, N.NAN, N.INF, 0.0]) == {"containment"}
    assert chk([1.0000001, N.NAN, N.INF, 0.0]) == {"containment"}
    assert chk([1.0, N.NAN, N.INF, -0.0]) == {"containment"}
    assert chk([N.NAN, 2.0, 3.0, 0.0]) == {"propagation", "containment"}
    # a finite element whose reference moved with the poison owes finiteness, not the clean run's bits
    moved = torch.tensor([1.5, N.NAN, N.INF, 0.0])
    assert N.check(moved, torch.tensor([1.25, N.NAN, N.INF, 0.0]), clean, clean) == {}
    assert set(N.check(moved, torch.tensor([N.NAN, N.NAN, N.INF, 0.0]), clean, clean)) == {"containment"}
    with pytest.raises(AssertionError, match="propagation"):
        N.check_all("k", {"y": ref}, {"y": clean}, {"y": clean}, {"y": clean})
    N.check_all("k", {"y": ref}, {"y": ref}, {"y": clean}, {"y": clean})


def test_positions_name_every_edge():
    """first / last row, both sides of a tile boundary inside a sample and of one in memory rows, channel 0 and C - 1"""
    p = N.positions(3, 70, 40, t_edges=(64,), flat_edges=(256,))
    rows = {(b, t) for b, t, _ in p.values()}
    assert {(0, 0), (2, 69), (1, 63), (1, 64), (2, 67), (2, 68)} <= rows          # memory row 256 = 2 * 86 + 16 + 68
    assert {c for _, _, c in p.values()} == {0, 39}
    assert N.row_positions(2, 40, flat_edges=(56,)).keys() == {"first row of the first sample", "last row of the last sample",
                                                               "memory row 55, below the boundary at 56"}     # row 56 is a pad row


# ---------------------------------------------------------------------------------------------------------------
# the loss kernels behind labels, SigmoidLoss and extra negatives: the cases tests/test_nonfinite_losses_gpu.py runs
# ---------------------------------------------------------------------------------------------------------------
def loss_case_groups():
    """(id, maker) of every group of cases the GPU tests run"""
    for b in N.LOSS_BLOCKS:
        for p in N.LOSS_PATTERNS:
            yield f"labels-{b}-{p}", lambda b=b, p=p: N.label_cases(*b, p)
            yield f"sigmoid-{b}-{p}", lambda b=b, p=p: N.sigmoid_cases(*b, p)
    for s in N.NEG_SHAPES:
        yield f"negatives-{s}", lambda s=s: N.neg_cases(*s)
    for s in N.DZ_SHAPES:
        for p in N.DZ_PATTERNS:
            yield f"dz_windows-{s}-{p}", lambda s=s, p=p: N.dz_cases(*s, p)
    for s in N.SIM_SHAPES:
        yield f"sim_gemm-{s}", lambda s=s: N.sim_cases(*s)


GROUPS = dict(loss_case_groups())


@pytest.mark.parametrize("group", GROUPS)
def test_no_loss_case_passes_vacuously(group):
    """for every case used on the GPU: every site reaches an output with at least one poison value (a dropped pair's site: with
    none, by the contract), and unless the maths couples the whole output (said per site) at least one element stays finite and
    independent of the poison, so the bit check has something to hold"""
    n = 0
    for case in GROUPS[group]():
        o, ref = case["operands"], case["ref"]
        ref_clean = ref(o)
        assert case["unreached"] <= {s[0] for s in case["sites"]} and case["coupled"] <= {s[0] for s in case["sites"]}
        if case["finite_clean"]:
            assert all(bool(torch.isfinite(t).all()) for t in ref_clean.values()), (case["kernel"], case["what"])
        for site, key, index in case["sites"]:
            reached = False
            for vname, v in case["values"].items():
                r = ref(dict(o, **{key: N.poisoned(o[key], index, v)}))
                reached = reached or any(bool((torch.isfinite(t) != torch.isfinite(ref_clean[k])).any()) for k, t in r.items())
                independent = any(bool((torch.isfinite(t) & (t == ref_clean[k])).any()) for k, t in r.items())
                assert independent or site in case["coupled"], (case["kernel"], case["what"], site, vname, "nothing is left for the bit check")
                n += 1
            assert reached == (site not in case["unreached"]), (case["kernel"], case["what"], site, "reached" if reached else "no value reaches an output")
    assert n > 0


# mutant -> (group of cases, kernels it is planted in, the check that has to catch it)
LOSS_MUTANTS = {
    "lse_max_skips_nan": ("labels-(15, 5, 10)-pair", {"clip_logits_stats_masked"}, "propagation"),
    "mask_by_multiply": ("labels-(15, 5, 10)-pair", {"clip_grad_labels", "clip_grad_y_labels"}, "containment"),
    "masked_times_zero": ("sigmoid-(15, 5, 10)-pair", {"sigmoid_grad_y", "sigmoid_pairs + sigmoid_finish"}, "containment"),
    "merge_with_fmaxf": ("negatives-(2, 31)", {"clip_neg_stats"}, "propagation"),
    "saturating_store": ("labels-(15, 5, 10)-pair", {"clip_grad_labels", "clip_grad_y_labels"}, "propagation"),
    "saturating_store (SigmoidLoss)": ("sigmoid-(15, 5, 10)-pair", {"sigmoid_grad_y", "sigmoid_pairs + sigmoid_finish"}, "propagation"),
    "saturating_store (negatives)": ("negatives-(2, 31)", {"clip_neg_grad"}, "propagation"),
    "colsum_skips_nonfinite": ("labels-(15, 5, 10)-pair", {"clip_grad_labels", "clip_grad_y_labels"}, "propagation"),
    "colsum_skips_nonfinite (SigmoidLoss)": ("sigmoid-(15, 5, 10)-pair", {"sigmoid_grad_y", "sigmoid_pairs + sigmoid_finish"}, "propagation"),
    "colsum_skips_nonfinite (negatives)": ("negatives-(2, 31)", {"clip_neg_grad"}, "propagation"),
    "window_row_outside_times_zero": ("dz_windows-(2, 31, 5)-overlap", {"clip_dz_windows"}, "containment"),
}


def loss_failures(case, mutant):
    """{(site, value): {output: check -> message}} of one case with `mutant` standing in for its restatement"""
    o, ref = case["operands"], case["ref"]
    clean, ref_clean = ref(o, mutant), ref(o)
    out = {}
    for site, key, index in case["sites"]:
        for vname, v in case["values"].items():
            p = dict(o, **{key: N.poisoned(o[key], index, v)})
            r, got = ref(p), ref(p, mutant)
            bad = {k: res for k in r for res in [N.check(r[k], got[k], clean[k], ref_clean[k])] if res}
            if bad:
                out[(site, vname)] = bad
    return out


@pytest.mark.parametrize("mutant", LOSS_MUTANTS)
def test_every_loss_mutant_is_caught_and_its_restatement_passes(mutant):
    group, kernels, kind = LOSS_MUTANTS[mutant]
    seen = set()
    for case in GROUPS[group]():
        if case["kernel"] not in kernels or (mutant.startswith("saturating") and case["dtype"] == torch.float32):
            continue
        if mutant in ("mask_by_multiply", "masked_times_zero") and case.get("mode") != "mask":
            continue
        assert loss_failures(case, None) == {}, (case["kernel"], case["what"])
        bad = loss_failures(case, mutant.split(" (")[0])
        kinds = {k for per_case in bad.values() for per_out in per_case.values() for k in per_out}
        assert kind in kinds, (mutant, case["kernel"], case["what"], bad)
        seen.add(case["kernel"])
    assert seen == kernels, (mutant, seen)


def test_the_exceptions_waive_no_more_than_they_say():
    """the data-gradient conv: pad channels only, and only in frames whose real channels are non-finite — a leak into another
    real channel of a poisoned frame, into a pad channel of another frame, or into a real channel's sum is still caught.
    wgrad_gemm: the other taps of a weight with a non-finite tap, nothing else."""
    k = "conv_gemm (data gradient)"
    assert set(N.EXCEPTIONS) == {k, "wgrad_gemm", "sim_gemm"}
    B, C, Cp, T = 2, 3, 5, 4
    clean = torch.arange(B * Cp * T, dtype=torch.float32).reshape(B, Cp, T)
    ref = clean.clone()
    ref[1, 2, 3] = N.NAN                                   # a poisoned saved operand: one element of frame (1, 3)
    split = lambda t: N.split_pad("dx", t, C)
    sums = lambda v: {"sums": v[:C].clone(), "sums" + N.PAD: v[C:].clone()}
    zero = torch.zeros(Cp)

    def outcome(at=None, sum_at=None):
        got, s = ref.clone(), zero.clone()
        if at is not None:
            got[at] = N.NAN
        if sum_at is not None:
            s[sum_at] = N.NAN
        try:
            N.check_all(k, dict(split(ref), **sums(zero)), dict(split(got), **sums(s)), dict(split(clean), **sums(zero)),
                        dict(split(clean), **sums(zero)))
            return "passes"
        except AssertionError as e:
            assert "containment" in str(e) and "propagation" not in str(e)
            return "caught"
    assert outcome() == "passes"
    assert outcome(at=(1, 4, 3)) == "passes"               # a pad channel of the poisoned frame
    assert outcome(sum_at=4) == "passes"                   # a pad channel's sum
    assert outcome(at=(1, 1, 3)) == "caught"               # another REAL channel of the poisoned frame
    assert outcome(at=(1, 4, 2)) == "caught"               # a pad channel of the frame next to it
    assert outcome(at=(0, 4, 3)) == "caught"               # a pad channel of the same frame of another sample
    assert outcome(sum_at=1) == "caught"                   # a real channel's sum
    # an output handed over whole (no pad channels named) gets no waiver at all
    with pytest.raises(AssertionError, match="containment"):
        got = ref.clone()
        got[1, 4, 3] = N.NAN
        N.check_all(k, {"dx": ref}, {"dx": got}, {"dx": clean}, {"dx": clean})
    g0 = torch.zeros(2, 3, 4, 3)                           # (segment, co, ci, tap)
    gref = g0.clone()
    gref[1, 2, 1, 1] = N.INF
    for at, want in (((1, 2, 1, 0), "passes"), ((1, 2, 0, 1), "caught"), ((0, 2, 1, 0), "caught"), ((1, 1, 1, 0), "caught")):
        got = gref.clone()
        got[at] = N.NAN
        try:
            N.check_all("wgrad_gemm", {"g": gref}, {"g": got}, {"g": g0}, {"g": g0})
            res = "passes"
        except AssertionError:
            res = "caught"
        assert res == want, (at, res)
    # sim_gemm: the pad columns of a row whose last real column is non-finite, nothing else
    s0, p0 = torch.ones(3, 4), torch.zeros(3, 2)
    sref = s0.clone()
    sref[1, 3] = N.NAN                                     # row 1's last real column
    sref[2, 0] = N.INF                                     # row 2: a non-finite column that is not the last
    for name, at, want in (("S" + N.PAD_COLS, (1, 0), "passes"), ("S" + N.PAD_COLS, (2, 1), "caught"), ("S" + N.PAD_COLS, (0, 1), "caught"),
                           ("S", (0, 3), "caught"), ("S", (1, 0), "caught")):
        got = {"S": sref.clone(), "S" + N.PAD_COLS: p0.clone()}
        got[name][at] = N.NAN
        try:
            N.check_all("sim_gemm", {"S": sref, "S" + N.PAD_COLS: p0}, got, {"S": s0, "S" + N.PAD_COLS: p0}, {"S": s0, "S" + N.PAD_COLS: p0})
            res = "passes"
        except AssertionError as e:
            assert "containment" in str(e) and "propagation" not in str(e)
            res = "caught"
        assert res == want, (name, at, res)
