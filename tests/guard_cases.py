"""Cases, a NumPy restatement and the checks of the gradient guard (csrc/grad_guard.hip, sda_adam_multi_guarded):
sda_grad_sumsq_multi's partial layout, sda_grad_guard_finish's rules and the guarded update.  The checks take the thing under
test as a function: tests/test_grad_guard_gpu.py hands them the HIP launches, tests/test_grad_guard_cpu.py the restatement — clean
(every check passes) and with one planted bug at a time (MUTANTS; every one fails a check).  Nothing here needs a GPU.

Conditions (none comes from a kernel's output):
  family (a)  integers |g| <= 2^10: every g^2 and every partial sum is an integer below 2^53, so any summation order in double is
              exact and the reference is compared with ==, slot by slot.
  (b), (c)    a double sum of N non-negative terms, in any order, is within (N - 1) 2^-53 relative of the exact sum; two such
              sums (kernel and reference) are within N 2^-52 of each other.  (c) holds one tensor at 3e38: its squares (9e76)
              overflow fp32 and not double, so the norm must come out finite.
  (d)         one inf / NaN element at a time: the count is exactly 1, and the finite sum is that of the other elements.
  finish      all inputs are small integers or powers of two, the rules are a handful of IEEE double operations: ==.
  COEF        the decision is taken in double and rounded once when Adam reads it: within one fp32 ulp of the float64 value for
              (b), equal to it where the sum of squares is a perfect square (sqrt is then exact)."""
import math

import numpy as np
import torch

from speech_decoding_amd import lib as L
from tests import elementwise_cases as E

G = {k[len("GUARD_"):]: v for k, v in L.CONSTANTS.items() if k.startswith("GUARD_")}       # slot name -> index (STATE: the size)
SHAPES = dict(E.adam_grads((), 0)[1], single=(1,))
NAMES = ("big", "three", "cplx", "offset", "zero", "never", "single")
MAGS = dict(big=1.0, three=1e-12, cplx=1e12, offset=1e-3, zero=0.0, single=1e6)
SENT = -7.0
B1, B2 = 0.9, 0.999


def numel(name):
    return int(np.prod(SHAPES[name]))


def gx_of(max_n):
    return min((max_n + 1023) // 1024, 256)


# ---------------------------------------------------------------------------------------------------------------
# cases: lists of (name, flat fp32 gradient or None, aligned)
# ---------------------------------------------------------------------------------------------------------------
def _case(values):
    return [(n, values.get(n), n != "offset") for n in NAMES]


def family_a(seed=61):
    g = torch.Generator().manual_seed(seed)
    vals = {n: torch.randint(-1024, 1025, (numel(n),), generator=g).float() for n in NAMES if n != "never"}
    vals["zero"].zero_()
    for n in ("big", "offset", "single", "cplx"):                  # the tail and the edges carry something to lose
        vals[n][-1] = 1024.0
        vals[n][0] = -1023.0
    return _case(vals)


def family_b(seed=67):
    g = torch.Generator().manual_seed(seed)
    return _case({n: torch.randn(numel(n), generator=g) * MAGS[n] for n in NAMES if n != "never"})


def family_c(seed=71):
    case = dict((n, v) for n, v, _ in family_b(seed))
    g = torch.Generator().manual_seed(seed)
    case["three"] = (torch.randint(0, 2, (3,), generator=g).float() * 2 - 1) * 3e38
    return _case({n: v for n, v in case.items() if v is not None})


SECOND_TRIP = 256 * 1024 + 5                                       # big: gx = 256, the second grid-stride trip starts at 262 144
POISON_AT = (("big", 0), ("big", numel("big") - 1), ("big", SECOND_TRIP), ("cplx", 2 * 17 + 1), ("single", 0))
POISON = (math.inf, -math.inf, math.nan)


def family_d():
    """[(label, case)]: family (a) with ONE element replaced, at each position by each of +inf, -inf, NaN"""
    out = []
    for name, at in POISON_AT:
        for bad in POISON:
            case = [(n, None if v is None else v.clone(), al) for n, v, al in family_a()]
            dict((n, v) for n, v, _ in case)[name][at] = bad
            out.append((f"{name}[{at}] = {bad}", case))
    return out


def many_tensors(seed=73, count=70):
    """70 tensors (grid.y beyond a real model's 60), 1 .. 2100 elements, integers; every third one unaligned"""
    g = torch.Generator().manual_seed(seed)
    sizes = [1 + int(torch.randint(0, 2100, (1,), generator=g)) for _ in range(count)]
    return [(f"t{i}", torch.randint(-1024, 1025, (s,), generator=g).float(), i % 3 != 0) for i, s in enumerate(sizes)]


def perfect_square_case():
    """sum g^2 = 9 x 262 144 + 16 x 262 144 = 25 x 2^18: sqrt = 2560 exactly"""
    return [("a", torch.full((262144,), 3.0), True), ("b", torch.full((262144,), -4.0), False)]


def with_grad(case):
    return [(n, v, al) for n, v, al in case if v is not None]


# ---------------------------------------------------------------------------------------------------------------
# the restatement.  mutant: one planted bug (MUTANTS)
# ---------------------------------------------------------------------------------------------------------------
MUTANTS = ("fp32_squares", "skip_tail", "skip_second_trip", "imag_not_counted", "no_1e-6", "coef_not_clamped", "step_on_skip",
           "scale_below_1", "growth_past_max", "good_not_reset", "bias_from_old_step")


def ref_partials(case, mutant=None):
    """sda_grad_sumsq_multi: float64 (n, gx, 2).  Workgroup b of a tensor reads [trip gx 1024 + b 1024, + 1024) of every trip."""
    case = with_grad(case)
    gx = gx_of(max(v.numel() for _, v, _ in case))
    out = np.zeros((len(case), gx, 2))
    for t, (name, v, _) in enumerate(case):
        g = v.numpy()
        n = g.size
        keep = np.ones(n, dtype=bool)
        if mutant == "skip_tail":
            keep[n - n % 4:] = False
        if mutant == "skip_second_trip":
            keep[gx * 1024:] = False
        if mutant == "imag_not_counted" and name == "cplx":
            keep[1::2] = False
        fin = np.isfinite(g)
        for b in range(min(gx, (n + 1023) // 1024)):
            idx = np.concatenate([np.arange(lo, min(lo + 1024, n)) for lo in range(b * 1024, n, gx * 1024)])
            idx = idx[keep[idx]]
            sel = g[idx][fin[idx]]
            if mutant == "fp32_squares":
                with np.errstate(over="ignore"):
                    s = np.float32(0)
                    for chunk in np.array_split(sel * sel, max(1, sel.size // 256)):        # (an fp32 accumulator per thread)
                        s = np.float32(s + chunk.sum(dtype=np.float32))
                out[t, b, 0] = float(s)
            else:
                out[t, b, 0] = float((sel.astype(np.float64) ** 2).sum())
            out[t, b, 1] = float((~fin[idx]).sum())
    return out


def f32(x):
    return float(np.float32(x))


def ref_finish(partials, state, max_norm, growth_interval, max_scale, dynamic, b1=B1, b2=B2, mutant=None):
    """sda_grad_guard_finish on float64 `state` (a new array is returned)"""
    st = np.array(state, dtype=np.float64)
    flat = np.asarray(partials, dtype=np.float64).reshape(-1, 2)
    s, c = float(flat[:, 0].sum()), float(flat[:, 1].sum())
    scale = st[G["SCALE"]]
    st[G["SUMSQ"]], st[G["NONFINITE"]] = s, c
    if c > 0:
        st[G["SKIP"]], st[G["GOOD"]], st[G["NORM"]], st[G["COEF"]] = 1.0, 0.0, math.inf, 0.0
        st[G["SKIPPED"]] += 1.0
        if mutant == "step_on_skip":
            st[G["STEP"]] += 1.0
        if dynamic:
            st[G["SCALE"]] = scale * 0.5 if mutant == "scale_below_1" else max(1.0, scale * 0.5)
        return st
    old_step = st[G["STEP"]]
    step, good = old_step + 1.0, st[G["GOOD"]] + 1.0
    if dynamic and good >= growth_interval:
        st[G["SCALE"]] = 2.0 * scale if mutant == "growth_past_max" else min(max_scale, 2.0 * scale)
        if mutant != "good_not_reset":
            good = 0.0
    norm = math.sqrt(s) / scale
    clip = 1.0
    if 0.0 < max_norm < math.inf:
        clip = max_norm / (norm + (0.0 if mutant == "no_1e-6" else 1e-6))
        if mutant != "coef_not_clamped":
            clip = min(1.0, clip)
    k = old_step if mutant == "bias_from_old_step" else step
    st[G["SKIP"]], st[G["STEP"]], st[G["GOOD"]], st[G["NORM"]], st[G["COEF"]] = 0.0, step, good, norm, (1.0 / scale) * clip
    st[G["BC1"]] = f32(1.0 - f32(b1) ** k)
    st[G["BC2_SQRT"]] = f32(math.sqrt(1.0 - f32(b2) ** k))
    return st


def ref_guarded_adam(p, g, m, v, state, lr=1e-3, b1=B1, b2=B2, eps=1e-8):
    """sda_adam_multi_guarded on flat fp32 tensors: untouched on a skip, else adam_multi_kernel (E.emul_adam) on fl32(g coef)"""
    if state[G["SKIP"]] != 0:
        return p, m, v
    coef = torch.tensor(state[G["COEF"]], dtype=torch.float64).float()
    return E.emul_adam(p, g * coef, m, v, int(state[G["STEP"]]), lr=lr, b1=b1, b2=b2, eps=eps)


def new_state(scale=1.0, step=0, good=0, skipped=0):
    st = np.zeros(G["STATE"])
    st[G["SCALE"]], st[G["STEP"]], st[G["GOOD"]], st[G["SKIPPED"]] = scale, step, good, skipped
    return st


# ---------------------------------------------------------------------------------------------------------------
# checks.  sumsq(case) -> float64 (n, gx, 2) of the tensors with a gradient, the buffer pre-filled with SENT by the caller's
# launcher;  finish(partials, state, max_norm, growth_interval, max_scale, dynamic) -> float64 state
# ---------------------------------------------------------------------------------------------------------------
def totals(parts):
    return float(parts[:, :, 0].sum()), float(parts[:, :, 1].sum())


def exact64(case):
    """(sum of squares of the finite elements, count of the others, element count) in float64 on the host"""
    s, c, n = 0.0, 0, 0
    for _, v, _ in with_grad(case):
        d = v.double()
        fin = torch.isfinite(d)
        s += float((d[fin] ** 2).sum())
        c += int((~fin).sum())
        n += v.numel()
    return s, c, n


def check_norm_pass(sumsq):
    for label, case in (("a", family_a()), ("70 tensors", many_tensors())):
        got, want = sumsq(case), ref_partials(case)
        assert got.shape == want.shape, (label, got.shape, want.shape)
        assert np.array_equal(got, want), (label, "slots differ from the float64 reference", np.argwhere(got != want)[:4].tolist())
        for t, (_, v, _) in enumerate(with_grad(case)):            # workgroups past a tensor's end wrote zeros over the sentinel
            assert not got[t, (v.numel() + 1023) // 1024:].any(), (label, t)
        s, c, _ = exact64(case)
        assert totals(got) == (s, float(c)) and c == 0, label
    for label, case in (("b", family_b()), ("c", family_c())):
        got = sumsq(case)
        s, c, n = exact64(case)
        gs, gc = totals(got)
        assert gc == 0.0 and math.isfinite(gs), (label, gs, gc)
        assert abs(gs - s) <= n * 2.0 ** -52 * s, (label, gs, s)
        assert math.isfinite(math.sqrt(gs)), label
        assert np.array_equal(got, sumsq(case)), (label, "two runs differ")
    for label, case in family_d():
        got = sumsq(case)
        s, c, _ = exact64(case)
        assert c == 1
        assert totals(got) == (s, 1.0), (label, totals(got), s)
        assert np.array_equal(got, ref_partials(case)), (label, "the count is in the wrong slot")


def spread(n, gx, sumsq_terms, bad_at=()):
    """hand-made partials (n, gx, 2): the terms dealt over the slots from the last one backwards, counts of 1 at bad_at"""
    p = np.zeros((n, gx, 2))
    flat = p.reshape(-1, 2)
    for i, term in enumerate(sumsq_terms):
        flat[-1 - (i * 7) % len(flat), 0] += term
    for at in bad_at:
        flat[at, 1] += 1.0
    return p


# (label, partials, state in, max_norm, growth_interval, max_scale, dynamic).  9 x 2^20 = 3072^2: norm 3 at scale 1024.
NINE = [2.0 ** 20] * 9
FINISH_CASES = (
    ("no clipping, max_norm 0", spread(3, 5, NINE), new_state(1024.0), 0.0, 2000, 2.0 ** 24, 1),
    ("no clipping, max_norm inf", spread(3, 5, NINE), new_state(1024.0, step=3, good=3), math.inf, 2000, 2.0 ** 24, 1),
    ("max_norm 1.5 below norm 3", spread(3, 5, NINE), new_state(1024.0, step=1, good=1), 1.5, 2000, 2.0 ** 24, 1),
    ("max_norm 4 above norm 3", spread(3, 5, NINE), new_state(1024.0, step=1, good=1), 4.0, 2000, 2.0 ** 24, 1),
    ("280 slots, scale 1 static", spread(70, 4, [4.0] * 64), new_state(1.0, step=6, good=6), 8.0, 2000, 2.0 ** 24, 0),
    ("skip halves the scale", spread(3, 5, NINE, bad_at=(14,)), new_state(1024.0, step=5, good=3, skipped=2), 1.5, 2000, 2.0 ** 24, 1),
    ("skip at scale 1 stays 1", spread(3, 5, NINE, bad_at=(0, 7)), new_state(1.0, step=5, good=3), 0.0, 2000, 2.0 ** 24, 1),
    ("skip, static scale", spread(70, 4, NINE, bad_at=(279,)), new_state(1024.0, step=5, good=3), 0.0, 2000, 2.0 ** 24, 0),
    ("growth", spread(3, 5, NINE), new_state(2.0 ** 23, step=40, good=9), 0.0, 10, 2.0 ** 24, 1),
    ("growth capped at max_scale", spread(3, 5, NINE), new_state(2.0 ** 24, step=40, good=9), 0.0, 10, 2.0 ** 24, 1),
    ("one short of growth", spread(3, 5, NINE), new_state(1024.0, step=40, good=8), 0.0, 10, 2.0 ** 24, 1),
    ("no growth when static", spread(3, 5, NINE), new_state(1024.0, step=40, good=9), 0.0, 10, 2.0 ** 24, 0),
    ("bias correction of step 7", spread(3, 5, NINE), new_state(1024.0, step=6, good=6), 0.0, 2000, 2.0 ** 24, 1),
)
SLOT_NAMES = [k for k in G if k != "STATE"]


def check_finish(finish):
    for label, parts, st, max_norm, gi, max_scale, dyn in FINISH_CASES:
        got, want = finish(parts, st, max_norm, gi, max_scale, dyn), ref_finish(parts, st, max_norm, gi, max_scale, dyn)
        bad = [k for k in SLOT_NAMES if not (got[G[k]] == want[G[k]])]
        assert not bad, (label, {k: (got[G[k]], want[G[k]]) for k in bad})
        assert not got[len(SLOT_NAMES):].any(), (label, "a slot without a name was written")
    # the rules' own words on a few of the cases, so that the restatement is not the only witness
    by = {c[0]: ref_finish(*c[1:]) for c in FINISH_CASES}
    assert by["no clipping, max_norm 0"][G["COEF"]] == 2.0 ** -10 and by["no clipping, max_norm 0"][G["NORM"]] == 3.0
    assert by["max_norm 4 above norm 3"][G["COEF"]] == 2.0 ** -10
    assert by["max_norm 1.5 below norm 3"][G["COEF"]] == 2.0 ** -10 * (1.5 / (3.0 + 1e-6))
    assert by["skip halves the scale"][G["SCALE"]] == 512.0 and by["skip halves the scale"][G["STEP"]] == 5.0
    assert by["skip at scale 1 stays 1"][G["SCALE"]] == 1.0 and by["skip, static scale"][G["SCALE"]] == 1024.0
    assert by["growth"][G["SCALE"]] == 2.0 ** 24 == by["growth capped at max_scale"][G["SCALE"]] and by["growth"][G["GOOD"]] == 0.0
    assert by["one short of growth"][G["SCALE"]] == 1024.0 == by["no growth when static"][G["SCALE"]]
    assert by["bias correction of step 7"][G["BC1"]] == f32(1.0 - f32(0.9) ** 7)


def check_coef(sumsq, finish):
    """the two launches together: COEF of family (b) within one fp32 ulp of the float64 value, equal on a perfect square"""
    for label, case, scale, max_norm, exact in (("b", family_b(), 1.0, 1e10, False), ("b scaled", family_b(), 1024.0, 1e6, False),
                                                ("perfect square", perfect_square_case(), 4.0, 160.0, True)):
        st = finish(sumsq(case), new_state(scale), max_norm, 2000, 2.0 ** 24, 0)
        s, c, _ = exact64(case)
        norm = math.sqrt(s) / scale
        want = (1.0 / scale) * min(1.0, max_norm / (norm + 1e-6))
        assert c == 0 and want < 1.0 / scale, (label, "the case does not clip")
        if exact:
            assert norm == 640.0 and st[G["NORM"]] == norm and st[G["COEF"]] == want, (label, st[G["COEF"]], want)
        else:
            assert abs(f32(st[G["COEF"]]) - want) <= float(E.ulp(torch.tensor(want), torch.float32)), (label, st[G["COEF"]], want)
