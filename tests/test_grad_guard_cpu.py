"""The gradient guard without a GPU: tests/guard_cases.py's NumPy restatement of the three launches passes every check the GPU
test applies to the HIP kernels, and each planted bug fails one of them; the three entry points refuse bad arguments before any
launch; train.run refuses an unknown fp16_guard before it touches a device."""
import ctypes
import math

import numpy as np
import pytest
import torch

from tests import elementwise_cases as E
from tests import guard_cases as GC

NORM_MUTANTS = ("fp32_squares", "skip_tail", "skip_second_trip", "imag_not_counted")
FINISH_MUTANTS = tuple(m for m in GC.MUTANTS if m not in NORM_MUTANTS)


def test_the_restatement_passes_every_check():
    GC.check_norm_pass(GC.ref_partials)
    GC.check_finish(GC.ref_finish)
    GC.check_coef(GC.ref_partials, GC.ref_finish)


@pytest.mark.parametrize("mutant", NORM_MUTANTS)
def test_norm_pass_checks_catch(mutant):
    with pytest.raises(AssertionError):
        GC.check_norm_pass(lambda case: GC.ref_partials(case, mutant=mutant))


@pytest.mark.parametrize("mutant", FINISH_MUTANTS)
def test_finish_checks_catch(mutant):
    assert set(NORM_MUTANTS) | set(FINISH_MUTANTS) == set(GC.MUTANTS)
    with pytest.raises(AssertionError):
        GC.check_finish(lambda *a: GC.ref_finish(*a, mutant=mutant))


def test_cases_are_what_they_claim():
    a = dict((n, v) for n, v, _ in GC.family_a())
    assert a["never"] is None and a["big"].numel() == 262144 + 1029 and a["big"].numel() % 4 == 1 and a["single"].numel() == 1
    assert GC.gx_of(a["big"].numel()) == 256 and 256 * 1024 < GC.SECOND_TRIP < a["big"].numel()
    s, c, n = GC.exact64(GC.family_a())
    assert c == 0 and s < 2.0 ** 53 and s == int(s) and n * 2.0 ** 20 < 2.0 ** 53
    c3 = dict((n, v) for n, v, _ in GC.family_c())["three"]
    assert bool(torch.isinf(c3 * c3).all()) and math.isfinite(GC.exact64(GC.family_c())[0])
    assert len(GC.family_d()) == 15 and len(GC.many_tensors()) == 70
    assert [al for _, _, al in GC.family_a()].count(False) == 1           # the element path: "offset"
    parts = GC.ref_partials(GC.family_a())
    assert parts.shape == (6, 256, 2) and parts[0, :, 0].all() and not parts[1, 1:].any()


def test_guarded_update_restatement():
    """skip: nothing moves; coefficient 1: adam_multi_kernel's emulation; a coefficient: the same on the fp32 product"""
    g = torch.Generator().manual_seed(3)
    p, grad, m, v = (torch.randn(37, generator=g) for _ in range(4))
    v = v.abs()
    st = GC.ref_finish(GC.spread(1, 1, [4.0]), GC.new_state(1.0, step=2, good=2), 0.0, 2000, 2.0 ** 24, 0)
    assert st[GC.G["COEF"]] == 1.0 and st[GC.G["STEP"]] == 3.0
    for got, want in zip(GC.ref_guarded_adam(p, grad, m, v, st), E.emul_adam(p, grad, m, v, 3)):
        assert torch.equal(got, want)
    st = GC.ref_finish(GC.spread(1, 1, [4.0]), GC.new_state(1.0, step=2, good=2), 0.5, 2000, 2.0 ** 24, 0)
    coef = torch.tensor(st[GC.G["COEF"]]).float()
    assert 0.0 < float(coef) < 1.0
    for got, want in zip(GC.ref_guarded_adam(p, grad, m, v, st), E.emul_adam(p, grad * coef, m, v, 3)):
        assert torch.equal(got, want)
    st = GC.ref_finish(GC.spread(1, 1, [4.0], bad_at=(0,)), GC.new_state(1.0, step=2, good=2), 0.5, 2000, 2.0 ** 24, 0)
    out = GC.ref_guarded_adam(p, grad, m, v, st)
    assert out[0] is p and out[1] is m and out[2] is v and st[GC.G["STEP"]] == 2.0


def test_argument_validation_without_launch():
    from speech_decoding_amd import lib
    L = lib.load()
    buf = (ctypes.c_double * 64)()
    ptr = ctypes.addressof(buf)                                     # a non-null pointer no refused call may follow
    assert L.sda_grad_guard_parts(3, 5000) == 2 * 3 * 5 and L.sda_grad_guard_parts(60, 10 ** 7) == 2 * 60 * 256
    for n, max_n in ((0, 1), (1, 0), (-1, 5)):
        assert L.sda_grad_guard_parts(n, max_n) == -1
    for args in ((None, 1, 1, ptr), (ptr, 1, 1, None), (ptr, 0, 1, ptr), (ptr, 1, 0, ptr)):
        assert L.sda_grad_sumsq_multi(*args, None) == -1
        assert b"grad_sumsq_multi" in L.sda_last_error()
    ok = dict(partials=ptr, n=1, gx=1, state=ptr, max_norm=1.0, beta1=0.9, beta2=0.999, growth_interval=2000, max_scale=2.0 ** 24, dynamic=1)
    for bad in (dict(partials=None), dict(state=None), dict(n=0), dict(gx=0), dict(growth_interval=-1), dict(max_norm=math.nan),
                dict(max_scale=0.5)):
        assert L.sda_grad_guard_finish(*{**ok, **bad}.values(), None) == -1, bad
        assert b"grad_guard_finish" in L.sda_last_error()
    for args in ((None, 1, 1, ptr), (ptr, 1, 1, None), (ptr, 0, 1, ptr), (ptr, 1, 0, ptr)):
        assert L.sda_adam_multi_guarded(args[0], args[1], args[2], 1e-3, 0.9, 0.999, 1e-8, args[3], None) == -1
        assert b"adam_multi_guarded" in L.sda_last_error()
    assert lib.GUARD_STATE == 16 and len({v for k, v in lib.CONSTANTS.items() if k.startswith("GUARD_")}) == 12


def test_train_run_refuses_an_unknown_fp16_guard():
    import train
    from speech_decoding_amd.config import Config
    with pytest.raises(ValueError, match="fp16_guard=gpu"):
        train.run(Config(fp16_guard="gpu"))
    assert train.guard_mode(Config()) == (False, None)
    assert train.guard_mode(Config(fp16_guard="device")) == (True, None)
    assert train.guard_mode(Config(max_grad_norm=1)) == (True, 1.0)
