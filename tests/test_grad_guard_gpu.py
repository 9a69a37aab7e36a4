"""The gradient guard's three HIP launches on an MI355X, each on its own, held to tests/guard_cases.py's checks (the ones
tests/test_grad_guard_cpu.py shows to catch planted bugs), and GuardedAdam against FusedAdam bit for bit:
  norm pass     exact against float64 on integers, N 2^-52 on real values, a finite norm where fp32 squares overflow, a count of
                exactly 1 for one inf / NaN anywhere, the same bits twice, zeros from workgroups past a tensor's end
  finish        every branch of the rules == the restatement, on hand-made partials
  guarded Adam  coefficient 1: FusedAdam's bits over seven steps; clipping: FusedAdam fed torch's fp32 g * coef; a skipped step
                leaves no trace and does not count; state_dict round trip
Non-finite values are data here, as in tests/test_nonfinite_gpu.py: nothing faults."""
import math

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from tests import elementwise_cases as E      # noqa: E402
from tests import guard_cases as GC           # noqa: E402

DEV = "cuda:0"


def on_device(v, aligned):
    """flat fp32 -> device tensor at a 16-byte aligned address, or 4 bytes past one (the element path)"""
    if aligned:
        t = v.to(DEV)
        assert t.data_ptr() % 16 == 0
        return t
    base = torch.zeros(v.numel() + 1, device=DEV)
    base[1:] = v.to(DEV)
    assert base.data_ptr() % 16 == 0
    return base[1:]


def sumsq(case):
    from speech_decoding_amd import ops
    from speech_decoding_amd.optim import adam_table
    grads = [on_device(v, al) for _, v, al in GC.with_grad(case)]
    raw, max_n = adam_table([(g, g, g, g) for g in grads])            # only .grad, .n and .aligned are read
    table = ops.upload_small(raw, DEV)
    n = len(grads)
    parts = torch.full((ops.grad_guard_parts(n, max_n),), GC.SENT, dtype=torch.float64, device=DEV)
    ops.grad_sumsq_multi(table, n, max_n, parts)
    torch.cuda.synchronize()
    assert parts.numel() == 2 * n * GC.gx_of(max_n)
    return parts.cpu().numpy().reshape(n, -1, 2)


def finish(parts, state, max_norm, growth_interval, max_scale, dynamic):
    from speech_decoding_amd import ops
    p = torch.from_numpy(np.ascontiguousarray(parts, dtype=np.float64)).to(DEV)
    st = torch.from_numpy(np.array(state, dtype=np.float64)).to(DEV)
    ops.grad_guard_finish(p.reshape(-1), p.shape[0], p.shape[1], st, max_norm, GC.B1, GC.B2, growth_interval, max_scale, dynamic)
    torch.cuda.synchronize()
    return st.cpu().numpy()


def test_norm_pass():
    GC.check_norm_pass(sumsq)


def test_finish_rules():
    GC.check_finish(finish)


def test_coefficient_of_the_two_launches_together():
    GC.check_coef(sumsq, finish)


# ---------------------------------------------------------------------------------------------------------------
# GuardedAdam against FusedAdam
# ---------------------------------------------------------------------------------------------------------------
ADAM_NAMES = ("big", "three", "cplx", "offset", "never", "zero")


def _real(t):
    return torch.view_as_real(t) if t.is_complex() else t


def make_params(seed=43):
    """the parameter set of tests/test_elementwise_gpu.py::test_adam_against_float64_adam (without `late`: GuardedAdam has one
    step count), fresh tensors on every call, the same values"""
    _, shapes = E.adam_grads((), 0)
    g = torch.Generator().manual_seed(seed)
    P = {}
    for n in ADAM_NAMES:
        t = torch.randn(shapes[n], generator=g)
        if n == "cplx":
            P[n] = torch.nn.Parameter(torch.view_as_complex(t.contiguous()).to(DEV))
        elif n == "offset":
            P[n] = torch.nn.Parameter(on_device(t, False))
        else:
            P[n] = torch.nn.Parameter(t.to(DEV))
    assert P["offset"].data_ptr() % 16 == 4 and P["big"].numel() % 4 == 1
    return P


def set_grads(P, grads, k, factor=None, poison=None):
    for n, p in P.items():
        gk = grads[n][k]
        if gk is None:
            p.grad = None
            continue
        gk = gk.clone()
        if poison is not None and n == poison[0]:
            gk.reshape(-1)[poison[1]] = poison[2]
        gk = gk.to(DEV)
        if factor is not None:
            gk = gk * factor                                          # torch's fp32 multiply, on the device
        p.grad = torch.view_as_complex(gk.contiguous()) if n == "cplx" else gk


def bits(P, opt):
    torch.cuda.synchronize()
    out = {}
    for n, p in P.items():
        out[f"{n} param"] = _real(p.detach()).cpu().clone()
        for k in ("exp_avg", "exp_avg_sq"):
            if k in opt.state.get(p, {}):
                out[f"{n} {k}"] = _real(opt.state[p][k]).cpu().clone()
    return out


def differing(a, b):
    assert a.keys() == b.keys(), sorted(set(a) ^ set(b))
    return [k for k in a if not torch.equal(a[k].reshape(-1).view(torch.int32), b[k].reshape(-1).view(torch.int32))]


def test_coefficient_one_is_fused_adam_bit_for_bit():
    from speech_decoding_amd.optim import FusedAdam, GuardedAdam
    grads, _ = E.adam_grads(ADAM_NAMES, 7)
    P, R = make_params(), make_params()
    opt, ref = GuardedAdam(P.values(), lr=1e-3), FusedAdam(R.values(), lr=1e-3)
    start = bits(P, opt)
    for k in range(7):
        set_grads(P, grads, k)
        set_grads(R, grads, k)
        opt.step()
        ref.step()
        assert differing(bits(P, opt), bits(R, ref)) == [], f"step {k + 1}"
        assert opt.last_coef == 1.0 and opt.steps_taken == k + 1 and opt.skipped_steps == 0 and opt.loss_scale == 1.0
    assert torch.equal(bits(P, opt)["never param"], start["never param"]) and P["never"] not in opt.state
    assert torch.equal(bits(P, opt)["zero param"], start["zero param"])
    s, _, _ = GC.exact64([(n, None if grads[n][6] is None else grads[n][6].reshape(-1), True) for n in ADAM_NAMES])
    assert abs(opt.last_grad_norm - math.sqrt(s)) <= 1e-9 * math.sqrt(s)


def test_clipping_is_fused_adam_on_the_fp32_product():
    from speech_decoding_amd.optim import FusedAdam, GuardedAdam
    grads, _ = E.adam_grads(ADAM_NAMES, 3)
    P, R = make_params(), make_params()
    opt, ref = GuardedAdam(P.values(), lr=1e-3, max_grad_norm=1e11, loss_scale=4.0), FusedAdam(R.values(), lr=1e-3)
    for k in range(3):
        set_grads(P, grads, k)
        opt.step()
        coef, norm = opt.last_coef, opt.last_grad_norm
        s, _, _ = GC.exact64([(n, None if grads[n][k] is None else grads[n][k].reshape(-1), True) for n in ADAM_NAMES])
        assert norm > 1e11 and abs(norm - math.sqrt(s) / 4.0) <= 1e-9 * norm        # (the cplx tensor's 1e12 entries; scale 4)
        assert coef == 0.25 * (1e11 / (norm + 1e-6))
        set_grads(R, grads, k, factor=torch.tensor(coef, dtype=torch.float64).float().to(DEV))
        ref.step()
        assert differing(bits(P, opt), bits(R, ref)) == [], f"step {k + 1}"
        # .grad is left as backward wrote it
        assert torch.equal(P["big"].grad.cpu(), grads["big"][k])


@pytest.mark.parametrize("bad", GC.POISON, ids=["+inf", "-inf", "nan"])
def test_a_skipped_step_leaves_no_trace_and_does_not_count(bad):
    from speech_decoding_amd.optim import FusedAdam, GuardedAdam
    grads, _ = E.adam_grads(ADAM_NAMES, 4)
    P, R = make_params(), make_params()
    opt = GuardedAdam(P.values(), lr=1e-3, loss_scale=8.0, dynamic=True, growth_interval=3)
    ref = FusedAdam(R.values(), lr=1e-3)                               # the twin never sees the poisoned step
    for k in (0, 1):
        set_grads(P, grads, k, factor=8.0)                            # a power-of-two scale and its un-scaling are exact
        set_grads(R, grads, k)
        opt.step()
        ref.step()
    before = bits(P, opt)
    assert differing(before, bits(R, ref)) == []
    set_grads(P, grads, 2, factor=8.0, poison=("cplx", 2 * 17 + 1, bad))
    opt.step()
    assert differing(bits(P, opt), before) == [], "a skipped step moved a parameter or a moment"
    assert (opt.steps_taken, opt.skipped_steps, opt.loss_scale, opt.last_coef) == (2, 1, 4.0, 0.0) and not math.isfinite(opt.last_grad_norm)
    set_grads(P, grads, 3, factor=4.0)
    set_grads(R, grads, 3)
    opt.step()
    ref.step()
    assert differing(bits(P, opt), bits(R, ref)) == [], "the step after a skip: bias correction from the applied steps (3), scale 4"
    assert (opt.steps_taken, opt.skipped_steps, opt.loss_scale) == (3, 1, 4.0)
    for k in (0, 1):                                                  # GOOD restarted at the skip: 3 good steps in a row double
        set_grads(P, grads, k, factor=4.0)
        opt.step()
    assert (opt.steps_taken, opt.loss_scale) == (5, 8.0)


def test_state_dict_round_trip():
    from speech_decoding_amd.optim import GuardedAdam
    grads, _ = E.adam_grads(ADAM_NAMES, 3)
    kw = dict(lr=1e-3, max_grad_norm=1e11, loss_scale=2.0, dynamic=True, growth_interval=2)
    P = make_params()
    opt = GuardedAdam(P.values(), **kw)
    for k in (0, 1):
        set_grads(P, grads, k)
        opt.step()
    sd = opt.state_dict()
    guard = sd["guard"].cpu().clone()
    assert guard[GC.G["STEP"]] == 2 and guard[GC.G["SCALE"]] == 4.0
    Q = make_params()
    with torch.no_grad():
        for n in ADAM_NAMES:
            Q[n].copy_(P[n])
    twin = GuardedAdam(Q.values(), **kw)
    twin.load_state_dict(sd)
    assert differing(bits(P, opt), bits(Q, twin)) == []
    assert torch.equal(twin.state_dict()["guard"].cpu().view(torch.int64), guard.view(torch.int64))
    for o, X in ((opt, P), (twin, Q)):
        set_grads(X, grads, 2)
        o.step()
    assert differing(bits(P, opt), bits(Q, twin)) == []
    assert torch.equal(twin.state_dict()["guard"].cpu().view(torch.int64), opt.state_dict()["guard"].cpu().view(torch.int64))
    assert twin.steps_taken == 3


def test_scale_is_a_device_multiply_and_late_parameters_are_refused():
    from speech_decoding_amd import SdaError
    from speech_decoding_amd.optim import GuardedAdam
    a, b = torch.nn.Parameter(torch.ones(5, device=DEV)), torch.nn.Parameter(torch.ones(3, device=DEV))
    opt = GuardedAdam([a, b], lr=1e-3, loss_scale=1024.0, dynamic=True)
    loss = torch.tensor(0.375, device=DEV)
    scaled = opt.scale(loss)
    assert scaled.dtype == torch.float32 and scaled.is_cuda and float(scaled) == 384.0
    assert opt.max_scale == 2.0 ** 24 and GuardedAdam([a], loss_scale=2.0 ** 25).max_scale == 2.0 ** 25
    a.grad = torch.ones(5, device=DEV)
    opt.step()
    b.grad = torch.ones(3, device=DEV)
    with pytest.raises(SdaError, match="first gradient after the first step"):
        opt.step()
