"""CPU half of the kernel-level tests of the wav2vec 2.0 embedder's HIP kernels (csrc/w2v2.hip).

1. Sensitivity of the designed inputs of tests/test_w2v2_kernels_gpu.py, proven without a GPU: a torch emulation of
   attention_kernel's algorithm (tests/w2v2_cases.py) meets the GPU test's tolerance against the float64 reference on every
   attention case and compute dtype, and each of its five mutants (last key dropped, alpha forgotten, tail of V^T used,
   scale forgotten, head offset lost) misses that tolerance by at least 10x on at least one case.  The same for LayerNorm
   with a one-pass variance on the offset-mean rows.
2. Host-side refusals: bad arguments return -1 with sda_last_error set before anything is launched (the pointers passed
   are host memory, so a launch that slipped through would show)."""
import ctypes

import pytest
import torch

from tests import w2v2_cases as W
from tests.test_kernels_gpu import tol

MARGIN = 10.0


def _att_ratio(case, T, heads, dtype, mutant=None):
    _, qh, kh, vh = case
    qh, kh, vh = W.q(qh, dtype), W.q(kh, dtype), W.q(vh, dtype)
    ref = W.attention_ref(qh, kh, vh, 0.125)
    vt = W.q(W.vt_with_tail(vh, W.ceil64(T), W.TAIL), dtype)
    got = W.attention_emulation(qh, kh, vt, T, 0.125, dtype, mutant=mutant)
    return W.tol_ratio(got, ref, **tol(dtype)), got, (qh, kh, vh)


@pytest.mark.parametrize("dtype", W.DTYPES)
@pytest.mark.parametrize("heads", W.ATT_HEADS)
@pytest.mark.parametrize("T", W.ATT_T)
def test_attention_emulation_meets_the_gpu_tolerance_on_every_case(T, heads, dtype):
    for case in W.attention_cases(T, heads):
        ratio, got, (qh, kh, vh) = _att_ratio(case, T, heads, dtype)
        assert ratio <= 1.0, (case[0], ratio)
        zero_tail = W.attention_emulation(qh, kh, W.vt_with_tail(vh, W.ceil64(T), 0.0), T, 0.125, dtype)
        assert torch.equal(got, zero_tail), case[0]                  # masked probabilities are exactly zero


def test_designed_logits_are_exact_in_every_dtype():
    for dtype in W.DTYPES:
        for name, qh, kh, _ in W.attention_cases(200, 3):
            if name.startswith("e_"):
                continue
            assert torch.equal(W.q(qh, dtype), qh) and torch.equal(W.q(kh, dtype), kh), (name, dtype)
            s = (qh @ kh.transpose(1, 2)) * 0.125
            assert torch.equal(s, kh[:, None, :, 0].expand_as(s)), name
    a = W.attention_cases(200, 1)[0][2][0, :, 0]                      # the rising ramp: > 20 from each block to the next
    assert float(a[64:128].min() - a[:64].max()) > 20 and float(a[192:].min() - a[128:192].max()) > 20


@pytest.mark.parametrize("dtype", W.DTYPES)
@pytest.mark.parametrize("mutant", W.ATT_MUTANTS)
def test_every_attention_mutant_misses_the_tolerance_by_10x(mutant, dtype):
    worst, where = 0.0, None
    for T in W.ATT_T:
        for heads in W.ATT_HEADS:
            for case in W.attention_cases(T, heads):
                r = _att_ratio(case, T, heads, dtype, mutant)[0]
                if r > worst:
                    worst, where = r, (case[0], T, heads)
        if worst >= 1e3 * MARGIN:
            break
    assert worst >= MARGIN, (mutant, worst, where)


def test_each_attention_mutant_is_caught_by_the_case_designed_for_it():
    """bf16, the widest tolerance: the pairing of mutant and designed case that the GPU test relies on."""
    dtype = torch.bfloat16
    pairs = [("drop_tail_key", "c_last_key", 65, 1), ("drop_tail_key", "c_last_key", 200, 1), ("no_rescale", "a_rising", 129, 1),
             ("no_rescale", "a_rising", 200, 3), ("tail_v_used", "e_random_std1", 17, 1), ("tail_v_used", "a_rising", 129, 3),
             ("no_scale", "e_random_std1", 63, 1), ("head_shift", "f_per_head", 64, 3)]
    for mutant, name, T, heads in pairs:
        case = [c for c in W.attention_cases(T, heads) if c[0] == name][0]
        assert _att_ratio(case, T, heads, dtype, mutant)[0] >= MARGIN, (mutant, name, T, heads)
        assert _att_ratio(case, T, heads, dtype)[0] <= 1.0


@pytest.mark.parametrize("dtype", W.DTYPES)
def test_one_pass_layernorm_misses_the_tolerance_by_10x_on_offset_mean_rows(dtype):
    g = torch.Generator().manual_seed(3)
    worst = 0.0
    for C in (64, 1000, 1024, 2048):
        gamma, beta = 1.0 + 0.5 * torch.randn(C, generator=g), 0.3 * torch.randn(C, generator=g)
        for kind in ("std0.1", "near_constant") if C & (C - 1) == 0 else ("std0.1",):
            x = W.offset_mean_rows(5, C, kind)
            assert torch.equal(W.q(x, dtype), x)                      # representable: the kernel reads exactly these rows
            assert abs(float(x.mean()) - 100.0) < 0.01
            if kind == "std0.1" and C >= 1000:
                assert abs(float(x.double().std(dim=-1, unbiased=False).mean()) - 0.1) < 2e-3
            ref = W.layernorm_ref(x, gamma, beta)
            assert W.tol_ratio(W.layernorm_emulation(x, gamma, beta, dtype), ref, **tol(dtype)) <= 1.0, (C, kind)
            worst = max(worst, W.tol_ratio(W.layernorm_emulation(x, gamma, beta, dtype, variance="one_pass"), ref, **tol(dtype)))
    assert worst >= MARGIN, worst


# ---------------------------------------------------------------------------------------------------------------
# host-side refusals
# ---------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def host():
    from speech_decoding_amd import lib
    L = lib.load()
    buf = (ctypes.c_char * (1 << 16))()                               # host memory that no kernel may ever see
    p = (ctypes.cast(buf, ctypes.c_void_p).value + 15) // 16 * 16
    return lib, L, p, buf


def _refused(L, rc, msg, what):
    assert rc == -1, what
    assert msg in L.sda_last_error(), (what, L.sda_last_error())


def test_attention_refuses_bad_arguments_without_launch(host):
    lib, L, p, _ = host
    ok = dict(T=70, heads=2, head_dim=64, qk_pitch=256, vt_pitch=128, out_pitch=128, dtype=lib.BF16)

    def call(**kw):
        a = dict(ok, **kw)
        return L.sda_w2v_attention(p, p, p, p, a["T"], a["heads"], a["head_dim"], a["qk_pitch"], a["vt_pitch"], a["out_pitch"],
                                   0.125, a["dtype"], None)
    for kw in (dict(head_dim=32), dict(head_dim=128), dict(vt_pitch=64), dict(vt_pitch=120), dict(T=129, vt_pitch=128),
               dict(out_pitch=64), dict(out_pitch=127), dict(qk_pitch=252), dict(vt_pitch=132), dict(qk_pitch=258, dtype=lib.F32),
               dict(vt_pitch=130, dtype=lib.F32), dict(T=0), dict(heads=0)):
        _refused(L, call(**kw), b"w2v_attention: bad arguments", kw)
    for dt in (3, -1):
        _refused(L, call(dtype=dt), b"unknown dtype", dt)


def test_layernorm_refuses_bad_arguments_without_launch(host):
    lib, L, p, _ = host

    def call(T=4, C=64, Cp=64, dtype=lib.F32):
        return L.sda_layernorm_rows(p, p, p, p, T, C, Cp, 1e-5, 0, dtype, None)
    for kw in (dict(C=1030, Cp=1088), dict(C=65, Cp=64), dict(C=96, Cp=96), dict(C=2100, Cp=2112, dtype=lib.BF16),
               dict(C=2100, Cp=2112, dtype=lib.F16), dict(T=0), dict(C=0)):
        _refused(L, call(**kw), b"layernorm_rows: bad arguments", kw)
    _refused(L, call(dtype=3), b"unknown dtype", "dtype")


def test_conv0_refuses_bad_arguments_without_launch(host):
    lib, L, p, _ = host

    def call(T=5, C=64, Cp=64, K=10, stride=5, n=None, dtype=lib.F32):
        n = (T - 1) * stride + K if n is None else n
        return L.sda_w2v_conv0(p, n, p, None, p, p, p, T, C, Cp, K, stride, 1e-5, dtype, None)
    for kw in (dict(n=(5 - 1) * 5 + 10 - 1), dict(T=1, n=9), dict(C=1024, Cp=1024, K=17), dict(C=64, Cp=1088), dict(C=65, Cp=64),
               dict(C=64, Cp=96), dict(T=0), dict(K=0), dict(stride=0)):
        _refused(L, call(**kw), b"w2v_conv0: bad arguments", kw)
    for C in (64, 512, 1024):                                         # every NI branch refuses an unknown dtype
        _refused(L, call(C=C, Cp=C, dtype=7), b"unknown dtype", C)


def test_group_split_and_merge_refuse_bad_arguments_without_launch(host):
    lib, L, p, _ = host
    PAD = lib.ROW_PAD
    ok = dict(T=17, Hp=128, gw=32, gwp=64, G=4, rows=24 + 17, lead=24, dtype=lib.BF16)

    def split(**kw):
        a = dict(ok, **kw)
        return L.sda_w2v_group_split(p, p, a["T"], a["Hp"], a["gw"], a["gwp"], a["G"], a["rows"], a["lead"], a["dtype"], None)

    def merge(**kw):
        a = dict(ok, rows=PAD + 17)
        a.update(kw)
        return L.sda_w2v_group_merge_add(p, p, p, a["T"], a["Hp"], a["gw"], a["gwp"], a["G"], a["rows"], None, 0, a["dtype"], None)
    common = (dict(gw=4), dict(gw=28), dict(gw=6, dtype=lib.F32), dict(gw=4, dtype=lib.F16), dict(gwp=96), dict(gw=72), dict(G=5), dict(T=0))
    for kw in common + (dict(rows=24 + 16), dict(lead=-1)):
        _refused(L, split(**kw), b"w2v_group_split: bad arguments", kw)
    for kw in common + (dict(rows=PAD + 16),):
        _refused(L, merge(**kw), b"w2v_group_merge_add: bad arguments", kw)
    _refused(L, split(dtype=3), b"unknown dtype", "split")
    _refused(L, merge(dtype=3), b"unknown dtype", "merge")


def test_epilogue_and_mean4_refuse_bad_arguments_without_launch(host):
    lib, L, p, _ = host
    for kw in (dict(ksplit=0), dict(T=0), dict(Cp=96)):
        a = dict(dict(ksplit=2, T=3, Cp=64), **kw)
        _refused(L, L.sda_splitk_epilogue(p, a["ksplit"], None, None, p, a["T"], a["Cp"], 0, lib.F32, None), b"splitk_epilogue: bad arguments", kw)
    _refused(L, L.sda_splitk_epilogue(None, 2, None, None, p, 3, 64, 0, lib.F32, None), b"splitk_epilogue: bad arguments", "partial")
    _refused(L, L.sda_splitk_epilogue(p, 2, None, None, p, 3, 64, 0, 3, None), b"unknown dtype", "epilogue")
    for kw in (dict(T=0), dict(C=0), dict(C=65)):
        a = dict(dict(T=3, C=64, Cp=64), **kw)
        _refused(L, L.sda_w2v_mean4(p, p, p, p, p, a["T"], a["C"], a["Cp"], lib.F32, None), b"w2v_mean4: bad arguments", kw)
    _refused(L, L.sda_w2v_mean4(p, p, p, None, p, 3, 64, 64, lib.F32, None), b"w2v_mean4: bad arguments", "null")
    _refused(L, L.sda_w2v_mean4(p, p, p, p, p, 3, 64, 64, 3, None), b"unknown dtype", "mean4")
