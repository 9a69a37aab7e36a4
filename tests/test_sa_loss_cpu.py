"""What tests/test_sa_loss_gpu.py relies on, shown without a GPU:
1. the shapes of tests/sa_loss_cases.py reach the edges they are named for (recomputed from the kernels' own constants);
2. the constants of its tolerance table are 4 x what the fp32 emulations measure against float64;
3. the unmutated emulation of every kernel passes every case with the GPU test's own check_*() functions, and each of the 20
   planted bugs misses a tolerance by 10 x or more (inf: an exact comparison failed, or NaN) on the case recorded next to it;
4. host-side refusals: bad arguments return -1 with sda_last_error set before anything is launched (the pointers passed are
   host memory)."""
import ctypes
import functools
import math

import pytest
import torch

from tests import sa_loss_cases as S

F32 = torch.float32
CAUGHT = {}          # mutant -> (case and check, ratio)

SA_MUTANTS = ("sa_drop_sensors_ge_256", "sa_drop_last_chunk", "sa_no_max_subtraction", "sa_mask_on_W", "sa_dot_without_mask",
              "sa_dz_re_im_swapped", "sa_backward_drop_m_ge_256", "sa_da_pads_unwritten")
CLIP_MUTANTS = ("clip_delta_at_i_eq_j", "clip_diag_not_zeroed", "clip_tie_rule_gt_only", "clip_tie_rule_local_index",
                "clip_row_lse_local_index", "clip_ymax_over_block_rows", "clip_zmax_over_local_zsq", "clip_gy_map_without_gap",
                "clip_gy_zero_row_unwritten", "clip_part_of_extra_block_written", "clip_finish_ignores_row0", "clip_lse_without_max")


@pytest.fixture(scope="module", autouse=True)
def _report():
    yield
    print("\nmutant -> case and check that catch it (error / tolerance; inf = an exact comparison failed or NaN)")
    for m, (case, r) in sorted(CAUGHT.items()):
        print(f"  {m:34s} {case:72s} {r:.3g}")


@functools.lru_cache(None)
def sa_case(*key):
    return S.sa_case(*key)


@functools.lru_cache(None)
def clip_case(*key):
    c = S.clip_case(*key)
    c["ranks"] = S.ranks_ref(c)
    return c


def sa_cases():
    for D1, K2, C, gemm in S.SA_SHAPES:
        for regime in S.SA_REGIMES:
            for mk in S.SA_MASKS:
                yield sa_case(D1, K2, C, regime, mk), gemm


def clip_cases():
    for shape in S.CLIP_SHAPES:
        for regime in S.CLIP_REGIMES:
            yield clip_case(*shape, regime)


def sa_run(case, gemm, dtype, hw=0, mutant=None):
    """every SpatialAttention check on the emulation: {check: error / tolerance}"""
    C = case["C"]
    ref = S.sa_forward_ref(case, gemm)
    out = {}
    fwd = S.emul_softmax_pack(S.emul_sa_scores(case, mutant), case, dtype, hw, mutant)
    out.update({"forward " + k: v for k, v in S.check_sa_forward(case, dtype, *fwd, ref["W"], ref["tol_W"]).items()})
    a32 = ref["a"].float()
    W2 = torch.softmax(a32.double(), 1)
    pack = S.emul_softmax_pack(a32, case, dtype, hw, mutant)
    out.update({"softmax_pack " + k: v for k, v in S.check_sa_forward(case, dtype, *pack, W2, S.sm_tol(a32.double(), W2, C)).items()})
    W32 = ref["W"].float()
    bref = S.sa_backward_ref(case, W32, gemm)
    out.update({"backward " + k: v for k, v in S.check_sa_backward(case, S.emul_sa_backward(case, W32, mutant), bref).items()})
    da = S.emul_sa_softmax_backward(case, W32, S.pad64(C), mutant)
    out.update({"softmax_backward " + k: v for k, v in S.check_sa_softmax_backward(case, da, bref).items()})
    return out


def clip_run(c, dtype, hw=0, mutant=None):
    out = {}
    out.update({"logits_stats " + k: v for k, v in S.check_logits_stats(c, *S.emul_logits_stats(c, hw, mutant)).items()})
    out.update({"grad " + k: v for k, v in S.check_clip_grad(c, dtype, *S.emul_clip_grad(c, dtype, hw, mutant)).items()})
    out.update({"grad_y " + k: v for k, v in S.check_clip_grad_y(c, dtype, *S.emul_clip_grad_y(c, dtype, hw, mutant)).items()})
    part32, row0, nrows = S.finish_case(c)
    fin = S.emul_clip_grad_y_finish(c, part32, row0, nrows, hw, mutant)
    out.update({"finish " + k: v for k, v in S.check_clip_grad_y_finish(c, part32, row0, nrows, *fin).items()})
    out["ranks equal"] = S.exact(torch.equal(S.emul_ranks(c, mutant), c["ranks"]))
    return out


def worst(d):
    k = max(d, key=lambda k: d[k])
    return k, d[k]


# ---------------------------------------------------------------------------------------------------------------
# 1. geometry
# ---------------------------------------------------------------------------------------------------------------
def test_shapes_reach_the_edges_they_are_named_for():
    sa = S.SA_SHAPES
    assert {s[0] for s in sa} == {1, S.SA_R, S.SA_R + 1, 20} and 20 % S.SA_R != 0
    alone = {s[1] for s in sa if not s[3]}
    assert alone == {1, 36, S.SA_MC, S.SA_MC + 1, 257}
    chunks = lambda K2: (K2 + S.SA_MC - 1) // S.SA_MC
    assert chunks(36) == 1 and chunks(S.SA_MC) == 1 and chunks(S.SA_MC + 1) == 2 and chunks(257) == 3
    assert (257 + 255) // 256 == 2 and 257 - 256 == 1                    # backward: a second blockIdx.y with one live thread
    matrix = {s[1] for s in sa if s[3]}
    assert matrix == {32, 1024} and all((2 * K2) % 64 == 0 for K2 in matrix)
    assert {s[2] for s in sa} == {1, 60, 208, 256, 257, 306, 512}
    assert {s[2] for s in sa if s[3]} >= {208, 306, 512}                 # the matrix path below and above 256 sensors and at the cap
    assert any(s[1] > 256 and s[2] > 256 for s in sa if not s[3])        # second pass of da[r][c] together with the second m block
    assert max(s[0] * s[1] * s[2] for s in sa) <= 20 * 1024 * 512
    assert S.CLIP_SHAPES == ((1, 1, 0), (3, 3, 0), (64, 64, 0), (255, 255, 0), (257, 257, 0), (300, 300, 0), (513, 70, 140),
                             (140, 70, 70), (15, 5, 10), (512, 256, 256))
    assert {Bn % 64 for _, Bn, _ in S.CLIP_SHAPES} >= {0, 1, 5, 6, 63}
    assert any(Bm > 256 and Bn < 256 for Bm, Bn, _ in S.CLIP_SHAPES) and any(Bn > 256 for _, Bn, _ in S.CLIP_SHAPES)
    assert any(col0 + Bn == Bm and col0 > 0 for Bm, Bn, col0 in S.CLIP_SHAPES)     # the last column block of a larger batch
    for Bm, Bn, col0 in S.CLIP_SHAPES:
        seg, seg_pitch, groups = S.gy_layout(Bm, Bn, col0)
        assert 0 <= col0 and col0 + Bn <= Bm and max(Bm, Bn) <= 513
        assert seg_pitch % 64 == 0 and seg_pitch >= seg and groups * seg >= Bm     # what sda_clip_grad_y accepts
        if Bm == Bn:
            assert (seg, seg_pitch, groups) == (Bm, S.pad64(Bm), 1)
    assert S.gy_layout(15, 5, 10) == (5, 64, 3) and S.gy_layout(140, 70, 70) == (70, 128, 2) and S.gy_layout(512, 256, 256) == (256, 256, 2)


def test_regimes_are_what_they_are_named():
    for D1, K2, C, gemm in S.SA_SHAPES:
        a = S.sa_forward_ref(sa_case(D1, K2, C, "saturated", "none"), gemm)["a"]
        assert 69.0 <= float(a.amax(1).abs().min()) and float(a.amax(1).abs().max()) <= 96.0 and float(a.abs().max()) < 160
        if D1 >= 2:
            assert float(a.amax()) > 88.73                                                           # past fp32 exp's overflow threshold
        if C >= 60:
            W = torch.softmax(a, 1)
            # a good share of the exp underflow (below fp32's smallest normal, some below its smallest subnormal) and two sensors carry the row
            assert float((W < S.FTZ).float().mean()) > 0.2 and float(W.topk(2, dim=1).values.sum(1).min()) > 0.7
            assert float((a.amax(1) - a.amin(1)).max()) > 104
        a1 = S.sa_forward_ref(sa_case(D1, K2, C, "o1", "none"), gemm)["a"]
        assert float(a1.abs().max()) < 12
    for Bm, Bn, col0 in S.CLIP_SHAPES:
        hot, sat, tr = clip_case(Bm, Bn, col0, "hot"), clip_case(Bm, Bn, col0, "saturated"), clip_case(Bm, Bn, col0, "trained")
        assert float(hot["logits"].abs().max()) > 1000
        jj = torch.arange(Bn)
        assert bool((sat["logits"][col0 + jj, jj] > 150).all())
        if Bn >= 64:
            p = torch.exp(tr["logits"].double() - tr["row_lse"].double()[:, None])[col0 + jj, jj]
            assert 0.001 < float(p.mean()) < 0.9                                                     # neither flat nor saturated
        nrm = clip_case(Bm, Bn, col0, "norms")
        if Bm >= 64:
            assert float(nrm["ysq"].max() / nrm["ysq"].min()) >= 2.0 ** 16 and float(nrm["zsq_all"].max() / nrm["zsq_all"].min()) >= 2.0 ** 16
            G = S.clip_grad_ref(nrm, torch.float16)["G"]
            assert float(G.abs().max()) < 65504 / 8
        if Bm > Bn:                                                                                  # the maxima lie outside the block
            assert int(tr["ysq"].argmax()) not in range(col0, col0 + Bn) and int(tr["zsq_all"].argmax()) not in range(col0, col0 + Bn)
            assert float(tr["zsq_all"].max()) > float(tr["zsq"].max())
            assert int((~tr["inb"]).sum()) == Bm - Bn
        ties = clip_case(Bm, Bn, col0, "ties")
        if Bn >= 2:
            l = ties["logits"]
            assert torch.equal(l[:, 0], l[:, Bn - 1])
            # the positive's equal lies on either side of i, and the rule counts it on one side only
            assert int(ties["ranks"][col0 + Bn - 1]) == int((l[col0 + Bn - 1] > l[col0 + Bn - 1, 0]).sum()) + 1
            assert int(ties["ranks"][col0]) == int((l[col0] > l[col0, 0]).sum())
        if Bm >= 3:
            assert torch.equal(ties["logits"][1], ties["logits"][Bm - 1])


# ---------------------------------------------------------------------------------------------------------------
# 2. the tolerance table
# ---------------------------------------------------------------------------------------------------------------
def test_tolerance_table_matches_the_emulation():
    """chosen constant = 4 x measured, rounded up by at most a quarter"""
    m = S.measure_constants([sa_case(D1, K2, C, r, "none") for D1, K2, C, _ in S.SA_SHAPES for r in S.SA_REGIMES], list(clip_cases()))
    chosen = dict(C_SM=S.C_SM, C_LOGIT=S.C_LOGIT, C_LSE=S.C_LSE, C_D=S.C_D)
    print("\nmeasured on the CPU (fp32 emulation against float64, exp moved by -1, 0, +1 ulp) and chosen:")
    for k, v in m.items():
        unit = S.U32 if k in ("C_SM", "C_LOGIT") else 1.0
        print(f"  {k:8s} measured {v / unit:.3f}  chosen {chosen[k] / unit:.3f}")
    for k, v in m.items():
        assert 4.0 * v <= chosen[k] <= 5.0 * v, (k, v, chosen[k])


# ---------------------------------------------------------------------------------------------------------------
# 3. emulations and mutants
# ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", S.DTYPES, ids=str)
def test_sa_emulation_passes_every_case(dtype):
    for case, gemm in sa_cases():
        for hw in (S.HW if case["mask_kind"] == "dropped" else (0,)):
            k, r = worst(sa_run(case, gemm, dtype, hw))
            assert r <= 1.0, (case["name"], dtype, hw, k, r)


@pytest.mark.parametrize("dtype", S.DTYPES, ids=str)
def test_clip_emulation_passes_every_case(dtype):
    for c in clip_cases():
        for hw in S.HW:
            k, r = worst(clip_run(c, dtype, hw))
            assert r <= 1.0, (c["name"], dtype, hw, k, r)


def test_merge_emulation_passes():
    for name, allp in S.merge_cases().items():
        for hw in S.HW:
            k, r = worst(S.check_merge(allp, *S.emul_merge(allp, hw)))
            assert r <= 1.0, (name, hw, k, r)
    allp = S.merge_cases()["a rank with row_sum 0 at row_max -3e38"]
    assert bool(torch.isfinite(S.merge_ref(allp)[0]).all())


def _catch(mutant, runs):
    best = ("", 0.0)
    for name, run in runs:
        k, r = worst(run())
        if r > best[1]:
            best = (f"{name}: {k}", r)
        if r == math.inf:
            break
    assert best[1] >= 10.0, (mutant, best)
    CAUGHT[mutant] = best


@pytest.mark.parametrize("mutant", SA_MUTANTS)
def test_sa_mutants_miss_a_tolerance(mutant):
    _catch(mutant, ((case["name"], functools.partial(sa_run, case, gemm, F32, 0, mutant)) for case, gemm in sa_cases()))


@pytest.mark.parametrize("mutant", CLIP_MUTANTS)
def test_clip_mutants_miss_a_tolerance(mutant):
    _catch(mutant, ((c["name"], functools.partial(clip_run, c, F32, 0, mutant)) for c in clip_cases()))


def test_every_mutant_of_the_issue_is_recorded():
    """20 planted bugs, each caught at least once above (run on its own, this test runs the mutant tests first)"""
    want = set(SA_MUTANTS) | set(CLIP_MUTANTS)
    for m in SA_MUTANTS:
        if m not in CAUGHT:
            test_sa_mutants_miss_a_tolerance(m)
    for m in CLIP_MUTANTS:
        if m not in CAUGHT:
            test_clip_mutants_miss_a_tolerance(m)
    assert len(want) == 20 and want <= set(CAUGHT), want - set(CAUGHT)


# ---------------------------------------------------------------------------------------------------------------
# 4. host-side refusals
# ---------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def host():
    from speech_decoding_amd import lib
    Lb = lib.load()
    buf = (ctypes.c_char * (1 << 16))()                               # host memory that no kernel may ever see
    p = (ctypes.cast(buf, ctypes.c_void_p).value + 15) // 16 * 16
    return lib, Lb, p, buf


def _refused(Lb, rc, msg, what):
    assert rc == -1, what
    assert msg in Lb.sda_last_error(), (what, Lb.sda_last_error())


def test_spatial_attention_refuses_bad_arguments_without_launch(host):
    lib, Lb, p, _ = host
    _refused(Lb, Lb.sda_sa_weights_forward(p, p, p, None, p, p, p, 8, 36, 513, 64, 576, lib.F32, None), b"sa_weights_forward: bad arguments", "C > 512")
    _refused(Lb, Lb.sda_sa_weights_forward(p, p, p, None, p, p, p, 8, 36, 60, 64, 64, 7, None), b"sa_weights_forward: unknown dtype", "dtype")
    _refused(Lb, Lb.sda_sa_weights_forward(p, p, p, None, p, p, p, 8, 36, 70, 64, 64, lib.F32, None), b"sa_weights_forward: bad arguments", "C > Cp")
    _refused(Lb, Lb.sda_sa_softmax_pack(p, 576, None, p, p, 8, 513, 64, 576, lib.BF16, None), b"sa_softmax_pack: bad arguments", "C > 512")
    _refused(Lb, Lb.sda_sa_softmax_pack(p, 59, None, p, p, 8, 60, 64, 64, lib.F16, None), b"sa_softmax_pack: bad arguments", "a_pitch < C")
    _refused(Lb, Lb.sda_sa_softmax_pack(p, 64, None, p, p, 8, 60, 64, 64, 3, None), b"sa_softmax_pack: unknown dtype", "dtype")
    _refused(Lb, Lb.sda_sa_weights_backward(p, p, None, p, p, p, 8, 36, 513, 576, None), b"sa_weights_backward: bad arguments", "C > 512")
    _refused(Lb, Lb.sda_sa_weights_backward(p, p, None, p, p, p, 8, 36, 70, 64, None), b"sa_weights_backward: bad arguments", "C > Cp")
    _refused(Lb, Lb.sda_sa_softmax_backward(p, 59, p, None, p, 64, 8, 60, None), b"sa_softmax_backward: bad arguments", "dwd_pitch < C")
    _refused(Lb, Lb.sda_sa_softmax_backward(p, 64, p, None, p, 59, 8, 60, None), b"sa_softmax_backward: bad arguments", "da_pitch < C")


def test_clip_tail_refuses_bad_arguments_without_launch(host):
    lib, Lb, p, _ = host
    grad = lambda col0, g_pitch, Bm, Bn, dt: Lb.sda_clip_grad(p, p, p, p, p, p, 0.5, col0, p, g_pitch, p, p, p, p, Bm, Bn, dt, None)
    _refused(Lb, grad(0, 63, 70, 70, lib.F32), b"clip_grad: null argument or g_pitch < Bn", "g_pitch < Bn")
    _refused(Lb, grad(0, 128, 70, 70, 5), b"clip_grad: unknown dtype", "dtype")
    for col0, Bm, Bn in ((-1, 70, 70), (1, 70, 70), (71, 140, 70), (0, 5, 6), (0, 0, 0), (0, 4, 0)):
        for dt in (lib.F32, lib.BF16, lib.F16):
            _refused(Lb, grad(col0, 128, Bm, Bn, dt), b"clip_grad: need Bm, Bn >= 1 and 0 <= col0, col0 + Bn <= Bm", (col0, Bm, Bn))
    stats = lambda s_pitch, Bm, Bn: Lb.sda_clip_logits_stats(p, s_pitch, p, p, p, p, p, p, p, p, p, Bm, Bn, 0, None)
    for s_pitch, Bm, Bn in ((69, 70, 70), (64, 0, 5), (64, 5, 0), (64, -1, 5)):
        _refused(Lb, stats(s_pitch, Bm, Bn), b"clip_logits_stats: bad arguments", (s_pitch, Bm, Bn))
    for Bm, Bn in ((0, 5), (5, 0), (-3, 5)):
        _refused(Lb, Lb.sda_clip_ranks(p, p, p, Bm, Bn, 0, None), b"clip_ranks: need Bm, Bn >= 1", (Bm, Bn))
    _refused(Lb, Lb.sda_clip_ranks(p, None, p, 5, 5, 0, None), b"clip_ranks: null argument", "null")
    _refused(Lb, Lb.sda_clip_grad_y(p, p, p, p, p, 5, 0, p, 64, 5, 64, p, 5, 5, 9, None), b"clip_grad_y: unknown dtype", "dtype")
