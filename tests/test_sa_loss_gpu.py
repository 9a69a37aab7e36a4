"""Kernel-level tests of csrc/sa_loss.hip on a real MI355X: the SpatialAttention weight build and its backward (stand-alone
kernels and the matrix path's soft-max halves) and the CLIP loss tail (logits and soft-max statistics, G, Gy and its finisher,
the loss scalars, the retrieval ranks, the cross-rank merge), each launched on its own — through its ops.* wrapper, and through
the C entry point where the test must own a sentinel-filled output buffer — and held to float64 on the fp32 inputs it is handed.
Inputs, references, tolerances (each with its derivation) and the check_*() functions are in tests/sa_loss_cases.py;
tests/test_sa_loss_cpu.py shows that these cases catch 20 planted bugs.

Edge -> test that launches it:
  m-chunks of sa_fwd_partial (1, 2, 3), both halves of sa_fwd_final's MAXC = 2, saturated / flat soft-max   test_sa_forward, test_sa_softmax_pack
  second 256-stride pass of da[r][c], second blockIdx.y of the backward, NaN padding of dWd                 test_sa_backward
  the matrix path (K2 = 32, 1024) and da's zero pad columns                                                 test_sa_forward, test_sa_backward
  blocks with col0 != 0, rows without a positive, large logits, saturated soft-max                          test_clip_logits_stats, test_clip_grad
  G's zero row and pad columns, ymax over every speech row, fp16 / bf16 with a norm ratio of 2^8            test_clip_grad
  segmented Gy layouts, Bn % 64 == 0 (the extra row block), zmax over zsq_all, stacked partials, row0 > 0   test_clip_grad_y, test_clip_grad_y_finish
  ties on either side of the positive, col0 != 0                                                            test_clip_ranks"""
import pytest
import torch

from tests import sa_loss_cases as S

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
F32 = torch.float32
WORST = {}                   # (kernel, dtype) -> max error / tolerance, printed when the module is done
_CASES = {}


@pytest.fixture(scope="module")
def ops():
    from speech_decoding_amd import ops as _ops
    from speech_decoding_amd import lib
    lib.load()
    assert torch.cuda.is_available(), "these tests need the MI355X"
    yield _ops
    print("\nworst error / tolerance per kernel and dtype:")
    for (kern, dt), r in sorted(WORST.items(), key=lambda kv: (kv[0][0], str(kv[0][1]))):
        print(f"  {kern:34s} {str(dt):16s} {r:.3f}")


def clip_case(*key):
    """one reference per case, shared by the tests and left unchanged"""
    if key not in _CASES:
        _CASES[key] = S.clip_case(*key)
    return _CASES[key]


def hold(kern, dtype, name, checks):
    """every figure is recorded and printed before anything is asserted on it"""
    torch.cuda.synchronize()
    for k, r in checks.items():
        WORST[(kern, dtype)] = max(WORST.get((kern, dtype), 0.0), r)
        print(f"{kern} {dtype} {name} {k}: error / tolerance {r:.3f}")
    bad = {k: r for k, r in checks.items() if not r <= 1.0}
    assert not bad, (kern, dtype, name, bad)


def dev(t):
    return None if t is None else t.to(DEV).contiguous()


def ptr(t):
    return None if t is None else t.data_ptr()


def sent(shape, dtype=F32):
    return torch.full(shape, S.SENT, dtype=dtype, device=DEV)


def same(*pairs):
    """bit-equal repeats"""
    return S.exact(all(torch.equal(a, b) for a, b in pairs))


def code(ops, dtype):
    return ops.dt_code(dtype)


def check_rc(rc, what):
    from speech_decoding_amd import lib
    lib.check(rc, what)


# ---------------------------------------------------------------------------------------------------------------
# SpatialAttention
# ---------------------------------------------------------------------------------------------------------------
def sa_forward_own(ops, case, gemm, dtype, cos, sin, tab_f=None):
    """the forward into sentinel-filled buffers the test owns: W (D1 + 1, C), Wp (D1p, Cp)"""
    from speech_decoding_amd import lib
    D1, K2, C, D1p, Cp = case["D1"], case["K2"], case["C"], case["D1p"], case["Cp"]
    z, mask = dev(case["z"].reshape(D1, 2 * K2)), dev(case["mask"])
    W, Wp = sent((D1 + 1, C)), sent((D1p, Cp), dtype)
    if gemm:
        a = ops.matmul_nt_splitk(z, tab_f, D1, C, 2 * K2, 2 * K2)
        check_rc(lib.load().sda_sa_softmax_pack(ptr(a), a.shape[1], ptr(mask), ptr(W), ptr(Wp), D1, C, D1p, Cp, code(ops, dtype), ops._st()),
                 "sa_softmax_pack")
    else:
        scratch = torch.empty(lib.load().sda_sa_scratch_floats(D1, K2, C), dtype=F32, device=DEV)
        check_rc(lib.load().sda_sa_weights_forward(ptr(z), ptr(cos), ptr(sin), ptr(mask), ptr(W), ptr(Wp), ptr(scratch),
                                                   D1, K2, C, D1p, Cp, code(ops, dtype), ops._st()), "sa_weights_forward")
    return W, Wp


@pytest.mark.parametrize("dtype", S.DTYPES, ids=str)
@pytest.mark.parametrize("D1,K2,C,gemm", S.SA_SHAPES)
def test_sa_forward(ops, dtype, D1, K2, C, gemm):
    """z -> W, Wp on the stand-alone kernels or the matrix path, against float64 from the same fp32 z and tables"""
    kern = "sa_forward(matrix path)" if gemm else "sa_weights_forward"
    for regime in S.SA_REGIMES:
        for mk in S.SA_MASKS:
            case = S.sa_case(D1, K2, C, regime, mk)
            ref = S.sa_forward_ref(case, gemm)
            cos, sin = dev(case["cos"]), dev(case["sin"])
            tab_f = ops.sa_gemm_tables(cos, sin)[0] if gemm else None
            W, Wp = sa_forward_own(ops, case, gemm, dtype, cos, sin, tab_f)
            checks = S.check_sa_forward(case, dtype, W, Wp, ref["W"], ref["tol_W"])
            zc = torch.view_as_complex(dev(case["z"]))
            W2, Wp2 = ops.sa_weights_forward(zc, cos, sin, dev(case["mask"]), case["D1p"], case["Cp"], dtype, fwd_table=tab_f)
            checks["the wrapper gives the same bits"] = same((W2, W[:D1]), (Wp2[0, 0], Wp))
            hold(kern, dtype, case["name"], checks)


@pytest.mark.parametrize("dtype", S.DTYPES, ids=str)
@pytest.mark.parametrize("D1,K2,C,gemm", S.SA_SHAPES)
def test_sa_softmax_pack(ops, dtype, D1, K2, C, gemm):
    """sda_sa_softmax_pack on exact fp32 scores (pitch > C, NaN in the padding): the soft-max's own arithmetic"""
    from speech_decoding_amd import lib
    for regime in S.SA_REGIMES:
        for mk in S.SA_MASKS:
            case = S.sa_case(D1, K2, C, regime, mk)
            a32 = S.sa_forward_ref(case, gemm)["a"].float()
            Wr = torch.softmax(a32.double(), 1)
            pitch = S.pad64(C) + 64
            a = torch.full((D1, pitch), float("nan"))
            a[:, :C] = a32
            a, mask = dev(a), dev(case["mask"])
            outs = []
            for _ in range(2):
                W, Wp = sent((D1 + 1, C)), sent((case["D1p"], case["Cp"]), dtype)
                check_rc(lib.load().sda_sa_softmax_pack(ptr(a), pitch, ptr(mask), ptr(W), ptr(Wp), D1, C, case["D1p"], case["Cp"], code(ops, dtype),
                                                        ops._st()), "sa_softmax_pack")
                outs.append((W, Wp))
            checks = S.check_sa_forward(case, dtype, *outs[0], Wr, S.sm_tol(a32.double(), Wr, C))
            checks["two calls give the same bits"] = same((outs[0][0], outs[1][0]), (outs[0][1], outs[1][1]))
            hold("sa_softmax_pack", dtype, case["name"], checks)


@pytest.mark.parametrize("D1,K2,C,gemm", S.SA_SHAPES)
def test_sa_backward(ops, D1, K2, C, gemm):
    """(dWd, W) -> dz and da; dWd has a pitch > C, NaN in its pad columns and in its rows >= D1"""
    from speech_decoding_amd import lib
    for regime in S.SA_REGIMES:
        for mk in S.SA_MASKS:
            case = S.sa_case(D1, K2, C, regime, mk)
            W32 = S.sa_forward_ref(case, gemm)["W"].float()
            ref = S.sa_backward_ref(case, W32, gemm)
            dWd, W, mask = dev(S.dwd_padded(case)), dev(W32), dev(case["mask"])
            cos, sin = dev(case["cos"]), dev(case["sin"])
            cosT, sinT = cos.t().contiguous(), sin.t().contiguous()
            Cq = S.pad64(C)
            das = []
            for _ in range(2):
                da = sent((D1 + 1, Cq))
                check_rc(lib.load().sda_sa_softmax_backward(ptr(dWd), dWd.shape[1], ptr(W), ptr(mask), ptr(da), Cq, D1, C, ops._st()),
                         "sa_softmax_backward")
                das.append(da)
            checks = S.check_sa_softmax_backward(case, das[0], ref)
            checks["two calls give the same bits"] = same((das[0], das[1]))
            hold("sa_softmax_backward", F32, case["name"], checks)
            tab_b = ops.sa_gemm_tables(cos, sin)[1] if gemm else None
            dz1 = torch.view_as_real(ops.sa_weights_backward(dWd, W, mask, cosT, sinT, K2, bwd_table=tab_b))
            dz2 = torch.view_as_real(ops.sa_weights_backward(dWd, W, mask, cosT, sinT, K2, bwd_table=tab_b))
            dz = sent((D1 + 1, K2, 2))
            if gemm:
                dz[:D1] = dz1
            else:
                check_rc(lib.load().sda_sa_weights_backward(ptr(dWd), ptr(W), ptr(mask), ptr(cosT), ptr(sinT), ptr(dz), D1, K2, C, dWd.shape[1],
                                                            ops._st()), "sa_weights_backward")
            checks = S.check_sa_backward(case, dz, ref)
            checks["two calls give the same bits"] = same((dz1, dz2), (dz1, dz[:D1]))
            hold("sa_backward(matrix path)" if gemm else "sa_weights_backward", F32, case["name"], checks)


# ---------------------------------------------------------------------------------------------------------------
# CLIP tail
# ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("Bm,Bn,col0", S.CLIP_SHAPES)
def test_clip_logits_stats(ops, Bm, Bn, col0):
    from speech_decoding_amd import lib
    for regime in S.CLIP_REGIMES:
        c = clip_case(Bm, Bn, col0, regime)
        Sd, ysq, zsq, temp = dev(c["S"]), dev(c["ysq"]), dev(c["zsq"]), dev(c["temp"])
        logits, st3, col_lse, row_lse = sent((Bm, Bn)), sent((3, Bm)), sent((Bn,)), sent((Bm,))
        check_rc(lib.load().sda_clip_logits_stats(ptr(Sd), Sd.shape[1], ptr(ysq), ptr(zsq), ptr(temp), ptr(logits), ptr(st3[0]), ptr(st3[1]),
                                                  ptr(col_lse), ptr(st3[2]), ptr(row_lse), Bm, Bn, col0, ops._st()), "clip_logits_stats")
        checks = S.check_logits_stats(c, logits, st3[0], st3[1], col_lse, st3[2], row_lse)
        w = ops.clip_logits_stats(Sd, ysq, zsq, temp, Bm, Bn, col0)
        checks["the wrapper gives the same bits"] = same(*zip(w, (logits, st3[0], st3[1], col_lse, st3[2], row_lse)))
        hold("clip_logits_stats", F32, c["name"], checks)


@pytest.mark.parametrize("dtype", S.DTYPES, ids=str)
@pytest.mark.parametrize("Bm,Bn,col0", S.CLIP_SHAPES)
def test_clip_grad(ops, dtype, Bm, Bn, col0):
    from speech_decoding_amd import lib
    for regime in S.CLIP_REGIMES:
        c = clip_case(Bm, Bn, col0, regime)
        ins = [dev(c[k]) for k in ("logits", "row_lse", "col_lse", "ysq", "zsq", "temp")]
        G = sent((Bm + 2, S.pad64(Bn)), dtype)
        rscale, cscale, colpart, scalars = sent((Bn,)), sent((Bn,)), sent((2 * Bn,)), sent((2,))
        check_rc(lib.load().sda_clip_grad(*map(ptr, ins), c["inv_norm"], col0, ptr(G), G.shape[1], ptr(rscale), ptr(cscale), ptr(colpart),
                                          ptr(scalars), Bm, Bn, code(ops, dtype), ops._st()), "clip_grad")
        checks = S.check_clip_grad(c, dtype, G, rscale, cscale, scalars)
        w = ops.clip_grad(*ins, c["inv_norm"], col0, dtype)
        checks["the wrapper gives the same bits"] = same(*zip(w, (G[:Bm + 1], rscale, cscale, scalars)))
        hold("clip_grad", dtype, c["name"], checks)


@pytest.mark.parametrize("dtype", S.DTYPES, ids=str)
@pytest.mark.parametrize("Bm,Bn,col0", S.CLIP_SHAPES)
def test_clip_grad_y(ops, dtype, Bm, Bn, col0):
    from speech_decoding_amd import lib
    seg, seg_pitch, groups = S.gy_layout(Bm, Bn, col0)
    for regime in S.CLIP_REGIMES:
        c = clip_case(Bm, Bn, col0, regime)
        ins = [dev(c[k]) for k in ("logits", "row_lse", "col_lse", "zsq", "zsq_all")]
        nparts = (Bn + 63) // 64
        Gy, part = sent((Bn + 2, groups * seg_pitch), dtype), sent((nparts + 1, Bm))
        check_rc(lib.load().sda_clip_grad_y(*map(ptr, ins), Bm, col0, ptr(Gy), Gy.shape[1], seg, seg_pitch, ptr(part), Bm, Bn, code(ops, dtype),
                                            ops._st()), "clip_grad_y")
        checks = S.check_clip_grad_y(c, dtype, Gy, part)
        w = ops.clip_grad_y(*ins, col0, dtype, seg=seg, seg_pitch=seg_pitch, groups=groups)
        checks["the wrapper gives the same bits"] = same((w[0], Gy[:Bn + 1]), (w[1], part[:nparts]))
        hold("clip_grad_y", dtype, c["name"], checks)


@pytest.mark.parametrize("Bm,Bn,col0", S.CLIP_SHAPES)
def test_clip_grad_y_finish(ops, Bm, Bn, col0):
    """the partials of every column block stacked in rank order (exact fp32 values), rows [row0, row0 + nrows) with row0 > 0"""
    for regime in S.CLIP_REGIMES:
        c = clip_case(Bm, Bn, col0, regime)
        part32, row0, nrows = S.finish_case(c)
        assert row0 > 0 or Bm == 1
        args = (dev(part32), dev(c["ysq"]), dev(c["zsq_all"]), dev(c["temp"]), c["inv_norm"], row0, nrows)
        r1, r2 = ops.clip_grad_y_finish(*args), ops.clip_grad_y_finish(*args)
        checks = S.check_clip_grad_y_finish(c, part32, row0, nrows, *r1)
        checks["two calls give the same bits"] = same(*zip(r1, r2))
        hold("clip_grad_y_finish", F32, c["name"], checks)


@pytest.mark.parametrize("Bm,Bn,col0", S.CLIP_SHAPES)
def test_clip_ranks(ops, Bm, Bn, col0):
    """the logits and the positives' logits are handed in: the counts are exact, ties by the global index rule"""
    for regime in S.CLIP_REGIMES:
        c = clip_case(Bm, Bn, col0, regime)
        cnt = ops.clip_ranks(dev(c["logits"]), dev(c["diag"]), col0)
        cnt2 = ops.clip_ranks(dev(c["logits"]), dev(c["diag"]), col0)
        hold("clip_ranks", F32, c["name"], {"counts equal": S.exact(torch.equal(cnt.cpu(), S.ranks_ref(c))), "two calls give the same bits": same((cnt, cnt2))})


def test_clip_merge_rows_edges(ops):
    for name, allp in S.merge_cases().items():
        lse, diag = ops.clip_merge_rows(dev(allp))
        hold("clip_merge_rows", F32, name, S.check_merge(allp, lse, diag))
