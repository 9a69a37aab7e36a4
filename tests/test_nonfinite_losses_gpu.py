"""inf / NaN propagation and containment of the loss kernels that came after tests/test_nonfinite_gpu.py, on a real MI355X: the
labelled CLIP tail (csrc/clip_labels.hip), SigmoidLoss's speech side and its mask mode (csrc/sigmoid_loss.hip), and the extra
negatives (csrc/clip_negatives.hip, the windowed form of csrc/sim_gemm.hip).  The cases — operands, named poison sites, values,
restatements, the sites the maths leaves out — are those of tests/nonfinite_cases.py (label_cases, sigmoid_cases, neg_cases,
dz_cases, sim_cases); tests/test_nonfinite_cpu.py shows that none of them passes vacuously and that the checks catch a masked
lse whose maximum skips NaN, a label mask applied by multiplication, a logaddexp on fmaxf / fminf, a saturating store, a column
sum that skips non-finite terms and a windows product that reads a row outside its window against a zero coefficient.  The
kernel-to-test table is in tests/test_nonfinite_gpu.py.

Every launch is a valid launch on valid addresses: poison goes into values only, never into labels, starts, sizes or pitches."""
import pytest
import torch

from tests import nonfinite_cases as N
from tests import sa_loss_cases as S

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
F32 = torch.float32


@pytest.fixture(scope="module")
def ops():
    from speech_decoding_amd import ops as _ops
    from speech_decoding_amd import lib
    lib.load()
    assert torch.cuda.is_available(), "these tests need the MI355X"
    return _ops


def host(t):
    torch.cuda.synchronize()
    return t.detach().cpu()


def dev(t, dtype=None):
    t = torch.as_tensor(t)
    return (t if dtype is None else t.to(dtype)).to(DEV).contiguous()


def ptr(t):
    return t.data_ptr()


def hold(case, run, seen=None):
    """one case of tests/nonfinite_cases.py through N.run_cases; -> the number of (site, value) launches checked"""
    return N.run_cases(case["kernel"], run, case["ref"], case["operands"], case["sites"], case["values"], case["what"], seen=seen,
                       unreached=case["unreached"], finite_clean=case["finite_clean"], structural=True)


def ids(v):
    return str(v)


# ---------------------------------------------------------------------------------------------------------------
# csrc/clip_labels.hip
# ---------------------------------------------------------------------------------------------------------------
def label_run(ops, case):
    from speech_decoding_amd import lib
    c = case["operands"]
    Bm, Bn, col0, mode, dtype = c["Bm"], c["Bn"], c["col0"], case["mode"], case["dtype"]
    lab, cnt = dev(c["labels"]), dev(c["counts"])
    rl, cl = ("row_lse_m", "col_lse_m") if mode == "mask" else ("row_lse", "col_lse")
    if case["kernel"] == "clip_logits_stats_masked":
        names = ("logits", "row_max", "row_sum", "col_lse", "diag", "row_lse")
        return lambda o: dict(zip(names, map(host, ops.clip_logits_stats_masked(dev(o["S"]), dev(o["ysq"]), dev(o["zsq"]), dev(o["temp"]), lab, Bm, Bn, col0))))
    if case["kernel"] == "clip_grad_labels":
        def run(o):                                     # the C entry point: colpart is a by-product the wrapper keeps to itself
            ins = [dev(o[k]) for k in ("logits", rl, cl, "ysq", "zsq", "temp")]
            G = torch.empty((Bm + 1, S.pad64(Bn)), dtype=dtype, device=DEV)
            rscale, cscale, colpart, scalars = (torch.empty(n, device=DEV) for n in (Bn, Bn, 2 * Bn, 2))
            lib.check(lib.load().sda_clip_grad_labels(*map(ptr, ins), ptr(lab), ptr(cnt), ops.clip_dup_code(mode), c["inv_norm"], col0, ptr(G),
                                                      G.shape[1], ptr(rscale), ptr(cscale), ptr(colpart), ptr(scalars), Bm, Bn, ops.dt_code(dtype),
                                                      ops._st()), "clip_grad_labels")
            return dict(G=host(G), rscale=host(rscale), cscale=host(cscale), colpart=host(colpart).reshape(Bn, 2), scalars=host(scalars))
        return run
    seg, seg_pitch, groups = S.gy_layout(Bm, Bn, col0)

    def run_y(o):
        ins = [dev(o[k]) for k in ("logits", rl, cl, "zsq", "zsq_all")]
        Gy, part = ops.clip_grad_y_labels(*ins, lab, cnt, mode, col0, dtype, seg=seg, seg_pitch=seg_pitch, groups=groups)
        return {"Gy": host(Gy), "part": host(part)}
    return run_y


@pytest.mark.parametrize("pattern", N.LOSS_PATTERNS)
@pytest.mark.parametrize("block", N.LOSS_BLOCKS, ids=ids)
def test_labelled_clip_kernels(ops, block, pattern):
    """sda_clip_logits_stats_masked (mask mode's statistics), sda_clip_grad_labels and sda_clip_grad_y_labels in both modes and
    the three storage types of G / Gy.  A poisoned S[i][j] or logit reaches what the unlabelled kernels let it reach — unless
    (i, j) is a repeat of column j's speech under mask: then nothing but the stored logits entry."""
    kernels = {}
    for case in N.label_cases(*block, pattern):
        kernels[case["kernel"]] = kernels.get(case["kernel"], 0) + hold(case, label_run(ops, case))
    assert set(kernels) == {"clip_logits_stats_masked", "clip_grad_labels", "clip_grad_y_labels"} and all(n >= 20 for n in kernels.values()), kernels


# ---------------------------------------------------------------------------------------------------------------
# csrc/sigmoid_loss.hip
# ---------------------------------------------------------------------------------------------------------------
def sigmoid_run(ops, case):
    c = case["operands"]
    Bm, Bn, col0, mode, dtype = c["Bm"], c["Bn"], c["col0"], case["mode"], case["dtype"]
    lab = dev(c["labels"])
    if case["kernel"] == "sigmoid_grad_y":
        seg, seg_pitch, groups = S.gy_layout(Bm, Bn, col0)

        def run_y(o):
            Gy, part = ops.sigmoid_grad_y(dev(o["a"]), dev(o["bias"]), dev(o["zsq"]), dev(o["zsq_all"]), col0, dtype, labels=lab, duplicates=mode,
                                          seg=seg, seg_pitch=seg_pitch, groups=groups)
            return {"Gy": host(Gy), "part": host(part)}
        return run_y

    def run(o):
        ysq, zsq, temp = dev(o["ysq"]), dev(o["zsq"]), dev(o["temp"])
        a, diag, G, part = ops.sigmoid_pairs(dev(o["S"]), ysq, zsq, temp, dev(o["bias"]), Bm, Bn, col0, dtype, labels=lab, duplicates=mode)
        rscale, cscale, scalars = ops.sigmoid_finish(part, ysq, zsq, temp, c["inv_norm"])
        return dict(a=host(a), diag=host(diag), G=host(G), part=host(part), rscale=host(rscale), cscale=host(cscale), scalars=host(scalars))
    return run


@pytest.mark.parametrize("pattern", N.LOSS_PATTERNS)
@pytest.mark.parametrize("block", N.LOSS_BLOCKS, ids=ids)
def test_sigmoid_loss_kernels(ops, block, pattern):
    """sda_sigmoid_grad_y with labels in both modes, sda_sigmoid_pairs + sda_sigmoid_finish in mask mode, fp32 and 16-bit G / Gy.
    Nothing couples the pairs: a poisoned a[i][j] reaches Gy[j][i] and row i's partial, a poisoned S[i][j] its own a, G entry, column
    j's sums and the three scalars; a dropped pair nothing but its own a."""
    kernels = {}
    for case in N.sigmoid_cases(*block, pattern):
        kernels[case["kernel"]] = kernels.get(case["kernel"], 0) + hold(case, sigmoid_run(ops, case))
    assert set(kernels) == {"sigmoid_grad_y", "sigmoid_pairs + sigmoid_finish"} and all(n >= 20 for n in kernels.values()), kernels


# ---------------------------------------------------------------------------------------------------------------
# csrc/clip_negatives.hip: the two scalar kernels
# ---------------------------------------------------------------------------------------------------------------
def neg_run(ops, case):
    from speech_decoding_amd import lib
    c = case["operands"]
    Bn, Nn, dtype = c["Bn"], c["N"], case["dtype"]
    if case["kernel"] == "clip_neg_stats":
        def run_s(o):
            col = dev(o["col_lse"]).clone()                  # merged in place
            mlog = ops.clip_neg_stats(dev(o["S"]), dev(o["wsq"]), dev(o["zsq"]), dev(o["temp"]), col, Bn, Nn)
            return {"mlog": host(mlog), "col_lse": host(col)}
        return run_s
    nr = ops.clip_neg_rows(Nn)

    def run(o):                                              # the C entry point: colpart is a by-product the wrapper keeps to itself
        ins = [dev(o[k]) for k in ("mlog", "col_lse_merged", "wsq", "zsq", "temp")]
        Gn = torch.full((nr, S.pad64(Bn)), S.SENT, dtype=dtype, device=DEV)
        cs, colpart = torch.empty(Bn, device=DEV), torch.empty(Bn, device=DEV)
        rscale, scalars = dev(o["rscale_in"]).clone(), dev(o["scalars_in"]).clone()      # added to in place
        lib.check(lib.load().sda_clip_neg_grad(*map(ptr, ins), c["inv_norm"], ptr(Gn), Gn.shape[1], ptr(cs), ptr(rscale), ptr(colpart), ptr(scalars),
                                               Bn, Nn, ops.dt_code(dtype), ops._st()), "clip_neg_grad")
        Gh = host(Gn)
        # the padding is an MFMA operand of clip_dz_windows: exact zeros whatever the poison (N.check holds it to the clean run's
        # bits; this says what those are)
        assert bool((Gh[Nn:] == 0).all()) and bool((Gh[:, Bn:] == 0).all()), (case["what"], "G^n's rows past N or pad columns are not zero")
        return {"Gn": Gh, "cscale_n": host(cs), "rscale": host(rscale), "scalars": host(scalars), "colpart": host(colpart)}
    return run


@pytest.mark.parametrize("shape", N.NEG_SHAPES, ids=ids)
def test_negatives_scalar_kernels(ops, shape):
    """sda_clip_neg_stats: a poisoned S[j][n] reaches m[j][n] and column j's merged lse; the incoming col_lse[j] its own merge.
    sda_clip_neg_grad: a poisoned m[j][n] reaches G^n[n][j], rscale[j], colpart[j] and d loss / d temp; the incoming rscale[j] and
    scalars[1] it adds to stay non-finite; G^n's rows N ... neg_rows(N) - 1 and pad columns are exact zeros whatever the poison."""
    kernels = {}
    for case in N.neg_cases(*shape):
        kernels[case["kernel"]] = kernels.get(case["kernel"], 0) + hold(case, neg_run(ops, case))
    assert set(kernels) == {"clip_neg_stats", "clip_neg_grad"} and all(n >= 15 for n in kernels.values()), kernels


# ---------------------------------------------------------------------------------------------------------------
# the windowed MFMA kernels: sda_clip_dz_windows, sda_sim_gemm_windows (and sda_sim_gemm beside it)
# ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("pattern", N.DZ_PATTERNS)
@pytest.mark.parametrize("shape", N.DZ_SHAPES, ids=ids)
def test_clip_dz_windows(ops, shape, pattern):
    """the whole row-layout buffer is the output (pad rows and slack included).  The K-steps past N re-read the last candidate's
    window against G^n's zero rows: whatever that makes non-finite, the last candidate's own term has made non-finite already,
    so the kernel needs no exception — a table element reaches exactly the dZ elements the restatement names, one in no window
    changes no bit."""
    for case in N.dz_cases(*shape, pattern):
        c, dtype = case["operands"], case["dtype"]
        Bn, Nn, T = c["Bn"], c["N"], c["T"]
        starts = dev(c["starts"])
        lo, hi = int(c["starts"].min()), int(c["starts"].max())
        typed = ("Gn", "table", "out")

        def run(o):
            out = dev(o["out"], dtype).clone()
            ops.clip_dz_windows(dev(o["Gn"], dtype), dev(o["table"], dtype), starts, lo, hi, out, dev(o["cscale"]), N=Nn, Bn=Bn, T=T,
                                out_scale=dev(o["out_scale"]))
            return {"dZ": host(out)}

        assert hold(case, run, seen=lambda o: {k: (S.q(v, dtype) if k in typed else v) for k, v in o.items()}) >= 24


@pytest.mark.parametrize("shape", N.SIM_SHAPES, ids=ids)
def test_sim_gemm_windows_and_sim_gemm(ops, shape):
    """S = X . windows^T at the kernel's own K split and at one slice, on the windowed kernel and on the plain one fed the same
    windows cut out.  The compared output is every stored element, the pad columns N ... pad64(N) - 1 included: rows past M and
    candidates past N are clamped reads whose results are not stored, or land in the pad columns as the repeat of the last real
    column that N.EXCEPTIONS["sim_gemm"] describes."""
    from speech_decoding_amd import lib as L
    from tests import clip_negative_cases as NC
    M, Nn = shape
    for case in N.sim_cases(M, Nn):
        c, dtype = case["operands"], case["dtype"]
        K, Fp, T, Np = c["K"], c["Fp"], c["T"], S.pad64(Nn)
        starts = dev(c["starts"])
        lo, hi = int(c["starts"].min()), int(c["starts"].max())
        chosen = L.load().sda_sim_gemm_ksplit(M, Nn, K, ops.dt_code(dtype))
        assert chosen > 1
        labels = [(kind, ks) for kind in ("windows", "plain") for ks in (chosen, 1)]

        def run(o):
            xm, table = dev(o["X"], dtype), dev(o["table"], dtype)
            wm = dev(NC.windows_of(o["table"], c["starts"], T), dtype)
            res = {}
            for kind, ks in labels:
                partial = torch.full((ks, M, Np), N.NAN, device=DEV)
                out = torch.full((M, Np), N.NAN, device=DEV)
                if kind == "windows":
                    ops.sim_gemm_windows_into(xm, K, table, starts, lo, hi, Fp, M, Nn, K, ks, partial, out)
                else:
                    ops.matmul_nt_splitk_into(xm, wm, M, Nn, K, K, True, ks, partial, out)
                res.update(N.split_pad(f"{kind}, ksplit {ks}", host(out), Nn, dim=1, pad=N.PAD_COLS))
            return res

        def ref(o, mutant=None):
            r = case["ref"](o)
            return {k.replace("S", f"{kind}, ksplit {ks}", 1): v for kind, ks in labels for k, v in r.items()}

        typed = ("X", "table")
        n = N.run_cases("sim_gemm", run, ref, c, case["sites"], case["values"], case["what"], unreached=case["unreached"], structural=True,
                        seen=lambda o: {k: (S.q(v, dtype) if k in typed else v) for k, v in o.items()})
        assert n >= 21
