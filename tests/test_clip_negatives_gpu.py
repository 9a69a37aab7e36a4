"""CLIPLoss with extra speech negatives read in place from resident tracks, on a real MI355X.

Per kernel: sda_clip_neg_stats, sda_clip_neg_grad and sda_clip_dz_windows launched on their own over the shapes, regimes and start
patterns of tests/clip_negative_cases.py — through the C entry point into sentinel-filled buffers the test owns and through the
ops.* wrapper — and held to float64 on the inputs they are handed, within that file's constants; sda_clip_dz_windows also exactly,
on small-integer operands (tests/test_exact_gpu.py's method).  tests/test_clip_negatives_cpu.py shows that these cases catch the
planted bugs.

Whole loss: CLIPLoss(x, y, negatives=bank) in bf16 and fp16 against float64 autograd of the two-line form on the operands as the
device sees them (loss, dZ, dY, dtemp), with and without labels, on the toy encoder's output, under two ranks; the bounds are the
project's.  Then bit identity without negatives, the reference's row offset through ops.gather_windows, the refusals
and train.py's clip_negatives option."""
import numpy as np
import pytest
import torch

from tests import builders as TB
from tests import clip_negative_cases as NC
from tests.parity import rel_l2
from tests.ranks import run_ranks

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
F32 = torch.float32
DT = {"bf16": torch.bfloat16, "fp16": torch.float16, "fp32": torch.float32}
GRAD_REL_L2 = {"bf16": 6e-2, "fp16": 8e-3}      # DESIGN §5, tests/test_clip_dy_gpu.py, tests/test_clip_labels_gpu.py
LOSS_REL = {"bf16": 1e-2, "fp16": 1e-2}
DTEMP = 1e-4                                    # x max(1, |dtemp|): dtemp is summed in fp32 from fp32 logits in every mode
WORST = {}
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


def case(maker, *key):
    """one reference per case, shared by the tests and left unchanged"""
    if (maker.__name__, *key) not in _CASES:
        _CASES[(maker.__name__, *key)] = maker(*key)
    return _CASES[(maker.__name__, *key)]


def hold(kern, dtype, name, checks):
    """every figure is recorded and printed before anything is asserted on it"""
    torch.cuda.synchronize()
    for k, r in checks.items():
        WORST[(kern, dtype)] = max(WORST.get((kern, dtype), 0.0), r)
        print(f"{kern} {dtype} {name} {k}: error / tolerance {r:.3f}")
    bad = {k: r for k, r in checks.items() if not r <= 1.0}
    assert not bad, (kern, dtype, name, bad)


def dev(t, dtype=None):
    t = torch.as_tensor(t)
    return (t if dtype is None else t.to(dtype)).to(DEV).contiguous()


def ptr(t):
    return None if t is None else t.data_ptr()


def sent(shape, dtype=F32):
    return torch.full(shape, NC.SENT, dtype=dtype, device=DEV)


def same(*pairs):
    return NC.exact(all(torch.equal(a, b) for a, b in pairs))


def check_rc(rc, what):
    from speech_decoding_amd import lib
    lib.check(rc, what)


# ---------------------------------------------------------------------------------------------------------------
# per kernel
# ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", NC.STATS_SHAPES, ids=str)
def test_neg_stats(ops, shape):
    from speech_decoding_amd import lib
    Bn, N = shape
    for regime in NC.STATS_REGIMES:
        c = case(NC.stats_case, Bn, N, regime)
        Sd, wsq, zsq, temp = dev(c["S"]), dev(c["wsq"]), dev(c["zsq"]), dev(c["temp"])
        mlog, cl = sent((Bn + 1, N)), sent((Bn + 1,))
        cl[:Bn] = dev(c["col_lse"])
        check_rc(lib.load().sda_clip_neg_stats(ptr(Sd), Sd.shape[1], ptr(wsq), ptr(zsq), ptr(temp), ptr(mlog), ptr(cl), Bn, N, ops._st()),
                 "clip_neg_stats")
        checks = NC.check_neg_stats(c, mlog, cl)
        cl_w = dev(c["col_lse"]).clone()
        w = ops.clip_neg_stats(Sd, wsq, zsq, temp, cl_w, Bn, N)
        checks["the wrapper gives the same bits"] = same((w, mlog[:Bn]), (cl_w, cl[:Bn]))
        hold("clip_neg_stats", F32, c["name"], checks)


@pytest.mark.parametrize("dtype", NC.DTYPES16, ids=str)
@pytest.mark.parametrize("shape", NC.STATS_SHAPES, ids=str)
def test_neg_grad(ops, dtype, shape):
    from speech_decoding_amd import lib
    Bn, N = shape
    nr = NC.neg_rows(N)
    assert ops.clip_neg_rows(N) == nr
    for regime in NC.STATS_REGIMES:
        c = case(NC.stats_case, Bn, N, regime)
        ins = [dev(c["mlog"]), dev(c["col_lse_merged"]), dev(c["wsq"]), dev(c["zsq"]), dev(c["temp"])]
        G, cs, colpart = sent((nr + 1, NC.pad64(Bn)), dtype), sent((Bn,)), sent((Bn,))
        rscale, scalars = dev(c["rscale_in"]).clone(), dev(c["scalars_in"]).clone()
        check_rc(lib.load().sda_clip_neg_grad(*map(ptr, ins), c["inv_norm"], ptr(G), G.shape[1], ptr(cs), ptr(rscale), ptr(colpart), ptr(scalars),
                                              Bn, N, ops.dt_code(dtype), ops._st()), "clip_neg_grad")
        checks = NC.check_neg_grad(c, dtype, G, cs, rscale, scalars)
        r2, s2 = dev(c["rscale_in"]).clone(), dev(c["scalars_in"]).clone()
        w = ops.clip_neg_grad(*ins, c["inv_norm"], r2, s2, dtype)
        checks["the wrapper gives the same bits"] = same((w[0], G[:nr]), (w[1], cs), (r2, rscale), (s2, scalars))
        hold("clip_neg_grad", dtype, c["name"], checks)


def launch_dz_windows(ops, c, dtype):
    """the C entry point on buffers the test owns: the table is an allocation of its own, exactly as long as its rows (a window
    that ends at the last row ends at the allocation), `out` has one sentinel row behind the row-layout buffer"""
    from speech_decoding_amd import lib
    Bn, N, T, Fp = c["Bn"], c["N"], c["T"], c["Fp"]
    Gn, table, starts = dev(c["Gn"], dtype), dev(c["table"], dtype), dev(c["starts"])
    cs, os_ = dev(c["cscale"]), dev(c["out_scale"])
    out = sent((c["out"].shape[0] + 1, Fp), dtype)
    out[:-1] = dev(c["out"], dtype)
    lo, hi = int(c["starts"].min()), int(c["starts"].max())
    check_rc(lib.load().sda_clip_dz_windows(ptr(Gn), Gn.shape[1], ptr(table), ptr(starts), lo, hi - lo, Fp, ptr(out), (T + NC.ROW_PAD) * Fp, ptr(cs),
                                            ptr(os_), N, Bn, T * Fp, ops.dt_code(dtype), ops._st()), "clip_dz_windows")
    out_w = dev(c["out"], dtype).clone()
    ops.clip_dz_windows(Gn, table, starts, lo, hi, out_w, cs, N=N, Bn=Bn, T=T, out_scale=os_)
    return out, out_w


@pytest.mark.parametrize("dtype", NC.DTYPES16, ids=str)
@pytest.mark.parametrize("shape", NC.DZ_SHAPES, ids=str)
def test_dz_windows(ops, dtype, shape):
    for pattern in NC.START_PATTERNS:
        c = case(NC.dz_case, *shape, pattern, dtype)
        out, out_w = launch_dz_windows(ops, c, dtype)
        checks = NC.check_dz_windows(c, dtype, out)
        checks["the wrapper gives the same bits"] = same((out_w, out[:-1]))
        hold("clip_dz_windows", dtype, c["name"], checks)


@pytest.mark.parametrize("dtype", NC.DTYPES16, ids=str)
@pytest.mark.parametrize("shape", NC.DZ_SHAPES, ids=str)
def test_dz_windows_exact(ops, dtype, shape):
    """small-integer operands, power-of-two factors, a non-zero `out` underneath: the exact sum rounded to nearest even, bit for bit"""
    for pattern in NC.START_PATTERNS:
        c = case(NC.dz_case, *shape, pattern, dtype, True)
        out, out_w = launch_dz_windows(ops, c, dtype)
        checks = NC.check_dz_windows(c, dtype, out)
        checks["the wrapper gives the same bits"] = same((out_w, out[:-1]))
        checks["a second launch on the same inputs gives the same bits"] = same((launch_dz_windows(ops, c, dtype)[0], out))
        hold("clip_dz_windows exact", dtype, c["name"], checks)


# ---------------------------------------------------------------------------------------------------------------
# whole loss
# ---------------------------------------------------------------------------------------------------------------
# (B, N, F, T, start pattern): every N and B of the axes, F in {3, 64}, T in {4, 5, 9}
LOSS_SHAPES = ((2, 1, 3, 4, "edges"), (64, 31, 64, 5, "overlap"), (65, 32, 3, 9, "descending"), (257, 33, 64, 4, "same"), (64, 255, 3, 5, "edges"),
               (65, 256, 64, 4, "descending"), (2, 257, 3, 9, "overlap"), (64, 289, 64, 5, "same"))
TEMP = 2.5


def randn(*shape, seed):
    return torch.randn(*shape, generator=torch.Generator().manual_seed(seed))


def clip(reduction="mean", temp=TEMP, duplicates="positive"):
    from speech_decoding.utils.loss import CLIPLoss
    return CLIPLoss(TB.Config(reduction=reduction, init_temperature=temp, clip_duplicates=duplicates)).to(DEV)


def make_bank(F, T, dtype, starts, L=None, seed=0, device=DEV):
    """a WindowBank of one track of L rows (values rounded to dtype) with windows at `starts`, and the track on the host (F, L)"""
    from speech_decoding_amd.retrieval import WindowBank
    L = NC.DZ_TABLE_ROWS if L is None else L
    E = (3.0 * randn(F, L, seed=77 + seed) * torch.exp(0.5 * randn(1, L, seed=78 + seed))).to(DT[dtype])
    bank = WindowBank(F, T, dtype=DT[dtype], device=device)
    bank.add_track(E.to(device), np.asarray(starts))
    return bank, E.float()


def windows_host(E, starts, T):
    """(N, F, T) the negatives as embeddings, from the host copy of the track"""
    return torch.stack([E[:, int(s): int(s) + T] for s in starts])


def operands(B, F, T, dtype, seed=0):
    x = randn(B, F, T, seed=1000 * B + seed).to(DT[dtype]).to(DEV).requires_grad_(True)
    y = (0.6 * x.detach().float().cpu() + randn(B, F, T, seed=1000 * B + seed + 1)).to(DT[dtype]).to(DEV).requires_grad_(True)
    return x, y


def batch_labels(B):
    lab = np.arange(B, dtype=np.int64) + 100
    lab[[0, B - 1]] = 7
    if B >= 8:
        lab[[1, 4, B - 2]] = 8
    return lab


def compare(tag, dtype, loss, grads, ref, want_x=True):
    """figures first, then the project's bounds: (loss, dx, dy, dtemp) against float64"""
    lr, dxr, dyr, dtr, _ = ref
    dx, dy, dt = grads
    figs = dict(loss=float(loss), loss_ref=float(lr), dy=rel_l2(dy, dyr), dtemp=float(dt), dtemp_ref=float(dtr))
    if want_x:
        figs["dx"] = rel_l2(dx, dxr)
    print(tag, dtype, figs)
    assert abs(float(loss) - float(lr)) <= LOSS_REL[dtype] * abs(float(lr)), figs
    assert figs["dy"] <= GRAD_REL_L2[dtype], figs
    assert not want_x or figs["dx"] <= GRAD_REL_L2[dtype], figs
    assert abs(float(dt) - float(dtr)) <= DTEMP * max(1.0, abs(float(dtr))), figs


@pytest.mark.parametrize("dtype", ["bf16", "fp16"])
@pytest.mark.parametrize("shape", LOSS_SHAPES, ids=str)
def test_whole_loss_against_float64_autograd(shape, dtype):
    B, N, F, T, pattern = shape
    starts = NC.starts_of(N, NC.DZ_TABLE_ROWS, T, pattern)
    bank, E = make_bank(F, T, dtype, starts)
    x, y = operands(B, F, T, dtype)
    w = windows_host(E, starts, T)
    for reduction in ("mean", "sum"):
        crit = clip(reduction)
        loss = crit(x, y, negatives=bank)
        grads = torch.autograd.grad(loss, [x, y, crit.temp])
        ref = NC.loss_ref_embeddings(x, y, w, TEMP, reduction=reduction)
        compare(f"{shape} {reduction}", dtype, loss, grads, ref)
        # the negatives are in it: the plain loss differs (a single far-away negative may change little: N = 1 is exempt)
        plain = float(NC.loss_ref_embeddings(x, y, w[:0], TEMP, reduction=reduction)[0])
        assert N == 1 or abs(plain - float(ref[0])) > 1e-3 * abs(plain)
    dz = grads[1]
    assert dz.dtype == DT[dtype] and tuple(dz.shape) == (B, F, T)


@pytest.mark.parametrize("dtype", ["bf16", "fp16"])
@pytest.mark.parametrize("mode", ["positive", "mask"])
def test_whole_loss_with_labels(mode, dtype):
    """the labelled kernels act on the paired block and are handed the widened column lse; the negatives carry fresh ids"""
    for B, N, F, T, pattern in ((12, 33, 64, 5, "edges"), (65, 40, 3, 9, "overlap")):
        starts = NC.starts_of(N, NC.DZ_TABLE_ROWS, T, pattern)
        bank, E = make_bank(F, T, dtype, starts)
        x, y = operands(B, F, T, dtype, seed=3)
        lab = batch_labels(B)
        crit = clip("mean", TEMP, mode)
        loss = crit(x, y, labels=lab, negatives=bank)
        grads = torch.autograd.grad(loss, [x, y, crit.temp])
        compare(f"B={B} N={N} labels {mode}", dtype, loss, grads, NC.loss_ref_embeddings(x, y, windows_host(E, starts, T), TEMP, lab, mode))


@pytest.mark.parametrize("dtype", ["bf16", "fp16"])
def test_fast_false_and_no_speech_gradient(dtype):
    B, N, F, T = 12, 33, 3, 5
    starts = NC.starts_of(N, NC.DZ_TABLE_ROWS, T, "descending")
    bank, E = make_bank(F, T, dtype, starts)
    x, y = operands(B, F, T, dtype, seed=5)
    crit = clip()
    logits, loss = crit(x.detach(), y, fast=False, return_logits=True, negatives=bank)
    (dy,) = torch.autograd.grad(loss, [y])
    lr, _, dyr, _, lg = NC.loss_ref_embeddings(x, y, windows_host(E, starts, T), TEMP, fast=False)
    assert abs(float(loss) - float(lr)) <= LOSS_REL[dtype] * abs(float(lr)) and rel_l2(dy, dyr) <= GRAD_REL_L2[dtype]
    assert tuple(logits.shape) == (B, B) and rel_l2(logits, lg.t()) <= 1e-5          # the turned PAIRED block, no temperature


def test_whole_loss_on_the_toy_encoders_output():
    """Z is the encoder's own row-layout output (T = 70: 17 whole tiles and a partial one): loss, dZ and dtemp against float64"""
    d = dict(TB.TOY)
    B, N, dtype = 12, 40, "bf16"
    loc, P, X, Y, subj = TB.toy_problem(d, B)
    enc = TB.build_encoder(P, TB.encoder_args(d, loc, dtype), DEV)
    starts = NC.starts_of(N, 120, d["T"], "edges")
    bank, E = make_bank(d["F"], d["T"], dtype, starts, L=120)
    crit = clip()
    Yd = Y.to(DT[dtype]).to(DEV)
    Z = enc(X.to(DEV), subj)
    Z.retain_grad()
    loss = crit(Yd, Z, negatives=bank)
    loss.backward()
    ref = NC.loss_ref_embeddings(Yd, Z, windows_host(E, starts, d["T"]), TEMP)
    compare("toy encoder", dtype, loss, (None, Z.grad, crit.temp.grad), ref, want_x=False)
    assert all(p.grad is not None and bool(torch.isfinite(p.grad if not p.grad.is_complex() else torch.view_as_real(p.grad)).all())
               for p in enc.parameters())


# ---------------------------------------------------------------------------------------------------------------
# launch and bit identity
# ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", ["bf16", "fp32"])
def test_negatives_none_is_the_plain_call_bit_for_bit(dtype):
    B, F, T = 12, 64, 5
    x = randn(B, F, T, seed=1).to(DT[dtype]).to(DEV).requires_grad_(True)
    y = randn(B, F, T, seed=2).to(DT[dtype]).to(DEV).requires_grad_(True)
    lab = batch_labels(B)

    def run(**kw):
        crit = clip()
        logits, loss = crit(x, y, return_logits=True, **kw)
        return (loss.detach().clone(), logits.clone(), *[g.clone() for g in torch.autograd.grad(loss, [x, y, crit.temp])])
    for kw in ({}, {"labels": lab}):
        for a, b in zip(run(**kw), run(negatives=None, **kw)):
            assert torch.equal(a, b)
    if dtype == "bf16":      # and a call with negatives in between changes nothing of a plain call after it
        before = run()
        bank, _ = make_bank(F, T, dtype, NC.starts_of(33, NC.DZ_TABLE_ROWS, T, "edges"))
        with_neg = run(negatives=bank)
        assert not torch.equal(with_neg[0], before[0])
        assert torch.equal(with_neg[1], before[1])          # the returned logits stay the paired block
        for a, b in zip(before, run()):
            assert torch.equal(a, b)


def test_reference_windows_are_the_gathered_windows(ops):
    """the N windows materialised through ops.gather_windows are the windows the float64 reference appends: the row offset"""
    F, T, N = 3, 9, 33
    starts = NC.starts_of(N, NC.DZ_TABLE_ROWS, T, "descending")
    bank, E = make_bank(F, T, "bf16", starts)
    rows = ops.gather_windows(bank.table, bank.starts, torch.arange(N, device=DEV), N, T)
    got = ops.unpack_rows(rows, N, F, T, torch.float32).cpu()
    assert torch.equal(got, windows_host(E, starts, T))
    x, y = operands(12, F, T, "bf16", seed=9)
    a = NC.loss_ref_embeddings(x, y, got, TEMP)
    b = NC.loss_ref_embeddings(x, y, NC.bank_windows(bank.table.float().cpu(), starts, F, T), TEMP)
    assert float(a[0]) == float(b[0]) and torch.equal(a[2], b[2])


# ---------------------------------------------------------------------------------------------------------------
# data parallelism
# ---------------------------------------------------------------------------------------------------------------
DP = dict(B=8, N=40, F=64, T=9, dtype="fp16")      # fp16: one storage ulp (2^-11) lies inside tests/test_dp_gpu.py's 2e-3 bound


def _dp_worker(rank, world, dev_, d):
    from speech_decoding_amd.distributed import shard_range
    from speech_decoding_amd.loss import retrieval_ranks
    B, N, F, T, dtype = d["B"], d["N"], d["F"], d["T"], d["dtype"]
    Bg = B * world
    x = randn(Bg, F, T, seed=11).to(DT[dtype])
    y = (0.6 * x.float() + randn(Bg, F, T, seed=12)).to(DT[dtype])
    starts = NC.starts_of(N, NC.DZ_TABLE_ROWS, T, "edges")
    bank, _ = make_bank(F, T, dtype, starts, device=dev_)          # every rank is handed the same negatives

    def run(xs, ys, global_negatives):
        from speech_decoding.utils.loss import CLIPLoss
        crit = CLIPLoss(TB.Config(reduction="mean", init_temperature=TEMP)).to(dev_)
        crit.global_negatives = global_negatives
        xs, ys = xs.to(dev_), ys.to(dev_).requires_grad_(True)
        loss = crit(xs, ys, negatives=bank)
        dz, dt = torch.autograd.grad(loss, [ys, crit.temp])
        return dict(loss=float(loss), dz=dz.float().cpu(), dtemp=float(dt), ranks=retrieval_ranks(xs, ys, global_negatives).cpu())
    lo, hi = shard_range(Bg, rank, world)
    res = run(x[lo:hi], y[lo:hi], True)
    if rank == 0:
        res["ref"] = run(x, y, False)
    return res


def test_two_ranks_match_one_process_on_the_global_batch():
    world, B = 2, DP["B"]
    out = run_ranks(_dp_worker, world, DP, backend="gloo")
    ref = out[0]["ref"]
    dt = sum(out[r]["dtemp"] for r in range(world))
    print({r: out[r]["loss"] for r in range(world)}, ref["loss"], dt, ref["dtemp"])
    scale = float(ref["dz"].abs().max())
    for r in range(world):
        assert abs(out[r]["loss"] - ref["loss"]) < 2e-5                       # tests/test_dp_gpu.py's bounds
        err = float((out[r]["dz"] - ref["dz"][r * B:(r + 1) * B]).abs().max())
        print(r, err, scale)
        assert err <= 2e-3 * scale + 1e-7
        assert torch.equal(out[r]["ranks"], ref["ranks"][r * B:(r + 1) * B])
    assert abs(dt - ref["dtemp"]) <= 2e-3 * abs(ref["dtemp"]) + 1e-7


# ---------------------------------------------------------------------------------------------------------------
# refusals, the feed, train.py
# ---------------------------------------------------------------------------------------------------------------
def test_refusals_reach_python_before_any_launch(ops):
    from speech_decoding_amd import lib
    from speech_decoding_amd.lib import SdaError
    F, T = 64, 5
    starts = NC.starts_of(8, NC.DZ_TABLE_ROWS, T, "edges")
    bank, _ = make_bank(F, T, "bf16", starts)
    x, y = operands(4, F, T, "bf16")
    crit = clip()
    with pytest.raises(SdaError, match="16-bit storage only"):
        crit(x.float(), y.float(), negatives=bank)                            # fp32 compute
    with pytest.raises(SdaError, match="F=64, T=5"):
        crit(*operands(4, 3, T, "bf16"), negatives=bank)                      # F
    with pytest.raises(SdaError, match="F=64, T=5"):
        crit(*operands(4, F, 9, "bf16"), negatives=bank)                      # T
    with pytest.raises(SdaError, match="bfloat16"):
        crit(*operands(4, F, T, "fp16"), negatives=bank)                      # dtype
    with pytest.raises(SdaError, match="empty bank"):
        crit(x, y, negatives=bank.select(np.zeros(0, dtype=np.int64)))
    with pytest.raises(SdaError, match="must be a WindowBank"):
        crit(x, y, negatives=torch.zeros(8, F, T, device=DEV))
    # a span that is too wide, at the C entry point with its arguments alone (no 4 GB table): refused, nothing launched
    span = ops.clip_dz_windows_span(64)
    assert span == (2 ** 31 - 256) // 64 and ops.clip_dz_windows_span(65) == 0
    small = torch.zeros(64, 64, dtype=torch.bfloat16, device=DEV)
    st = torch.zeros(8, dtype=torch.int32, device=DEV)
    cs = torch.zeros(8, device=DEV)
    out = sent((64, 64), torch.bfloat16)
    args = lambda **kw: {**dict(g_pitch=64, base=0, span=0, re=64, pitch=(T + 16) * 64, N=8, Bn=2, K=T * 64, dt=ops.dt_code(torch.bfloat16)), **kw}

    def rc(Gn=small, table=small, starts=st, o=out, c=cs, **kw):
        a = args(**kw)
        return lib.load().sda_clip_dz_windows(ptr(Gn), a["g_pitch"], ptr(table), ptr(starts), a["base"], a["span"], a["re"], ptr(o), a["pitch"], ptr(c),
                                              None, a["N"], a["Bn"], a["K"], a["dt"], ops._st())
    for bad in (dict(span=span + 1), dict(span=-1), dict(dt=ops.dt_code(torch.float32)), dict(K=T * 64 + 16), dict(K=T * 64 + 32), dict(re=96),
                dict(base=-1), dict(g_pitch=1), dict(g_pitch=12), dict(pitch=T * 64), dict(N=0), dict(Bn=0), dict(Gn=None), dict(table=None),
                dict(starts=None), dict(o=None), dict(c=None), dict(table=small.view(-1)[4:]), dict(o=out.view(-1)[4:])):
        assert rc(**bad) == -1, bad
        assert lib.load().sda_last_error()
    torch.cuda.synchronize()
    assert bool((out == NC.SENT).all())                                       # no launch wrote anything
    with pytest.raises(SdaError, match="more than the"):
        ops.clip_dz_windows(small, small.new_zeros(64, 64), st, 0, span + 1, small.new_zeros(2 * (T + 16) + 200, 64), cs, N=8, Bn=2, T=T)


def train_args(*more):
    from oracle import brain_oracle as O
    from speech_decoding_amd import load_config
    args = load_config(overrides=["dataset=Gwilliams2022", "num_subjects=4", "D1=32", "D2=48", "F=64", "K=4", "batch_size=12", "epochs=2",
                                  "num_channels=20", "preprocs.last4layers=False", "preprocs.seq_len_sec=1", "preprocs.brain_resample_rate=16",
                                  "preprocs.baseline_len_sec=0.25", "lr=3e-4", "synthetic_segments=64", "updates_per_epoch=2",
                                  "split_ratio=0.8", "compute_dtype=bf16", "data=tracks", "reproducible=True", *more])
    args["sensor_positions"] = O.synthetic_positions(20, seed=7).numpy()
    return args


def test_feed_draws_negatives_from_the_training_split():
    from speech_decoding_amd import data as D
    from speech_decoding_amd.lib import SdaError
    args = train_args()
    feed, train_idx, test_idx = D.synthetic_track_dataset(args, DEV, n_segments=64, dtype=torch.bfloat16)
    batch = train_idx[:12]
    neg = feed.draw_negatives(16, batch, train_idx)
    assert len(set(neg.tolist())) == 16 and set(neg.tolist()) <= set(train_idx.tolist()) and not set(neg.tolist()) & set(test_idx.tolist())
    assert not set(feed.speech_ids(neg).tolist()) & set(feed.speech_ids(batch).tolist())
    bank = feed.speech_bank(neg)
    assert len(bank) == 16 and bank.table.data_ptr() == feed.speech_bank().table.data_ptr()      # the resident table, shared
    with pytest.raises(ValueError, match="the pool holds"):
        feed.draw_negatives(len(train_idx), batch, train_idx)
    with pytest.raises(SdaError, match="materialised Y"):
        D.synthetic_resident_dataset(args, DEV, n_segments=64)[0].draw_negatives(4, batch, train_idx)


def test_train_with_clip_negatives(tmp_path, monkeypatch):
    """train.py clip_negatives=N: N = 0 is today's run figure for figure; N = 12 trains on a larger loss and gives another model"""
    import train
    monkeypatch.chdir(tmp_path)                                               # model_last.pt

    def history(*more):
        h, _, _ = train.run(train_args(*more), log=lambda *a: None)
        return [(float(r["train_loss"]), float(r["test_loss"]), float(r["temp"])) for r in h]
    plain, zero, neg = history(), history("clip_negatives=0"), history("clip_negatives=12")
    print(plain, neg)
    assert plain == zero
    assert all(np.isfinite(v) for row in neg for v in row)
    assert neg[0][0] > plain[0][0]                                            # 12 more candidates per brain segment: a larger loss
    assert neg[1][1] != plain[1][1]                                           # and another model at evaluation (which has no negatives)
