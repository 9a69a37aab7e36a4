"""The CLIP loss with speech labels on a real MI355X.

Per kernel: every entry point of csrc/clip_labels.hip launched on its own over the shapes x label patterns x regimes of
tests/clip_label_cases.py — through its ops.* wrapper and through the C entry point into sentinel-filled buffers the test owns —
and held to float64 on the fp32 inputs it is handed, within that file's constants; counts and ranks exactly.
tests/test_clip_labels_cpu.py shows that these cases catch the planted bugs.

Whole loss: CLIPLoss(x, y, labels=) at B = 12 and 70 against float64 autograd of the two-line forms on the operands as the device
sees them (loss, dZ, dY, dtemp), both reductions, both modes, the three compute dtypes, with the project's bounds.

Invariants, refusals, the feeds' speech ids and train.py's clip_duplicates option follow."""
import numpy as np
import pytest
import torch

from tests import builders as TB
from tests import clip_label_cases as LC
from tests import sa_loss_cases as S
from tests.parity import rel_l2

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
F32 = torch.float32
DT = {"fp32": torch.float32, "bf16": torch.bfloat16, "fp16": torch.float16}
GRAD_REL_L2 = {"fp32": 1e-5, "bf16": 6e-2, "fp16": 8e-3}      # DESIGN §5, tests/test_clip_dy_gpu.py
LOSS_REL = {"fp32": 1e-5, "bf16": 1e-2, "fp16": 1e-2}
WORST = {}
_BASE, _CASES = {}, {}


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


def cases(shape, regimes=LC.CLIP_REGIMES, patterns=LC.LABEL_PATTERNS):
    """one reference per case, shared by the tests and left unchanged"""
    for regime in regimes:
        for pattern in patterns:
            key = (*shape, regime, pattern)
            if key not in _CASES:
                if key[:4] not in _BASE:
                    _BASE[key[:4]] = S.clip_case(*shape, regime)
                _CASES[key] = LC.label_case(*shape, regime, pattern, base=_BASE[key[:4]])
            yield _CASES[key]


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
    return S.exact(all(torch.equal(a, b) for a, b in pairs))


def check_rc(rc, what):
    from speech_decoding_amd import lib
    lib.check(rc, what)


def mode_code(ops, mode):
    return ops.clip_dup_code(mode)


# ---------------------------------------------------------------------------------------------------------------
# per kernel
# ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", LC.LABEL_SHAPES, ids=str)
def test_label_counts(ops, shape):
    from speech_decoding_amd import lib
    Bm = shape[0]
    for c in cases(shape, regimes=("flat",)):
        lab = dev(c["labels"])
        buf = torch.full((Bm + 3,), -7, dtype=torch.int32, device=DEV)
        check_rc(lib.load().sda_clip_label_counts(ptr(lab), ptr(buf), Bm, ops._st()), "clip_label_counts")
        w = ops.clip_label_counts(lab)
        hold("clip_label_counts", "int32", c["name"], {"counts equal": S.exact(torch.equal(buf[:Bm].cpu(), c["counts"])),
                                                        "past Bg untouched": S.exact((buf[Bm:] == -7).all()),
                                                        "the wrapper gives the same bits": same((w, buf[:Bm]))})


@pytest.mark.parametrize("shape", LC.LABEL_SHAPES, ids=str)
def test_logits_stats_masked(ops, shape):
    from speech_decoding_amd import lib
    Bm, Bn, col0 = shape
    for c in cases(shape):
        Sd, ysq, zsq, temp, lab = dev(c["S"]), dev(c["ysq"]), dev(c["zsq"]), dev(c["temp"]), dev(c["labels"])
        logits, st3, col_lse, row_lse = sent((Bm + 1, Bn)), sent((3, Bm)), sent((Bn + 1,)), sent((Bm + 1,))
        check_rc(lib.load().sda_clip_logits_stats_masked(ptr(Sd), Sd.shape[1], ptr(ysq), ptr(zsq), ptr(temp), ptr(lab), ptr(logits), ptr(st3[0]),
                                                         ptr(st3[1]), ptr(col_lse), ptr(st3[2]), ptr(row_lse), Bm, Bn, col0, ops._st()),
                 "clip_logits_stats_masked")
        checks = LC.check_masked_stats(c, logits[:Bm], st3[0], st3[1], col_lse[:Bn], st3[2], row_lse[:Bm])
        checks["past the outputs untouched"] = S.exact(bool((logits[Bm:] == S.SENT).all()) and float(col_lse[Bn]) == S.SENT and float(row_lse[Bm]) == S.SENT)
        w = ops.clip_logits_stats_masked(Sd, ysq, zsq, temp, lab, Bm, Bn, col0)
        checks["the wrapper gives the same bits"] = same(*zip(w, (logits[:Bm], st3[0], st3[1], col_lse[:Bn], st3[2], row_lse[:Bm])))
        if c["pattern"] == "distinct":
            u = ops.clip_logits_stats(Sd, ysq, zsq, temp, Bm, Bn, col0)
            checks["all distinct: the unlabelled kernel's bits"] = same(*zip(w, u))
        hold("clip_logits_stats_masked", F32, c["name"], checks)


@pytest.mark.parametrize("dtype", S.DTYPES, ids=str)
@pytest.mark.parametrize("shape", LC.LABEL_SHAPES, ids=str)
def test_grad_labels(ops, dtype, shape):
    from speech_decoding_amd import lib
    Bm, Bn, col0 = shape
    for c in cases(shape):
        lab, cnt = dev(c["labels"]), dev(c["counts"])
        for mode in LC.MODES:
            rl, cl = LC.lse_inputs(c, mode)
            ins = [dev(c["logits"]), dev(rl), dev(cl), dev(c["ysq"]), dev(c["zsq"]), dev(c["temp"])]
            G = sent((Bm + 2, S.pad64(Bn)), dtype)
            rscale, cscale, colpart, scalars = sent((Bn,)), sent((Bn,)), sent((2 * Bn,)), sent((2,))
            check_rc(lib.load().sda_clip_grad_labels(*map(ptr, ins), ptr(lab), ptr(cnt), mode_code(ops, mode), c["inv_norm"], col0, ptr(G), G.shape[1],
                                                     ptr(rscale), ptr(cscale), ptr(colpart), ptr(scalars), Bm, Bn, ops.dt_code(dtype), ops._st()),
                     "clip_grad_labels")
            checks = LC.check_grad_labels(c, mode, dtype, G, rscale, cscale, scalars)
            w = ops.clip_grad_labels(*ins, lab, cnt, mode, c["inv_norm"], col0, dtype)
            checks["the wrapper gives the same bits"] = same(*zip(w, (G[:Bm + 1], rscale, cscale, scalars)))
            hold(f"clip_grad_labels[{mode}]", dtype, c["name"], checks)


@pytest.mark.parametrize("dtype", S.DTYPES, ids=str)
@pytest.mark.parametrize("shape", LC.LABEL_SHAPES, ids=str)
def test_grad_y_labels(ops, dtype, shape):
    from speech_decoding_amd import lib
    Bm, Bn, col0 = shape
    seg, seg_pitch, groups = S.gy_layout(Bm, Bn, col0)
    nparts = (Bn + 63) // 64
    for c in cases(shape):
        lab, cnt = dev(c["labels"]), dev(c["counts"])
        for mode in LC.MODES:
            rl, cl = LC.lse_inputs(c, mode)
            ins = [dev(c["logits"]), dev(rl), dev(cl), dev(c["zsq"]), dev(c["zsq_all"])]
            Gy, part = sent((Bn + 2, groups * seg_pitch), dtype), sent((nparts + 1, Bm))
            check_rc(lib.load().sda_clip_grad_y_labels(*map(ptr, ins), Bm, ptr(lab), ptr(cnt), mode_code(ops, mode), col0, ptr(Gy), Gy.shape[1], seg,
                                                       seg_pitch, ptr(part), Bm, Bn, ops.dt_code(dtype), ops._st()), "clip_grad_y_labels")
            checks = LC.check_grad_y_labels(c, mode, dtype, Gy, part)
            w = ops.clip_grad_y_labels(*ins, lab, cnt, mode, col0, dtype, seg=seg, seg_pitch=seg_pitch, groups=groups)
            checks["the wrapper gives the same bits"] = same((w[0], Gy[:Bn + 1]), (w[1], part[:nparts]))
            hold(f"clip_grad_y_labels[{mode}]", dtype, c["name"], checks)


@pytest.mark.parametrize("shape", LC.LABEL_SHAPES, ids=str)
def test_ranks_labels(ops, shape):
    from speech_decoding_amd import lib
    Bm, Bn, col0 = shape
    for c in cases(shape):
        logits, diag, lab = dev(c["logits"]), dev(c["diag"]), dev(c["labels"])
        buf = torch.full((Bm + 3,), -7, dtype=torch.int32, device=DEV)
        check_rc(lib.load().sda_clip_ranks_labels(ptr(logits), ptr(diag), ptr(lab), ptr(buf), Bm, Bn, col0, ops._st()), "clip_ranks_labels")
        w = ops.clip_ranks_labels(logits, diag, lab, col0)
        checks = {"counts equal": S.exact(torch.equal(buf[:Bm].cpu(), LC.ranks_labels_ref(c))), "past Bm untouched": S.exact((buf[Bm:] == -7).all()),
                  "the wrapper gives the same bits": same((w, buf[:Bm]))}
        if c["pattern"] == "distinct":
            checks["all distinct: the unlabelled counts"] = same((w, ops.clip_ranks(logits, diag, col0)))
        hold("clip_ranks_labels", "int32", c["name"], checks)


# ---------------------------------------------------------------------------------------------------------------
# whole loss
# ---------------------------------------------------------------------------------------------------------------
F_, T_ = 64, 40


def randn(*shape, seed):
    return torch.randn(*shape, generator=torch.Generator().manual_seed(seed))


def batch_labels(B, kind):
    """mixed: a pair, a class of three and (B = 70) a class of a quarter of the batch; one_class: every sample the same"""
    lab = np.arange(B, dtype=np.int64) + 100
    if kind == "one_class":
        lab[:] = 5
        return lab
    lab[[1, B - 2]] = 7
    lab[[0, 4, B - 1]] = 8
    if B >= 40:
        lab[10:10 + B // 4] = 9
    return lab


def clip(reduction="mean", temp=2.5, duplicates="positive"):
    from speech_decoding.utils.loss import CLIPLoss
    return CLIPLoss(TB.Config(reduction=reduction, init_temperature=temp, clip_duplicates=duplicates)).to(DEV)


def operands(B, dtype, seed=0):
    """speech x and brain y as the device sees them (rounded to the compute dtype), leaves on the device"""
    x = randn(B, F_, T_, seed=1000 * B + seed).to(DT[dtype]).to(DEV).requires_grad_(True)
    y = (0.6 * x.detach().float().cpu() + randn(B, F_, T_, seed=1000 * B + seed + 1)).to(DT[dtype]).to(DEV).requires_grad_(True)
    return x, y


@pytest.mark.parametrize("dtype", ["fp32", "bf16", "fp16"])
@pytest.mark.parametrize("mode", LC.MODES)
@pytest.mark.parametrize("reduction", ["mean", "sum"])
@pytest.mark.parametrize("B", [12, 70])
def test_whole_loss_against_float64_autograd(B, reduction, mode, dtype):
    x, y = operands(B, dtype)
    lab = batch_labels(B, "mixed")
    crit = clip(reduction, 2.5, mode)
    loss = crit(x, y, labels=lab)
    dx, dy, dt = torch.autograd.grad(loss, [x, y, crit.temp])
    lr, dxr, dyr, dtr, _ = LC.loss_ref_embeddings(x, y, 2.5, lab, mode, reduction)
    figs = dict(loss=float(loss), loss_ref=float(lr), dx=rel_l2(dx, dxr), dy=rel_l2(dy, dyr), dtemp=float(dt), dtemp_ref=float(dtr))
    print(B, reduction, mode, dtype, figs)
    assert abs(float(loss) - float(lr)) <= LOSS_REL[dtype] * abs(float(lr)), figs
    assert figs["dx"] <= GRAD_REL_L2[dtype] and figs["dy"] <= GRAD_REL_L2[dtype], figs
    if dtype == "fp32":
        assert abs(float(dt) - float(dtr)) <= 1e-4 * max(1.0, abs(float(dtr))), figs
    # the loss differs from the unlabelled one: the labels are in it
    assert abs(float(LC.loss_ref_embeddings(x, y, 2.5, None, mode, reduction)[0]) - float(lr)) > 1e-3 * abs(float(lr))


@pytest.mark.parametrize("reduction", ["mean", "sum"])
@pytest.mark.parametrize("B", [12, 70])
def test_one_class_under_mask_is_zero(B, reduction):
    """every sample carries the same speech: nothing is a negative, the loss is 0 (compared absolutely) and so are the gradients"""
    x, y = operands(B, "fp32")
    crit = clip(reduction, 2.5, "mask")
    loss = crit(x, y, labels=batch_labels(B, "one_class"))
    dx, dy, dt = torch.autograd.grad(loss, [x, y, crit.temp])
    plain = clip(reduction, 2.5)
    gx, gy = torch.autograd.grad(plain(x, y), [x, y])
    figs = dict(loss=float(loss), dx=float(dx.norm() / gx.norm()), dy=float(dy.norm() / gy.norm()), dtemp=float(dt))
    print(B, reduction, figs)
    scale = 1.0 if reduction == "mean" else float(B)
    assert abs(float(loss)) <= LC.LOSS_ABS_FLOOR * scale, figs
    assert figs["dx"] <= GRAD_REL_L2["fp32"] and figs["dy"] <= GRAD_REL_L2["fp32"] and abs(float(dt)) <= 1e-4, figs


@pytest.mark.parametrize("fast", [True, False])
def test_fast_false_takes_labels_too(fast):
    B = 12
    x, y = operands(B, "fp32", seed=7)
    lab = batch_labels(B, "mixed")
    crit = clip("mean", 2.5, "positive")
    logits, loss = crit(x, y, fast=fast, return_logits=True, labels=lab)
    lr, dxr, dyr, _, lg = LC.loss_ref_embeddings(x, y, 2.5, lab, "positive", "mean", fast=fast)
    dx, dy = torch.autograd.grad(loss, [x, y])
    assert abs(float(loss) - float(lr)) <= 1e-5 * abs(float(lr))
    assert rel_l2(dx, dxr) <= 1e-5 and rel_l2(dy, dyr) <= 1e-5
    assert rel_l2(logits, lg if fast else lg.t()) <= 1e-5           # the returned logits are the unmasked similarities


# ---------------------------------------------------------------------------------------------------------------
# invariants
# ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", ["fp32", "bf16"])
@pytest.mark.parametrize("mode", LC.MODES)
def test_all_distinct_labels_give_the_unlabelled_results(mode, dtype):
    B = 70
    x, y = operands(B, dtype, seed=3)
    crit = clip("mean", 2.5, mode)
    l0 = crit(x, y)
    g0 = torch.autograd.grad(l0, [x, y, crit.temp])
    l1 = crit(x, y, labels=np.arange(B) * 3 - 50)
    g1 = torch.autograd.grad(l1, [x, y, crit.temp])
    assert abs(float(l1) - float(l0)) <= LOSS_REL[dtype] * abs(float(l0))
    assert rel_l2(g1[0], g0[0].float()) <= GRAD_REL_L2[dtype] and rel_l2(g1[1], g0[1].float()) <= GRAD_REL_L2[dtype]
    assert abs(float(g1[2]) - float(g0[2])) <= 1e-4 * max(1.0, abs(float(g0[2])))


@pytest.mark.parametrize("mode", LC.MODES)
def test_identical_speech_with_a_shared_label_is_symmetric(mode):
    """samples a and b hear the same speech (Y_a == Y_b) and share a label: which id the class carries changes no bit of dZ, and
    exchanging the two brain rows exchanges the two rows of dZ"""
    B, a, b = 12, 2, 9
    x, y = operands(B, "fp32", seed=5)
    with torch.no_grad():
        x[b] = x[a]
    lab = np.arange(B) + 100
    lab[b] = lab[a]
    crit = clip("mean", 2.5, mode)
    (dz,) = torch.autograd.grad(crit(x, y, labels=lab), [y])
    lab2 = lab.copy()
    lab2[[a, b]] = -2 ** 31                                  # the same classes under other ids
    (dz2,) = torch.autograd.grad(crit(x, y, labels=lab2), [y])
    assert torch.equal(dz, dz2)
    perm = list(range(B))
    perm[a], perm[b] = b, a
    ys = y.detach()[perm].clone().requires_grad_(True)
    (dzs,) = torch.autograd.grad(crit(x, ys, labels=lab), [ys])
    assert rel_l2(dzs[perm], dz) <= GRAD_REL_L2["fp32"]


def test_unlabelled_calls_around_a_labelled_one_are_bit_identical():
    from speech_decoding.models import Classifier
    B = 12
    x, y = operands(B, "fp32", seed=9)
    crit, clf = clip("mean", 2.5, "mask"), Classifier()

    def unlabelled():
        loss = crit(x, y)
        ranks = clf.ranks(y, x).clone()                      # (the loss's cached ranks)
        return (loss.detach().clone(), *[g.clone() for g in torch.autograd.grad(loss, [x, y, crit.temp])], ranks)

    before = unlabelled()
    lab = batch_labels(B, "mixed")
    loss = crit(x, y, labels=lab)
    torch.autograd.grad(loss, [x, y])
    labelled_ranks = clf.ranks(y, x, labels=lab).clone()
    # the cache hands a labelled result to the same labels only
    from speech_decoding_amd import loss as sda_loss
    assert sda_loss._cached_ranks(x, y) is None and sda_loss._cached_ranks(x, y, np.asarray(lab, dtype=np.int32).tobytes()) is not None
    fresh = clf.ranks(y, x).clone()                          # an unlabelled query after a labelled forward: computed, not the cache
    after = unlabelled()
    for u, v in zip(before, after):
        assert torch.equal(u, v)
    assert torch.equal(fresh, before[-1])
    assert sda_loss._cached_ranks(x, y, np.asarray(lab, dtype=np.int32).tobytes()) is None     # and not the reverse
    assert torch.equal(clf.ranks(y, x, labels=lab), labelled_ranks)


def test_a_repeat_scores_as_correct_with_labels_and_wrong_without():
    from speech_decoding.models import Classifier
    B, a, b = 12, 3, 8
    Y = randn(B, F_, T_, seed=21)
    Y[b] = Y[a]                                              # the same speech segment twice
    Z = Y + 0.3 * randn(B, F_, T_, seed=22)
    Z[b] = Y[b]                                              # b's brain matches the shared speech better than a's own
    Y, Z = Y.to(DEV), Z.to(DEV)
    lab = np.arange(B)
    lab[b] = lab[a]
    clf = Classifier()
    plain = clf.ranks(Z, Y).cpu()
    with_labels = clf.ranks(Z, Y, labels=lab).cpu()
    assert int(plain[a]) == 1 and int(with_labels[a]) == 0
    keep = [i for i in range(B) if i != a]
    assert torch.equal(plain[keep], with_labels[keep])
    t1_plain, _ = clf(Z, Y)
    t1_lab, _ = clf(Z, Y, labels=lab)
    assert t1_lab == 1.0 and abs(t1_plain - (B - 1) / B) < 1e-9


# ---------------------------------------------------------------------------------------------------------------
# refusals, before any launch
# ---------------------------------------------------------------------------------------------------------------
def test_refusals_come_before_any_launch(monkeypatch):
    from speech_decoding.utils.loss import CLIPLoss
    from speech_decoding_amd import ops
    B = 12
    x, y = operands(B, "fp32", seed=11)
    crit = clip()
    torch.cuda.synchronize()

    def boom(*a, **k):
        raise AssertionError("a kernel was launched before the labels were refused")

    for name in ("pack_rows", "rows_sumsq", "matmul_nt_splitk", "upload_small", "clip_label_counts"):
        monkeypatch.setattr(ops, name, boom)
    for bad in (np.arange(B - 1), list(range(B + 1)), torch.arange(B).reshape(2, -1)):
        with pytest.raises(ValueError, match="expected 12 speech ids"):
            crit(x, y, labels=bad)
    for bad in (np.arange(B, dtype=np.float32), torch.arange(B, dtype=torch.float32), [0.5] * B, torch.arange(B, device=DEV).half()):
        with pytest.raises(ValueError, match="int"):
            crit(x, y, labels=bad)
    for bad in (np.arange(B, dtype=np.int64) + 2 ** 31 - 5, torch.arange(B) - 2 ** 31 - 1):
        with pytest.raises(ValueError, match="fit int32"):
            crit(x, y, labels=bad)
    for bad in ("ignore", "negative", ""):
        with pytest.raises(ValueError, match="duplicates"):
            CLIPLoss(TB.Config(reduction="mean", init_temperature=1.0, clip_duplicates=bad))


def test_accepted_label_forms_agree():
    B = 12
    x, y = operands(B, "fp32", seed=13)
    lab = batch_labels(B, "mixed")
    crit = clip()
    forms = [lab, lab.tolist(), torch.from_numpy(lab), torch.from_numpy(lab).to(torch.int32), torch.from_numpy(lab).to(DEV),
             torch.from_numpy(lab).to(torch.int32).to(DEV), lab.astype(np.uint8)]
    outs = [crit(x, y, labels=f).detach().clone() for f in forms]
    assert all(torch.equal(o, outs[0]) for o in outs)


# ---------------------------------------------------------------------------------------------------------------
# feeds and train.py
# ---------------------------------------------------------------------------------------------------------------
def tiny_args(**over):
    from oracle import brain_oracle as O
    from speech_decoding_amd import load_config
    loc = O.synthetic_positions(12, seed=7)
    args = load_config(overrides=["dataset=Gwilliams2022", "num_subjects=3", "D1=16", "D2=24", "F=32", "K=4", "batch_size=12", "epochs=1",
                                  "num_channels=12", "preprocs.last4layers=False", "preprocs.seq_len_sec=1", "preprocs.brain_resample_rate=40",
                                  "preprocs.baseline_len_sec=0.25", "lr=3e-4", "synthetic_segments=20", "updates_per_epoch=2",
                                  "split_ratio=0.5", "data=resident"])
    args["sensor_positions"] = loc.numpy()
    args.update(over)
    return args


def test_speech_ids_and_the_four_tuple():
    from speech_decoding_amd import data as D
    args = tiny_args()
    feed, train_idx, _ = D.synthetic_resident_dataset(args, DEV, n_segments=20, seed=1234)
    idx = np.array([3, 17, 17, 9, 0])
    ids = feed.speech_ids(idx)
    assert ids.dtype == np.int64 and ids.tolist() == idx.tolist()                   # materialised Y: the segment index
    sampler = D.ShardedRandomSampler(len(train_idx), 12, 2, seed=5)
    three = list(feed.batches(sampler, index_map=train_idx))
    feed2 = D.synthetic_resident_dataset(args, DEV, n_segments=20, seed=1234)[0]
    four = list(feed2.batches(D.ShardedRandomSampler(len(train_idx), 12, 2, seed=5), index_map=train_idx, with_ids=True))
    assert all(len(b) == 3 for b in three) and all(len(b) == 4 for b in four)
    want = [np.asarray(train_idx)[i.numpy()] for i in D.ShardedRandomSampler(len(train_idx), 12, 2, seed=5)]
    for b3, b4, w in zip(three, four, want):
        assert all(torch.equal(u, v) for u, v in zip(b3, b4[:3]))                    # today's batch, plus the ids
        assert b4[3].dtype == torch.int64 and b4[3].tolist() == w.tolist()
        assert len(set(w.tolist())) < 12                                            # 12 draws from 10 segments: a repeat in every batch
    # Brennan2018's feed: the chunk index
    args_b = tiny_args(dataset="Brennan2018")
    Xc, Yc = D.synthetic_subject_dataset(args_b, DEV, length=20 * 40 + 6 + 13, seed=1)
    sf = D.ResidentSubjectFeed(Xc, Yc, srate=40, seq_len_sec=1, baseline_len_sec=0.25, clamp_lim=20.0, seed=3)
    assert sf.speech_ids([4, 4, 1]).tolist() == [4, 4, 1]
    assert len(next(iter(sf.batches([torch.tensor([0, 1, 1])], with_ids=True)))) == 4


def test_speech_ids_of_a_window_bank_follow_track_and_start():
    from speech_decoding_amd import data as D
    args = tiny_args(compute_dtype="bf16")
    feed, _, _ = D.synthetic_track_dataset(args, DEV, n_segments=20, dtype=torch.bfloat16, seed=1234)
    bank = feed.speech_bank()
    # a feed on the same tracks whose candidates 0 and 1 are one window (same track, same start), under two segment numbers
    twin = bank.select(np.array([5, 5, 6]))
    feed.Y = twin
    feed.seg_task, feed.seg_in_task = feed.seg_task[[5, 5, 6]], feed.seg_in_task[[5, 5, 6]]
    ids = feed.speech_ids([0, 1, 2])
    assert ids.dtype == np.int64 and ids[0] == ids[1] != ids[2]
    assert ids.tolist() == bank.starts_host[[5, 5, 6]].tolist()


def run_train(monkeypatch, tmp_path, **over):
    import train as T
    monkeypatch.chdir(tmp_path)
    args = tiny_args(**over)
    torch.manual_seed(0)
    np.random.seed(0)
    hist, _, lossf = T.run(args, log=lambda *a: None)
    return hist, lossf


@pytest.mark.parametrize("mode", LC.MODES)
def test_train_runs_with_repeats_in_every_batch(mode, tmp_path, monkeypatch):
    """10 training segments, batches of 12 drawn with replacement: every batch holds a repeat; the labelled loss and accuracies run"""
    from speech_decoding_amd import ops
    calls = {"counts": 0, "ranks": 0}
    real_counts, real_ranks = ops.clip_label_counts, ops.clip_ranks_labels
    monkeypatch.setattr(ops, "clip_label_counts", lambda *a, **k: (calls.__setitem__("counts", calls["counts"] + 1), real_counts(*a, **k))[1])
    monkeypatch.setattr(ops, "clip_ranks_labels", lambda *a, **k: (calls.__setitem__("ranks", calls["ranks"] + 1), real_ranks(*a, **k))[1])
    hist, lossf = run_train(monkeypatch, tmp_path, clip_duplicates=mode)
    assert lossf.duplicates == mode and len(hist) == 1
    assert np.isfinite(hist[0]["train_loss"]) and np.isfinite(hist[0]["test_loss"])
    assert calls["counts"] == 3 and calls["ranks"] == 3         # two training steps and the evaluation; the accuracies reuse them
    plain, _ = run_train(monkeypatch, tmp_path)
    if mode == "mask":
        assert hist[0]["train_loss"] != plain[0]["train_loss"]   # the repeats left the denominators: another loss
    else:
        # a feed's repeats have bit-identical speech rows, so l_aj == l_bj for a pair (a, b): the mean logit of the two positives
        # of a column is the logit of its own, and the multi-positive loss VALUE (and dZ) is the unlabelled one; what the labels
        # change here is the accuracies (and dY, where the speech side is trained)
        assert abs(hist[0]["train_loss"] - plain[0]["train_loss"]) <= 1e-5 * abs(plain[0]["train_loss"])
    assert hist[0]["trainTop1acc"] >= plain[0]["trainTop1acc"] - 1e-9 if mode == "positive" else True


def test_train_ignore_is_the_run_without_the_option(tmp_path, monkeypatch):
    from speech_decoding_amd import ops
    plain, _ = run_train(monkeypatch, tmp_path)

    def boom(*a, **k):
        raise AssertionError("clip_duplicates=ignore reached a labelled entry point")

    for name in ("clip_label_counts", "clip_logits_stats_masked", "clip_grad_labels", "clip_grad_y_labels", "clip_ranks_labels"):
        monkeypatch.setattr(ops, name, boom)
    ignore, _ = run_train(monkeypatch, tmp_path, clip_duplicates="ignore")
    assert ignore == plain                                      # the same launches: every figure of the history bit for bit


def test_train_refuses_the_option_it_cannot_serve(tmp_path, monkeypatch):
    import train as T
    with pytest.raises(ValueError, match="clip_duplicates"):
        T.run(tiny_args(clip_duplicates="positive", loss="mse"), log=lambda *a: None)
    with pytest.raises(ValueError, match="clip_duplicates"):
        T.run(tiny_args(clip_duplicates="sometimes"), log=lambda *a: None)
