"""Class-level decoding on the MI355X (retrieval.retrieve_classes; sda_retrieval_class_reduce / sda_retrieval_pool_rows).

Yardstick: tests/class_decode_cases.py — float64 on the fp32 cosine (kernel tests) or on the operands rounded to the compute
dtype (whole path), and the error bound derived there, which the CPU suite holds the fp32 emulation of the kernels to.  The
kernels alone must lie inside that bound; the whole path gets scale * TOL on top, TOL = 1e-4 being the project's exact-path
tolerance on the cosine (test_retrieval_gpu.py).  Selection over classes is checked to the bit against a CPU top-k of the
returned value matrix.  Every check prints its figure before it asserts.

MEASURED below: the largest share of its bound any value / row_lse used on the MI355X, per test family.
"""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from tests import class_decode_cases as K      # noqa: E402

DEV = "cuda:0"
DT = {"fp32": torch.float32, "bf16": torch.bfloat16, "fp16": torch.float16}
TOL = 1e-4
SMALL_SCRATCH = 64 << 10
SENTINEL = 12345.0
TEMP = K.SCALES[1]                 # exp(5.1), the loss's initial temperature
# largest |error| / bound seen on the MI355X (the checks below use 1.0, not these)
# kernels alone: share of the derived bound (values; row_lse reached 0.418); whole path: share of scale * TOL + bound, the largest
# |value - fp64 value| being 1.13e-4 (fp32, small scratch) at scale = exp(5.1)
MEASURED = {"kernel_small": 0.486, "kernel_large": 0.367, "pool_kernel": 0.380, "whole_path": 0.0116}

_ref = {}


def dev(a, dtype=None):
    t = torch.from_numpy(np.ascontiguousarray(a))
    return (t if dtype is None else t.to(dtype)).to(DEV)


def reference(case_name, case, scale, mode, groups=None):
    key = (case_name, scale, mode, None if groups is None else tuple(groups))
    if key not in _ref:
        want, lse = K.class_values64(case["cos"], case["order"], case["offsets"], scale, mode, groups)
        bound, b_lse = K.value_bound(case["cos"], case["order"], case["offsets"], scale, mode, groups)
        _ref[key] = (want, lse, bound, b_lse)
    return _ref[key]


def run_reduce(case, chunk, scale, mode, pitch=None):
    """The kernel on the case's chunk-major matrix, into a sentinel-filled output of the given pitch."""
    from speech_decoding_amd import ops
    n, M, C = case["n"], case["M"], case["C"]
    flat = dev(K.chunk_major(case["S"], chunk))
    pitch = K.pad64(C) if pitch is None else pitch
    out = torch.full((n, pitch), SENTINEL, dtype=torch.float32, device=DEV)
    got, lse = ops.retrieval_class_reduce(flat, dev(case["qsq"]), dev(case["csq"]), dev(case["order"]), dev(case["offsets"]),
                                          n, M, C, scale, mode, chunk, out=out)
    assert got is out
    return out.cpu().numpy(), lse.cpu().numpy()


def check_reduce(name, case_name, case, chunk, scale, mode, pitch=None):
    C = case["C"]
    want, lse, bound, b_lse = reference(case_name, case, scale, mode)
    out, got_lse = run_reduce(case, chunk, scale, mode, pitch)
    got = out[:, :C]
    r_val, r_lse = K.miss(got, want, bound), K.miss(got_lse, lse, b_lse)
    emu, emu_lse = K.emulate_reduce(K.chunk_major(case["S"], chunk), case["qsq"], case["csq"], case["order"], case["offsets"],
                                    case["n"], case["M"], chunk, scale, mode)
    same = float((emu.view(np.int32) == np.ascontiguousarray(got).view(np.int32)).mean())
    print(f"{name}: values use {r_val:.3f} of the bound, row_lse {r_lse:.3f}; {same:.3f} of the values equal the emulation's bits")
    assert not np.isnan(out).any() and not np.isnan(got_lse).any()
    assert (out[:, C:] == SENTINEL).all(), "padding columns were written"
    assert np.isneginf(got[:, np.diff(case["offsets"]) == 0]).all() and np.isfinite(got[:, np.diff(case["offsets"]) > 0]).all()
    assert r_val <= 1.0 and r_lse <= 1.0
    return max(r_val, r_lse)


# ---------------------------------------------------------------------------------------------------------------------------
# 1. the reduction kernel alone on a synthetic S
# ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("scale", K.SCALES)
@pytest.mark.parametrize("chunk", [256, 384, 1024])
def test_class_reduce_kernel_small(chunk, scale):
    """n = 5, M = 1000, C = 37 (class_decode_cases.small_case): four chunks of 256 (the last 232 wide at pitch 256), three of 384
    (the last at pitch 256, not 384) and the unchunked matrix."""
    case = K.small_case()
    for mode in K.MODES:
        check_reduce(f"small chunk {chunk} scale {scale:g} {mode}", "small", case, chunk, scale, mode)
    check_reduce(f"small chunk {chunk} scale {scale:g} sum, pitch 200", "small", case, chunk, scale, "sum", pitch=200)


@pytest.mark.parametrize("scale,mode", [(K.SCALES[1], "sum"), (K.SCALES[1], "mean"), (K.SCALES[2], "max"), (K.SCALES[0], "sum")])
def test_class_reduce_kernel_large(scale, mode):
    """n = 8, M = 20000, C = 3000 with Zipf-like counts, the largest class 4200 members."""
    case = K.large_case()
    assert np.diff(case["offsets"]).max() >= 4096
    check_reduce(f"large scale {scale:g} {mode}", "large", case, 8192, scale, mode)


def test_class_reduce_twice_gives_the_same_bits():
    case = K.large_case()
    a, la = run_reduce(case, 8192, TEMP, "sum")
    b, lb = run_reduce(case, 8192, TEMP, "sum")
    assert np.array_equal(a.view(np.int32), b.view(np.int32)) and np.array_equal(la.view(np.int32), lb.view(np.int32))


# ---------------------------------------------------------------------------------------------------------------------------
# 2. the pooling kernel alone
# ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("scale", K.SCALES)
def test_pool_rows_kernel(scale):
    from speech_decoding_amd import ops
    case = K.small_case()
    groups = [1, 0, 1, 2, 1]
    rows, goff = K.csr(groups, 3)
    C = case["C"]
    for mode in K.MODES:
        values, _ = run_reduce(case, 256, scale, mode)
        out = torch.full((3, 128), SENTINEL, dtype=torch.float32, device=DEV)
        ops.retrieval_pool_rows(dev(values), dev(rows), dev(goff), 5, 3, C, out=out)
        got = out.cpu().numpy()
        want, _, bound, _ = reference("small", case, scale, mode, groups)
        r = K.miss(got[:, :C], want, bound)
        print(f"pool scale {scale:g} {mode}: pooled values use {r:.3f} of the bound")
        assert not np.isnan(got).any() and (got[:, C:] == SENTINEL).all()
        assert np.isneginf(got[:, :C][:, np.diff(case["offsets"]) == 0]).all()           # empty in every row: -inf, not NaN
        assert r <= 1.0
        assert np.array_equal(got[0, :C].view(np.int32), np.ascontiguousarray(values[1, :C]).view(np.int32))   # a group of one row is that row


# ---------------------------------------------------------------------------------------------------------------------------
# 3. the whole path
# ---------------------------------------------------------------------------------------------------------------------------
def path_reference(shape, dtype, scale, mode, groups=None):
    key = ("path", shape, dtype, scale, mode, None if groups is None else tuple(groups))
    if key not in _ref:
        p = K.path_case(shape)
        ckey = ("cos", shape, dtype)
        if ckey not in _ref:
            _ref[ckey] = K.cosine64_of(p["queries"], p["bank"], DT[dtype])
        cos = _ref[ckey]
        order, offsets = K.csr(p["ids"], p["C"])
        want, _ = K.class_values64(cos, order, offsets, scale, mode, groups)
        bound, _ = K.value_bound(cos, order, offsets, scale, mode, groups)
        _ref[key] = (want, bound + np.float32(scale) * TOL * np.isfinite(want))
    return _ref[key]


def run_path(shape, dtype, scale=TEMP, mode="sum", k=10, groups=None, labels="classes", **kw):
    from speech_decoding_amd import ClassIndex, SpeechBank, retrieve_classes
    p = K.path_case(shape)
    bank = SpeechBank.from_tensor(p["bank"].to(DEV), dtype=DT[dtype])
    if isinstance(labels, str):
        labels = torch.from_numpy(p["ids"])[p["labels"]].to(DEV)
    index = ClassIndex(p["ids"], num_classes=p["C"], device=DEV)         # the last class has no member: C is not max id + 1
    return retrieve_classes(p["queries"].to(DEV), bank, index, k=k, scale=scale, reduce=mode, labels=labels, groups=groups, **kw)


def expected_selection(matrix, labels, k):
    """CPU: a stable sort by (-value, class id) and a plain count, on the returned matrix itself."""
    v = matrix + 0.0
    order = torch.sort(-v, dim=1, stable=True).indices[:, :k]
    R, C = v.shape
    vl = v[torch.arange(R), labels][:, None]
    j = torch.arange(C)[None, :]
    ranks = ((v > vl) | ((v == vl) & (j < labels[:, None]))).sum(dim=1).to(torch.int32)
    return order, torch.gather(v, 1, order), ranks


def check_selection(res, labels, k):
    m = res.matrix.cpu()
    assert not torch.isnan(m).any()
    want_idx, want_val, want_rank = expected_selection(m, labels, k)
    assert res.classes.dtype == torch.int64 and res.log_probs.dtype == torch.float32 and res.ranks.dtype == torch.int32
    assert torch.equal(res.classes.cpu(), want_idx)
    assert torch.equal(res.log_probs.cpu().view(torch.int32), want_val.view(torch.int32))          # bits, not values
    assert torch.equal(res.ranks.cpu(), want_rank)


def check_ranks(ranks, ref, tol, labels):
    """#{c : v_c > v_l + 2 tol} <= rank <= #{c != l : v_c >= v_l - 2 tol} in float64 (test_retrieval_gpu.check_ranks)."""
    R, C = ref.shape
    t = 2 * float(tol[np.isfinite(ref)].max())
    vl = ref[np.arange(R), labels][:, None]
    lo = (ref > vl + t).sum(axis=1)
    other = np.arange(C)[None, :] != labels[:, None]
    hi = ((ref >= vl - t) & other).sum(axis=1)
    r = ranks.cpu().numpy()
    assert (lo <= r).all() and (r <= hi).all(), (lo.tolist(), r.tolist(), hi.tolist())


@pytest.mark.parametrize("scratch", [1 << 30, SMALL_SCRATCH])
@pytest.mark.parametrize("dtype", ["fp32", "bf16", "fp16"])
@pytest.mark.parametrize("shape", ["a", "b"])
def test_whole_path_against_fp64(shape, dtype, scratch):
    from speech_decoding_amd import lib as L
    from speech_decoding_amd.retrieval import plan_class_blocks
    p = K.path_case(shape)
    if scratch == SMALL_SCRATCH:
        nb, mc, _, _ = plan_class_blocks(p["N"], p["M"], p["C"], L.rows_tp(p["T"]) * L.pad_channels(p["F"]), DT[dtype], scratch)
        assert nb < p["N"] and mc < p["M"]                 # several query blocks and bank chunks
    res = run_path(shape, dtype, return_matrix=True, scratch_bytes=scratch)
    want, tol = path_reference(shape, dtype, TEMP, "sum")
    got = res.matrix.cpu().numpy()
    assert got.shape == want.shape and res.matrix.is_cuda and res.classes.is_cuda and res.ranks.is_cuda
    r = K.miss(got, want, tol)
    fin = np.isfinite(want)
    print(f"{K.SHAPES[shape]} {dtype} scratch {scratch}: max |value - fp64| {np.abs(got[fin] - want[fin]).max():.3e}, {r:.4f} of the tolerance")
    assert r <= 1.0
    true = p["ids"][p["labels"].numpy()]
    check_selection(res, torch.from_numpy(true), 10)
    check_ranks(res.ranks, want, tol, true)
    lp = np.exp(got.astype(np.float64)).sum(axis=1)
    assert np.abs(lp - 1.0).max() < 1e-3                   # "sum": log-probabilities over the classes
    # the planted words: the float64 yardstick itself puts every one of them first
    assert (want.argmax(axis=1) == true).all()
    assert res.accuracy(1) == res.accuracy(10) == 1.0


@pytest.mark.parametrize("mode", ["mean", "max"])
@pytest.mark.parametrize("scale", [1.0, 1000.0])
def test_whole_path_other_modes_and_scales(mode, scale):
    res = run_path("b", "bf16", scale=scale, mode=mode, k=64, return_matrix=True, scratch_bytes=SMALL_SCRATCH)
    want, tol = path_reference("b", "bf16", scale, mode)
    r = K.miss(res.matrix.cpu().numpy(), want, tol)
    print(f"{mode} at scale {scale:g}: {r:.4f} of the tolerance")
    assert r <= 1.0
    p = K.path_case("b")
    check_selection(res, torch.from_numpy(p["ids"][p["labels"].numpy()]), 64)


def test_without_matrix_and_without_labels():
    full = run_path("a", "bf16", return_matrix=True, scratch_bytes=SMALL_SCRATCH)
    lean = run_path("a", "bf16", scratch_bytes=SMALL_SCRATCH)
    assert lean.matrix is None
    assert torch.equal(lean.classes, full.classes) and torch.equal(lean.log_probs, full.log_probs) and torch.equal(lean.ranks, full.ranks)
    bare = run_path("a", "bf16", labels=None)
    assert bare.ranks is None and bare.matrix is None and torch.equal(bare.classes, full.classes)
    with pytest.raises(ValueError):
        bare.accuracy(1)


# ---------------------------------------------------------------------------------------------------------------------------
# 4. selection exactness on deliberate ties
# ---------------------------------------------------------------------------------------------------------------------------
def test_selection_is_exact_on_tied_classes():
    """Two identical candidates in two singleton classes give two equal class values; three classes are empty (-inf ties)."""
    from speech_decoding_amd import ClassIndex, SpeechBank, retrieve_classes
    g = torch.Generator().manual_seed(5)
    M, N, F, T = 64, 6, 8, 10
    bank = torch.randn(M, F, T, generator=g)
    bank[9] = bank[5]
    bank[40] = bank[5]
    ids = np.arange(M) % 20
    ids[5], ids[9], ids[40] = 21, 20, 23                              # classes 20, 21, 23: one copy each; 22, 24, 25 empty
    index = ClassIndex(ids, num_classes=26, device=DEV)
    queries = torch.randn(N, F, T, generator=g)
    queries[0] = bank[5]                                              # the tied classes lead row 0
    labels = torch.tensor([21, 20, 23, 22, 0, 25])
    b = SpeechBank.from_tensor(bank.to(DEV), dtype=torch.float32)
    for mode in K.MODES:
        res = retrieve_classes(queries.to(DEV), b, index, k=26, scale=TEMP, reduce=mode, labels=labels, return_matrix=True)
        m = res.matrix.cpu()
        assert torch.equal(m[:, 20], m[:, 21]) and torch.equal(m[:, 20], m[:, 23])
        assert torch.isneginf(m[:, [22, 24, 25]]).all() and torch.isfinite(m[:, :22]).all()
        check_selection(res, labels, 26)
        assert res.classes[0, :3].tolist() == [20, 21, 23]            # equal values: the lower class id first
        assert res.classes[:, -3:].tolist() == [[22, 24, 25]] * N     # classes without a member come last, in id order
        assert int(res.ranks[0]) == 1 and int(res.ranks[3]) == 23 and int(res.ranks[5]) == 25


# ---------------------------------------------------------------------------------------------------------------------------
# 5. pooling repeated queries
# ---------------------------------------------------------------------------------------------------------------------------
def interleaved_groups(N):
    """Groups of sizes 1, 2 and 7 (in turn) dealt over N = 40 queries by a fixed permutation: members of one group lie
    far apart, in different query blocks."""
    sizes, g = [], 0
    while sum(sizes) < N:
        sizes.append((1, 2, 7)[g % 3]); g += 1
    ids = np.repeat(np.arange(len(sizes)), sizes)[:N]
    return ids[np.random.default_rng(11).permutation(N)]


@pytest.mark.parametrize("dtype", ["fp32", "bf16"])
def test_pooling_groups_against_fp64(dtype):
    p = K.path_case("b")
    groups = interleaved_groups(p["N"])
    G = int(groups.max()) + 1
    assert sorted(set(np.bincount(groups).tolist())) == [1, 2, 7] and (np.bincount(groups) > 0).all()
    glabels = torch.from_numpy(np.arange(G) % p["C"])
    res = run_path("b", dtype, groups=groups, labels=glabels, return_matrix=True, scratch_bytes=SMALL_SCRATCH)
    want, tol = path_reference("b", dtype, TEMP, "sum", groups)
    got = res.matrix.cpu().numpy()
    assert got.shape == (G, p["C"]) and res.classes.shape == (G, 10) and res.ranks.shape == (G,)
    r = K.miss(got, want, tol)
    print(f"pooled {dtype}: {r:.4f} of the tolerance")
    assert r <= 1.0
    empty = np.bincount(p["ids"], minlength=p["C"]) == 0
    assert empty.any() and np.isneginf(got[:, empty]).all() and not np.isnan(got).any()
    check_selection(res, glabels, 10)
    check_ranks(res.ranks, want, tol, glabels.numpy())
    # the same groups handed over as a device tensor and as a list
    again = run_path("b", dtype, groups=torch.from_numpy(groups).to(DEV), labels=glabels, return_matrix=True, scratch_bytes=SMALL_SCRATCH)
    assert all(torch.equal(x, y) for x, y in zip(res, again))


def test_groups_of_one_equal_no_groups():
    p = K.path_case("b")
    plain = run_path("b", "bf16", return_matrix=True)
    single = run_path("b", "bf16", groups=np.arange(p["N"]), return_matrix=True)
    assert all(torch.equal(x, y) for x, y in zip(plain, single))
    perm = np.random.default_rng(2).permutation(p["N"])                # group g = query perm^-1(g): the rows come back permuted
    moved = run_path("b", "bf16", groups=perm, labels=None, return_matrix=True)
    assert torch.equal(moved.matrix[torch.from_numpy(perm).to(DEV)], plain.matrix)


# ---------------------------------------------------------------------------------------------------------------------------
# 6. determinism, device labels, Classifier.decode_classes
# ---------------------------------------------------------------------------------------------------------------------------
def test_same_call_same_bits():
    p = K.path_case("a")
    groups = np.arange(p["N"]) % 17
    labels = torch.from_numpy(np.arange(17))
    a = run_path("a", "bf16", groups=groups, labels=labels, return_matrix=True, scratch_bytes=SMALL_SCRATCH)
    b = run_path("a", "bf16", groups=groups, labels=labels, return_matrix=True, scratch_bytes=SMALL_SCRATCH)
    assert all(torch.equal(x, y) for x, y in zip(a, b))
    c, d = run_path("a", "fp32", mode="max"), run_path("a", "fp32", mode="max")
    assert torch.equal(c.classes, d.classes) and torch.equal(c.log_probs, d.log_probs) and torch.equal(c.ranks, d.ranks)


def test_host_and_device_labels_and_a_label_outside_the_classes():
    from speech_decoding_amd import SpeechBank, retrieve_classes
    p = K.path_case("b")
    true = torch.from_numpy(p["ids"])[p["labels"]]
    on_dev = run_path("b", "bf16", labels=true.to(DEV))
    for host in (true, true.tolist(), true.numpy().astype(np.int32)):
        assert torch.equal(run_path("b", "bf16", labels=host).ranks, on_dev.ranks)
    outside = true.clone()
    outside[3] = p["C"]
    with pytest.raises(IndexError):
        run_path("b", "bf16", labels=outside)
    r = run_path("b", "bf16", labels=outside.to(DEV)).ranks           # device labels: nothing is read back, the kernel flags it
    assert int(r[3]) == -1 and torch.equal(r[:3], on_dev.ranks[:3]) and torch.equal(r[4:], on_dev.ranks[4:])


def test_classifier_decode_classes_delegates():
    from speech_decoding_amd import ClassIndex, SpeechBank, retrieve_classes
    from speech_decoding.models import Classifier
    p = K.path_case("b")
    bank = SpeechBank.from_tensor(p["bank"].to(DEV))
    index = ClassIndex(p["ids"], num_classes=p["C"], device=DEV)
    assert index.order_dev.is_cuda and index.order_dev.dtype == torch.int32 and index.offsets_dev.numel() == p["C"] + 1
    Z = p["queries"].to(DEV)
    true = torch.from_numpy(p["ids"])[p["labels"]]
    a = Classifier().decode_classes(Z, bank, index, k=7, scale=TEMP, labels=true)
    b = retrieve_classes(Z, bank, index, k=7, scale=TEMP, labels=true)
    assert a.matrix is None and b.matrix is None
    assert all(torch.equal(x, y) for x, y in zip(a[:3], b[:3]))
    assert a.accuracy(1) == 1.0
