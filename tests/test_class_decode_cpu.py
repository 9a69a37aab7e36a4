"""CPU checks of class-level decoding (retrieval.ClassIndex / retrieve_classes, sda_retrieval_class_reduce,
sda_retrieval_pool_rows): the entry points are declared, exported and bound and refuse bad arguments without a launch; the
index build and every argument error; the extended blocking plan; and the arithmetic's yardsticks themselves — the fp32
emulation of the kernels' summation order stays inside the derived bound (class_decode_cases.py) on every shared case, and each
planted bug misses that bound by at least 10x.  No kernel is launched."""
import ctypes
import math
import os
import re

import numpy as np
import pytest
import torch

from tests import class_decode_cases as K

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = ("sda_retrieval_class_reduce", "sda_retrieval_pool_rows")


@pytest.fixture(scope="module")
def lib():
    from speech_decoding_amd import lib as L
    if not os.path.exists(L.LIB_PATH):
        import __graft_entry__ as g
        g.build()
    return L


def test_new_symbols_are_declared_exported_and_bound(lib):
    header = open(os.path.join(ROOT, "include", "sd_amd.h")).read()
    code = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    cdll = ctypes.CDLL(lib.LIB_PATH)
    for name in NEW_SYMBOLS:
        assert re.search(r"\b%s\s*\(" % name, code), f"{name} not declared in sd_amd.h"
        assert hasattr(cdll, name), f"{name} not exported"
        assert name in lib.SIGNATURES
    assert lib.load().sda_abi_version() == lib.ABI_VERSION == 4        # additions only: the ABI version stays
    import speech_decoding_amd as A
    from speech_decoding_amd import ops, retrieval
    assert A.ClassIndex is retrieval.ClassIndex and A.retrieve_classes is retrieval.retrieve_classes
    assert A.ClassRetrieval is retrieval.ClassRetrieval
    assert {"ClassIndex", "ClassRetrieval", "retrieve_classes"} <= set(A.__all__)
    assert callable(ops.retrieval_class_reduce) and callable(ops.retrieval_pool_rows) and callable(A.Classifier.decode_classes)
    assert "result-sized" in retrieval.retrieve_classes.__doc__


def test_entry_points_refuse_bad_arguments_without_launch(lib):
    L = lib.load()
    one = ctypes.c_void_p(64)            # a non-null, 16-byte aligned address that is never dereferenced: every call below is refused
    good = dict(pitch=64, n=4, M=100, C=37, chunk=128, scale=1.0, mode=0)

    def reduce(ptrs=None, **kw):
        a = dict(good, **kw)
        p = [one] * 7 if ptrs is None else ptrs
        return L.sda_retrieval_class_reduce(*p, a["pitch"], a["n"], a["M"], a["C"], a["chunk"], a["scale"], a["mode"], None)

    assert reduce([None] * 7) == -1 and b"null" in L.sda_last_error()
    for missing in range(7):             # S, qsq, csq, order, offsets, out, row_lse
        p = [one] * 7
        p[missing] = None
        assert reduce(p) == -1 and b"null" in L.sda_last_error()
    for kw in (dict(n=0), dict(n=-3), dict(M=0), dict(C=0), dict(C=-1)):
        assert reduce(**kw) == -1 and b">= 1" in L.sda_last_error()
    for chunk in (0, 100, -64):
        assert reduce(chunk=chunk) == -1 and b"chunk_cols" in L.sda_last_error()
    assert reduce([ctypes.c_void_p(68)] + [one] * 6) == -1 and b"aligned" in L.sda_last_error()          # S: 16 bytes
    assert reduce([one] * 5 + [ctypes.c_void_p(66), one]) == -1 and b"aligned" in L.sda_last_error()     # out: 4 bytes
    assert reduce(pitch=36) == -1 and b"pitch" in L.sda_last_error()
    for scale in (0.0, -1.0, math.inf, math.nan):
        assert reduce(scale=scale) == -1 and b"scale" in L.sda_last_error()
    for mode in (-1, 3, 100):
        assert reduce(mode=mode) == -1 and b"mode" in L.sda_last_error()

    def pool(ptrs=None, v_pitch=64, out_pitch=64, N=9, G=3, C=37):
        p = [one] * 4 if ptrs is None else ptrs
        return L.sda_retrieval_pool_rows(p[0], v_pitch, p[1], p[2], p[3], out_pitch, N, G, C, None)

    for missing in range(4):             # V, rows, group_offsets, out
        p = [one] * 4
        p[missing] = None
        assert pool(p) == -1 and b"null" in L.sda_last_error()
    for kw in (dict(N=0), dict(G=0), dict(C=0), dict(G=-2)):
        assert pool(**kw) == -1 and b">= 1" in L.sda_last_error()
    assert pool(v_pitch=36) == -1 and b"pitch" in L.sda_last_error()
    assert pool(out_pitch=36) == -1 and b"pitch" in L.sda_last_error()
    assert pool([one, ctypes.c_void_p(66), one, one]) == -1 and b"aligned" in L.sda_last_error()
    assert pool(G=1 << 30, C=1 << 20, v_pitch=1 << 20, out_pitch=1 << 20) == -1 and b"grid" in L.sda_last_error()


# ---------------------------------------------------------------------------------------------------------------------------
# ClassIndex and retrieve_classes' arguments
# ---------------------------------------------------------------------------------------------------------------------------
def test_class_index_order_offsets_stability_and_empty_classes():
    from speech_decoding_amd import ClassIndex
    ids = [3, 0, 3, 5, 0, 3, 1]
    for given in (ids, np.array(ids, dtype=np.int16), np.array(ids, dtype=np.uint8), torch.tensor(ids)):
        ix = ClassIndex(given)
        assert (ix.M, ix.C, len(ix)) == (7, 6, 7)
        assert ix.order.dtype == np.int32 and ix.order.tolist() == [1, 4, 6, 0, 2, 5, 3]      # ascending bank index inside a class
        assert ix.offsets.dtype == np.int32 and ix.offsets.tolist() == [0, 2, 3, 3, 6, 6, 7]  # classes 2 and 4 are empty
        assert ix.counts.tolist() == [2, 1, 0, 3, 0, 1]
    ix = ClassIndex(ids, num_classes=9)                                                    # trailing empty classes
    assert ix.C == 9 and ix.offsets.tolist() == [0, 2, 3, 3, 6, 6, 7, 7, 7, 7]
    rng = np.random.default_rng(3)
    big = rng.integers(0, 50, size=5000)
    ix = ClassIndex(big, num_classes=64)
    order, offsets = K.csr(big, 64)
    assert np.array_equal(ix.order, order) and np.array_equal(ix.offsets, offsets)
    for c in range(64):
        seg = ix.order[ix.offsets[c]: ix.offsets[c + 1]]
        assert (big[seg] == c).all() and (np.diff(seg) > 0).all()


def test_class_index_errors():
    from speech_decoding_amd import ClassIndex
    for bad in ([0.5, 1.0], np.array([1.0, 2.0]), torch.tensor([1.0]), ["a", "b"], [True, False], [], [[0, 1], [1, 0]]):
        with pytest.raises(ValueError):
            ClassIndex(bad)
    with pytest.raises(ValueError, match="negative"):
        ClassIndex([0, -1, 2])
    with pytest.raises(ValueError, match="outside"):
        ClassIndex([0, 1, 5], num_classes=5)
    for bad in (0, -2, 2.5, True):
        with pytest.raises(ValueError):
            ClassIndex([0, 1], num_classes=bad)


def test_argument_errors_come_before_the_device(lib):
    from speech_decoding_amd import ClassIndex, SpeechBank, retrieve_classes
    bank = SpeechBank(8, 5)
    Q = torch.zeros(4, 8, 5)
    with pytest.raises(ValueError, match="empty"):
        retrieve_classes(Q, bank, [0, 1])
    bank._size = 20                      # stands for a filled bank
    ids = np.arange(20) % 6
    with pytest.raises(ValueError):
        retrieve_classes(Q, "bank", ids)
    for bad in (torch.zeros(2, 9, 5), torch.zeros(2, 8, 4), torch.zeros(8, 5), torch.zeros(0, 8, 5)):
        with pytest.raises(ValueError):
            retrieve_classes(bad, bank, ids)
    for bad_ids in (ids[:19], ClassIndex(np.arange(21) % 6), [0.5] * 20, [-1] + [0] * 19):
        with pytest.raises(ValueError):
            retrieve_classes(Q, bank, bad_ids)
    for k in (0, -3, 65, 7, 2.5, True):  # 1 ... min(64, C = 6)
        with pytest.raises(ValueError):
            retrieve_classes(Q, bank, ids, k=k)
    for scale in (0.0, -1.0, float("inf"), float("nan"), 1e39, "1", None, True):
        with pytest.raises(ValueError, match="scale"):
            retrieve_classes(Q, bank, ids, k=3, scale=scale)
    with pytest.raises(ValueError, match="reduce"):
        retrieve_classes(Q, bank, ids, k=3, reduce="median")
    for groups in ([0, 1, 3, 3], [0, 0, 2, 2], [0, 1], [0.0, 1.0, 0.0, 1.0], [-1, 0, 0, 0]):      # group 2 / 1 empty, wrong length, ...
        with pytest.raises(ValueError):
            retrieve_classes(Q, bank, ids, k=3, groups=groups)
    for labels in ([0, 6, 1, 2], [-1, 3, 0, 0], torch.tensor([5, 99, 0, 0]), np.array([6, 0, 0, 0])):
        with pytest.raises(IndexError):
            retrieve_classes(Q, bank, ids, k=3, labels=labels)
    for labels in ([1, 2, 3], [0.5, 1.0, 0.0, 0.0], torch.zeros(4, 1, dtype=torch.int64)):
        with pytest.raises(ValueError):
            retrieve_classes(Q, bank, ids, k=3, labels=labels)
    with pytest.raises(ValueError):      # with groups the labels are per group
        retrieve_classes(Q, bank, ids, k=3, groups=[0, 1, 0, 1], labels=[0, 1, 2, 3])
    with pytest.raises(IndexError):
        retrieve_classes(Q, bank, ids, k=3, groups=[0, 1, 0, 1], labels=[0, 6])
    with pytest.raises(ValueError, match="scratch"):
        retrieve_classes(Q, bank, ids, k=3, scratch_bytes=8 * 64 + 4 * 64)          # the scores fit twice, the class values do not


def test_cpu_tensors_are_refused(lib):
    from speech_decoding_amd import ClassIndex, SdaError, SpeechBank, retrieve_classes
    from speech_decoding_amd.models import Classifier
    bank = SpeechBank(8, 5)
    bank._size = 20                      # stands for a filled bank: the device check comes after every argument check
    ids = np.arange(20) % 6
    with pytest.raises(SdaError):
        retrieve_classes(torch.zeros(2, 8, 5), bank, ids, k=5)
    with pytest.raises(SdaError):
        retrieve_classes(torch.zeros(4, 8, 5), bank, ClassIndex(ids), k=5, labels=[3, 1], groups=[0, 1, 1, 0], return_matrix=True)
    with pytest.raises(SdaError):
        Classifier().decode_classes(torch.zeros(2, 8, 5), bank, ids, k=2, scale=164.0, reduce="max")
    with pytest.raises(SdaError):
        ClassIndex(ids, device="cpu").order_dev


# ---------------------------------------------------------------------------------------------------------------------------
# the blocking plan
# ---------------------------------------------------------------------------------------------------------------------------
PLAN_CASES = [(96, 1000, 6784, 64 << 10), (96, 1000, 6784, 1 << 30), (1, 1000, 6784, 1 << 20), (40, 300, 4224, 32 << 10),
              (256, 32768, 385024, 1 << 30), (256, 32768, 385024, 64 << 20), (1000, 4096, 385024, 8 << 20)]
# plan_blocks(N, M, K, dtype, scratch) of the commit before class decoding, bf16 / fp16 (fp32 differs in tiles256 / ksplit only
# through ops.splitk_plan, which is untouched): recorded from that commit's code
OLD_PLAN_NB_MC = {(96, 1000, 6784, 64 << 10): (8, 256), (96, 1000, 6784, 1 << 30): (96, 1024)}


def test_extended_plan_keeps_the_memory_bound(lib):
    from speech_decoding_amd import lib as L
    from speech_decoding_amd.retrieval import plan_blocks, plan_class_blocks
    lib.load()
    for dtype in (torch.float32, torch.bfloat16, torch.float16):
        for N, M, Kk, scratch in PLAN_CASES:
            for C in (1, 37, M // 8, M, 3 * M):
                if scratch < 8 * (L.pad_channels(M) + L.pad_channels(C)):
                    with pytest.raises(ValueError):
                        plan_class_blocks(N, M, C, Kk, dtype, scratch)
                    continue
                nb, mc, tiles256, ks = plan_class_blocks(N, M, C, Kk, dtype, scratch)
                assert plan_class_blocks(N, M, C, Kk, dtype, scratch) == (nb, mc, tiles256, ks)
                assert 1 <= nb <= N and mc % 64 == 0 and (mc >= M or mc % 256 == 0 or dtype == torch.float32)
                slab = 32 if (tiles256 or dtype == torch.float32) else 64
                assert 1 <= ks <= Kk // slab
                used = 4 * nb * (L.pad_channels(M) + L.pad_channels(C)) + (4 * ks * nb * mc if ks > 1 else 0)
                assert used <= scratch, (N, M, C, Kk, scratch, dtype, nb, mc, ks, used)
    nb, mc, _, _ = plan_class_blocks(96, 1000, 333, 6784, torch.bfloat16, 64 << 10)
    assert nb < 96 and mc < 1000          # the setting the GPU suite uses to force several query blocks and bank chunks


def test_old_plan_is_unchanged(lib):
    """plan_blocks as called before: the formula of the previous commit, restated here, on the existing suite's cases."""
    from speech_decoding_amd import lib as L, ops
    from speech_decoding_amd.retrieval import plan_blocks
    lib.load()

    def previous(N, M, Kk, dtype, scratch_bytes):
        Mp = L.pad_channels(M)
        nb = min(N, scratch_bytes // 2 // (4 * Mp))
        if nb >= 256:
            nb = nb // 256 * 256
        budget = scratch_bytes - 4 * nb * Mp
        mc = Mp
        if dtype == torch.float32:
            mc = min(mc, max(64, ((1 << 31) // (4 * Kk)) // 64 * 64))
        while True:
            tiles256, ks = ops.splitk_plan(dtype, nb, min(mc, M), Kk, Kk)
            if ks == 1 or 4 * ks * nb * mc <= budget or mc <= 256:
                break
            mc = max(256, (mc // 2 + 255) // 256 * 256)
        return nb, mc, tiles256, max(1, min(ks, budget // (4 * nb * mc)))

    for dtype in (torch.float32, torch.bfloat16, torch.float16):
        for case in PLAN_CASES:
            assert plan_blocks(*case[:3], dtype, case[3]) == previous(*case[:3], dtype, case[3])
    for case, want in OLD_PLAN_NB_MC.items():
        assert plan_blocks(*case[:3], torch.bfloat16, case[3])[:2] == want
    with pytest.raises(ValueError, match="retrieve:"):
        plan_blocks(2, 20, 4224, torch.bfloat16, 16)


# ---------------------------------------------------------------------------------------------------------------------------
# the emulation against the bound, and the planted bugs
# ---------------------------------------------------------------------------------------------------------------------------
GROUPS5 = [1, 0, 1, 2, 1]                # rows of the small case in interleaved groups of 1, 3 and 1 rows
GROUPS8 = [0, 1, 0, 2, 2, 0, 2, 2]


def reduce_cases():
    """(name, case, chunk_cols, scale, mode) of everything the emulation is held to."""
    s, big = K.small_case(), K.large_case()
    out = [(f"small/{ch}/{sc:g}/{mode}", s, ch, sc, mode) for ch in s["chunks"] for sc in K.SCALES for mode in K.MODES]
    out += [(f"large/{sc:g}/{mode}", big, 8192, sc, mode) for sc, mode in ((K.SCALES[1], "sum"), (K.SCALES[1], "mean"),
                                                                          (K.SCALES[2], "max"), (K.SCALES[0], "sum"))]
    return out


def emulated(case, chunk, scale, mode, bug=None):
    flat = K.chunk_major(case["S"], chunk)
    return K.emulate_reduce(flat, case["qsq"], case["csq"], case["order"], case["offsets"], case["n"], case["M"], chunk, scale, mode, bug)


def test_emulation_stays_inside_the_bound_on_every_case():
    worst = 0.0
    for name, case, chunk, scale, mode in reduce_cases():
        want, lse = K.class_values64(case["cos"], case["order"], case["offsets"], scale, mode)
        bound, b_lse = K.value_bound(case["cos"], case["order"], case["offsets"], scale, mode)
        got, got_lse = emulated(case, chunk, scale, mode)
        r_val, r_lse = K.miss(got, want, bound), K.miss(got_lse, lse, b_lse)
        print(f"{name}: values use {r_val:.3f} of the bound, row_lse {r_lse:.3f}")
        assert r_val <= 1.0 and r_lse <= 1.0, name
        assert np.isneginf(got[:, np.diff(case["offsets"]) == 0]).all()
        worst = max(worst, r_val, r_lse)
        groups = GROUPS5 if case["n"] == 5 else GROUPS8
        wantp, _ = K.class_values64(case["cos"], case["order"], case["offsets"], scale, mode, groups)
        boundp, _ = K.value_bound(case["cos"], case["order"], case["offsets"], scale, mode, groups)
        r_pool = K.miss(K.emulate_pool(got, groups), wantp, boundp)
        print(f"{name}: pooled values use {r_pool:.3f} of the bound")
        assert r_pool <= 1.0, name
        worst = max(worst, r_pool)
    # the bound is not padded: the emulation's worst case uses at least a quarter of it (no more than 4x slack)
    assert worst >= 0.25, worst


def worst_miss(bug, scales=K.SCALES, modes=K.MODES, chunks=None):
    s = K.small_case()
    worst = 0.0
    for chunk in (chunks or s["chunks"]):
        for scale in scales:
            for mode in modes:
                want, _ = K.class_values64(s["cos"], s["order"], s["offsets"], scale, mode)
                bound, _ = K.value_bound(s["cos"], s["order"], s["offsets"], scale, mode)
                worst = max(worst, K.miss(emulated(s, chunk, scale, mode, bug)[0], want, bound))
    return worst


@pytest.mark.parametrize("bug,kw", [
    ("row_max", dict(scales=(1000.0,))),                   # classes far below the row's best underflow to -inf
    ("no_scale", dict(scales=K.SCALES[1:])),
    ("mean_no_logn", dict(modes=("mean",))),
    ("drop_last", {}), ("take_next", {}), ("order_ignored", {}),
    ("last_pitch", dict(chunks=(384,))),                   # three chunks, the last 232 columns wide at pitch 256, not 384
])
def test_planted_reduce_bug_misses_the_bound_tenfold(bug, kw):
    assert worst_miss(None, **kw) <= 1.0
    assert worst_miss(bug, **kw) >= 10.0


def test_last_pitch_bug_shows_where_the_last_chunk_is_narrower():
    """With chunk_cols = 256 the last chunk of M = 1000 is 232 columns wide at pitch pad64(232) = 256 = chunk_cols, so a kernel
    that takes chunk_cols for every pitch reads the same addresses; the shared case therefore also runs in chunks of 384, whose
    last chunk (232 wide, pitch 256) is where that bug shows."""
    s = K.small_case()
    assert K.pad64(1000 - 3 * 256) == 256 and K.pad64(1000 - 2 * 384) == 256 != 384 and 384 in s["chunks"]
    want, _ = K.class_values64(s["cos"], s["order"], s["offsets"], 1.0, "sum")
    bound, _ = K.value_bound(s["cos"], s["order"], s["offsets"], 1.0, "sum")
    assert K.miss(emulated(s, 256, 1.0, "sum", "last_pitch")[0], want, bound) <= 1.0
    want, _ = K.class_values64(s["cos"], s["order"], s["offsets"], 1.0, "sum")
    bound, _ = K.value_bound(s["cos"], s["order"], s["offsets"], 1.0, "sum")
    assert K.miss(emulated(s, 384, 1.0, "sum")[0], want, bound) <= 1.0
    assert K.miss(emulated(s, 384, 1.0, "sum", "last_pitch")[0], want, bound) >= 10.0


@pytest.mark.parametrize("bug", ["arith_mean", "nan_on_empty"])
def test_planted_pool_bug_misses_the_bound_tenfold(bug):
    s = K.small_case()
    scale = K.SCALES[1]
    got, _ = emulated(s, 256, scale, "sum")
    want, _ = K.class_values64(s["cos"], s["order"], s["offsets"], scale, "sum", GROUPS5)
    bound, _ = K.value_bound(s["cos"], s["order"], s["offsets"], scale, "sum", GROUPS5)
    assert K.miss(K.emulate_pool(got, GROUPS5), want, bound) <= 1.0
    assert K.miss(K.emulate_pool(got, GROUPS5, bug), want, bound) >= 10.0
