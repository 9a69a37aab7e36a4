"""CPU checks of decoding against windows of continuous speech tracks (retrieval.WindowBank, sda_sim_gemm_windows,
sda_window_sumsq): the new C entry points are declared, exported and bound and refuse bad arguments without a launch; WindowBank
validates its arguments before touching the device, in the order _ScorePass keeps, and refuses fp32 storage and CPU tensors; the
memory figure is arithmetic; and the numpy restatement the GPU tests lean on (window_bank_cases.restate) reproduces a float64
brute force on the integer cases and tells every planted bug apart.  No kernel is launched."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

from tests import window_bank_cases as W

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = ("sda_sim_gemm_windows", "sda_sim_gemm_windows_span", "sda_window_sumsq")
BF16, F16, F32 = 1, 2, 0


@pytest.fixture(scope="module")
def lib():
    from speech_decoding_amd import lib as L
    if not os.path.exists(L.LIB_PATH):
        import __graft_entry__ as g
        g.build()
    return L


def test_new_symbols_are_declared_exported_bound_and_reexported(lib):
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
    assert A.WindowBank is retrieval.WindowBank and "WindowBank" in A.__all__
    assert callable(ops.sim_gemm_windows_into) and callable(ops.window_sumsq)
    for doc in (A.Classifier.decode.__doc__, A.Classifier.decode_classes.__doc__):
        assert "SpeechBank" in doc and "WindowBank" in doc


def gemm_args(**kw):
    """A call of sda_sim_gemm_windows that would be served (2 queries against 3 windows of case a's shape), on addresses that are
    never dereferenced: every call the tests make with it is refused before a launch."""
    one = ctypes.c_void_p(64)
    a = dict(X=one, x_pitch=40 * 64, table=one, starts=one, base_row=0, row_elems=64, partial=one, M=2, N=3, Np=64, K=24 * 64,
             ksplit=8, dtype=BF16, stream=None)
    a.update(kw)
    return list(a.values())


def test_sim_gemm_windows_refuses_bad_arguments_without_launch(lib):
    L = lib.load()
    err = L.sda_last_error
    for name in ("X", "table", "starts", "partial"):
        assert L.sda_sim_gemm_windows(*gemm_args(**{name: None})) == -1
        assert b"null" in err()
    assert L.sda_sim_gemm_windows(*gemm_args(dtype=F32)) == -1
    assert b"16-bit" in err() and b"fp32" in err()
    assert L.sda_sim_gemm_windows(*gemm_args(dtype=7)) == -1
    for bad in (dict(K=24 * 64 + 16), dict(K=0), dict(x_pitch=24 * 64 - 64), dict(x_pitch=40 * 64 + 4), dict(M=0), dict(N=0)):
        assert L.sda_sim_gemm_windows(*gemm_args(**bad)) == -1, bad
        assert b"K-steps" in err()
    for bad in (dict(row_elems=40), dict(row_elems=0), dict(row_elems=96), dict(base_row=-1)):
        assert L.sda_sim_gemm_windows(*gemm_args(**bad)) == -1, bad
        assert b"multiple of 64" in err()
    for bad in (dict(Np=2), dict(Np=6), dict(N=70, Np=64)):
        assert L.sda_sim_gemm_windows(*gemm_args(**bad)) == -1, bad
        assert b"padded width" in err()
    for ks in (0, -1, 49, 1000):                 # K = 1536 is 48 K-steps
        assert L.sda_sim_gemm_windows(*gemm_args(ksplit=ks)) == -1
        assert b"ksplit" in err()
    assert L.sda_sim_gemm_windows(*gemm_args(x_pitch=1 << 23, K=64, ksplit=2)) == -1         # 256 rows of X span 4 GB
    assert b"4 GB" in err()
    for name, addr in (("X", 72), ("table", 68), ("partial", 80 + 8), ("starts", 66)):
        assert L.sda_sim_gemm_windows(*gemm_args(**{name: ctypes.c_void_p(addr)})) == -1, name
        assert b"aligned" in err()
    # the span one launch serves: (2^31 - 32) elements of 16-bit storage behind base_row
    assert L.sda_sim_gemm_windows_span(64) == ((1 << 31) - 32) // 64
    assert L.sda_sim_gemm_windows_span(1024) == ((1 << 31) - 32) // 1024 == 2097151
    assert L.sda_sim_gemm_windows_span(0) == L.sda_sim_gemm_windows_span(40) == L.sda_sim_gemm_windows_span(-64) == 0


def test_window_sumsq_refuses_bad_arguments_without_launch(lib):
    L = lib.load()
    one = ctypes.c_void_p(64)
    for missing in range(3):
        args = [one, one, one]
        args[missing] = None
        assert L.sda_window_sumsq(*args, 4, 24, None) == -1
        assert b"null" in L.sda_last_error()
    for M, T in ((0, 24), (-1, 24), (4, 0), (4, -3)):
        assert L.sda_window_sumsq(one, one, one, M, T, None) == -1
        assert b"M, T" in L.sda_last_error()
    for slot in range(3):
        args = [one, one, one]
        args[slot] = ctypes.c_void_p(66)
        assert L.sda_window_sumsq(*args, 4, 24, None) == -1
        assert b"aligned" in L.sda_last_error()


def test_ops_wrappers_refuse_cpu_tensors(lib):
    from speech_decoding_amd import SdaError, ops
    z = torch.zeros(64 * 64, dtype=torch.bfloat16)
    with pytest.raises(SdaError):
        ops.sim_gemm_windows_into(z, 64, z, torch.zeros(3, dtype=torch.int32), 0, 2, 64, 1, 3, 64, 1, torch.zeros(0), torch.zeros(64))
    with pytest.raises(SdaError):
        ops.window_sumsq(torch.zeros(30), torch.zeros(3, dtype=torch.int32), 3, 24)


def test_argument_errors_come_before_the_device_and_in_order(lib):
    from speech_decoding_amd import SdaError, WindowBank, retrieve, retrieve_classes
    with pytest.raises(ValueError):
        WindowBank(0, 5)
    with pytest.raises(ValueError):
        WindowBank(8, 0)
    with pytest.raises(ValueError, match="16-bit"):
        WindowBank(8, 5, dtype=torch.float32)                       # no fp32 window path, and no materialising instead
    with pytest.raises(ValueError):
        WindowBank(8, 5, dtype=torch.float64)
    with pytest.raises(SdaError):
        WindowBank(8, 5, device="cpu")
    bank = WindowBank(8, 5, dtype=torch.float16)
    assert len(bank) == 0 and bank.F == 8 and bank.T == 5 and bank.dtype == torch.float16 and bank.nbytes == 0
    E = torch.zeros(8, 30)                                          # a CPU tensor: refused LAST
    for bad in (torch.zeros(9, 30), torch.zeros(30, 8), torch.zeros(8), torch.zeros(1, 8, 30), torch.zeros(8, 4), "track"):
        with pytest.raises(ValueError):
            bank.add_track(bad, [0])
    for starts in ([[0, 1]], [0.5, 1.0], 3):
        with pytest.raises(ValueError):
            bank.add_track(E, starts)
    for starts in ([-1], [26], [0, 25, 26], np.array([3, 400])):    # L - T = 25 is the last window
        with pytest.raises(IndexError):
            bank.add_track(E, starts)
    with pytest.raises(IndexError):                                 # a wrong start on a CPU tensor: the start is named first
        bank.add_track(E, [26])
    for starts in ([0], [25, 0, 25], np.array([7], dtype=np.uint16), torch.tensor([0, 3])):
        with pytest.raises(SdaError):                               # everything right but the device
            bank.add_track(E, starts)
    assert len(bank) == 0 and bank.nbytes == 0
    Q = torch.zeros(2, 8, 5)
    with pytest.raises(ValueError, match="empty"):
        retrieve(Q, bank)
    with pytest.raises(ValueError, match="SpeechBank or a WindowBank"):
        retrieve(Q, "bank", k=5)
    bank._size = 20                                                 # stands for a filled bank
    for bad in (torch.zeros(2, 9, 5), torch.zeros(2, 8, 4), torch.zeros(8, 5), torch.zeros(0, 8, 5)):
        with pytest.raises(ValueError):
            retrieve(bad, bank, k=5)
    for k in (0, 65, 21, 2.5):
        with pytest.raises(ValueError):
            retrieve(Q, bank, k=k)
    with pytest.raises(IndexError):
        retrieve(Q, bank, k=5, labels=[0, 20])
    with pytest.raises(ValueError):
        retrieve(Q, bank, k=5, scratch_bytes=16)
    with pytest.raises(ValueError):
        retrieve_classes(Q, bank, np.arange(19))                    # the class index covers 19 candidates, the bank 20
    with pytest.raises(SdaError):                                   # and only then the device
        retrieve(Q, bank, k=5, labels=[3, 19])
    with pytest.raises(SdaError):
        retrieve_classes(Q, bank, np.arange(20) % 7, k=3)


def test_score_pass_contracts_over_the_valid_rows_only(lib):
    """Against a window bank the query operand is the packed rows from their ROW_PAD-th row on and K = T * pad64(F) — the
    plan is made with that K; against a SpeechBank nothing changes."""
    from speech_decoding_amd import SpeechBank, WindowBank
    from speech_decoding_amd import lib as L
    from speech_decoding_amd.retrieval import _ScorePass
    Q = torch.zeros(3, 40, 24)
    wb, sb = WindowBank(40, 24), SpeechBank(40, 24)
    wb._size = sb._size = 600
    w, s = _ScorePass("retrieve", Q, wb), _ScorePass("retrieve", Q, sb)
    assert (w.K, w.q_pitch, w.q_skip) == (24 * 64, 40 * 64, L.ROW_PAD * 64)
    assert (s.K, s.q_pitch, s.q_skip) == (40 * 64, 40 * 64, 0) and s.K == sb.row_elems
    assert wb.row_elems == 64


def test_memory_figure_is_arithmetic(lib):
    """nbytes = table + starts and norms + per-row sums; for case a's candidates it is well below the materialised bank's rows."""
    from speech_decoding_amd import WindowBank
    c = W.case("a")
    bank = WindowBank(c["F"], c["T"])
    bank._L, bank._size = c["table"].shape[0], c["M"]               # what add_track leaves for case a's tracks
    Cp = W.pad64(c["F"])
    assert bank.nbytes == 833 * Cp * 2 + 8 * 600 + 4 * 833 == 114756
    materialised = c["M"] * (c["T"] + 16) * Cp * 2
    assert materialised == 3072000 and bank.nbytes < materialised / 25


@pytest.mark.parametrize("shape", ["a", "b"])
def test_cases_have_the_edges_they_promise(shape):
    c = W.case(shape)
    sh = W.SHAPES[shape]
    assert c["starts"].shape == (sh["M"],) and c["queries"].shape == (sh["N"], sh["F"], sh["T"])
    row0 = 0
    for Lt, s in zip(sh["tracks"], c["local"]):
        assert s.min() == 0 and s.max() == Lt - sh["T"]             # both ends of every track
        assert Lt // 3 in s and Lt // 3 + 1 in s and (s == Lt // 3).sum() >= 2          # adjacent starts and a duplicate
        assert not np.array_equal(s, np.sort(s))                    # shuffled
        row0 += Lt
    assert c["table"].shape == (row0, sh["F"])
    for arr in (c["table"], c["queries"]):                          # integers, exact in bf16 and fp16
        assert np.array_equal(arr, np.round(arr)) and np.abs(arr).max() <= 9
        assert np.array_equal(W.rounded(arr, "bf16"), arr) and np.array_equal(W.rounded(arr, "fp16"), arr)


@pytest.mark.parametrize("shape", ["a", "b"])
def test_restatement_reproduces_the_float64_brute_force(shape):
    """Dot products and squared norms are the brute force's integers, all below 2^24 (so fp32 sums are exact in any order and
    under any K split); the fp32 scores are the float64 cosine to three roundings; a chunked restatement gives the same."""
    c = W.case(shape)
    cos, csq, dots = W.cosine64(c)
    r = W.restate(c)
    assert not r.outside
    assert np.array_equal(r.S, dots) and np.array_equal(r.csq, csq)
    for v in (r.S, r.qsq, r.csq):
        assert np.array_equal(v, np.round(v)) and np.abs(v).max() < 2 ** 24
    assert np.abs(r.S).max() <= 1.4e5
    idx, sc, ranks = r
    top = -np.sort(-cos, axis=1)[:, :10]
    assert np.abs(sc - top).max() <= 3 * 2.0 ** -24
    assert np.abs(np.take_along_axis(cos, idx, 1) - sc).max() <= 3 * 2.0 ** -24
    # ranks: the labelled candidate's position in float64, counting an exact tie (a duplicate window) to the lower index
    sl = cos[np.arange(c["N"]), c["labels"]][:, None]
    gap = np.abs(cos - sl)
    assert not ((gap > 0) & (gap < 1e-6)).any()                     # no near-tie that fp32 could turn round
    want = ((cos > sl) | ((cos == sl) & (np.arange(c["M"])[None, :] < c["labels"][:, None]))).sum(1)
    assert np.array_equal(ranks, want)
    assert (ranks[:3] <= 1).all() and ranks.dtype == np.int32
    for mc in (256, 64):
        again = W.restate(c, mc=mc)
        assert all(np.array_equal(x, y) for x, y in zip(r, again))


@pytest.mark.parametrize("mutant", W.MUTANTS)
def test_every_planted_bug_is_told_apart(mutant):
    """Each planted bug changes (indices, scores, ranks) of at least one shared case, whole or in 256-candidate chunks (the GPU
    suite runs both).  One cannot: a contraction one row LONG multiplies the next query's zero pad row — on the device it is an
    address past the last window's end, and the cases have a window at L - T of every track so that it is one."""
    told, outside = False, False
    for shape in ("a", "b"):
        c = W.case(shape)
        for mc in (None, 256):
            good, bad = W.restate(c, mc=mc), W.restate(c, mc=mc, mutant=mutant)
            told |= any(not np.array_equal(x, y) for x, y in zip(good, bad))
            outside |= bad.outside
    if mutant == "k_one_row_long":
        assert outside and not told
    else:
        assert told


def test_tile_and_chunk_offsets_are_told_apart_at_case_a():
    c = W.case("a")
    good = W.restate(c)
    assert any(not np.array_equal(x, y) for x, y in zip(good, W.restate(c, mutant="tile_offset_dropped")))
    good = W.restate(c, mc=256)
    assert any(not np.array_equal(x, y) for x, y in zip(good, W.restate(c, mc=256, mutant="chunk_offset_dropped")))
