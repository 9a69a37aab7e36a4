"""CPU checks of the decoding surface (speech_decoding_amd/retrieval.py, csrc/retrieval.hip): the new C entry points are
declared, exported and bound and refuse bad arguments without a launch; SpeechBank / retrieve validate their arguments before
touching the device and refuse CPU tensors (no CPU path); the blocking plan keeps its memory bound.  No kernel is launched."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = ("sda_retrieval_select", "sda_retrieval_scores_floats")


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
    assert A.SpeechBank is retrieval.SpeechBank and A.retrieve is retrieval.retrieve and A.Retrieval is retrieval.Retrieval
    assert {"SpeechBank", "Retrieval", "retrieve"} <= set(A.__all__)
    assert callable(ops.retrieval_select) and callable(A.Classifier.decode)
    assert "queries" in A.Classifier.decode.__doc__.lower() and "candidates" in A.Classifier.decode.__doc__.lower()


def test_entry_points_refuse_bad_arguments_without_launch(lib):
    L = lib.load()
    one = ctypes.c_void_p(64)            # a non-null, 16-byte aligned address that is never dereferenced: every call below is refused
    assert L.sda_retrieval_select(None, None, None, None, None, None, None, 1, 1, 1, 64, None) == -1
    assert b"null" in L.sda_last_error()
    for missing in range(5):            # S, qsq, csq, indices, scores
        args = [one, one, one, None, one, one, None]
        args[missing if missing < 3 else missing + 1] = None
        assert L.sda_retrieval_select(*args, 4, 100, 10, 128, None) == -1
        assert b"null" in L.sda_last_error()
    for k in (0, -1, 65, 1000):
        assert L.sda_retrieval_select(one, one, one, None, one, one, None, 4, 100, k, 128, None) == -1
        assert b"k =" in L.sda_last_error()
    assert L.sda_retrieval_select(one, one, one, None, one, one, None, 4, 8, 9, 64, None) == -1       # k > M
    assert L.sda_retrieval_select(one, one, one, one, one, one, None, 4, 100, 10, 128, None) == -1    # labels without ranks
    assert L.sda_retrieval_select(one, one, one, None, one, one, None, 0, 100, 10, 128, None) == -1   # n
    assert L.sda_retrieval_select(one, one, one, None, one, one, None, 4, 0, 1, 128, None) == -1      # M
    for chunk in (0, 100, -64):
        assert L.sda_retrieval_select(one, one, one, None, one, one, None, 4, 100, 10, chunk, None) == -1
        assert L.sda_retrieval_scores_floats(4, 100, chunk) == -1
    assert L.sda_retrieval_select(ctypes.c_void_p(68), one, one, None, one, one, None, 4, 100, 10, 128, None) == -1   # alignment
    assert L.sda_retrieval_scores_floats(0, 100, 64) == -1 and L.sda_retrieval_scores_floats(4, 0, 64) == -1
    # chunk-major size: whole chunks at their own width, the last one padded to 64 columns
    assert L.sda_retrieval_scores_floats(4, 100, 128) == 4 * 128
    assert L.sda_retrieval_scores_floats(4, 1000, 1024) == 4 * 1024
    assert L.sda_retrieval_scores_floats(8, 1000, 256) == 8 * (3 * 256 + 256)
    assert L.sda_retrieval_scores_floats(8, 1000, 384) == 8 * (2 * 384 + 256)


def test_cpu_tensors_are_refused(lib):
    from speech_decoding_amd import SdaError, SpeechBank, retrieve
    bank = SpeechBank(8, 5)
    with pytest.raises(SdaError):
        bank.add(torch.zeros(3, 8, 5))
    with pytest.raises(SdaError):
        SpeechBank.from_tensor(torch.zeros(3, 8, 5))
    with pytest.raises(SdaError):
        SpeechBank(8, 5, device="cpu")
    bank._size = 20                      # stands for a filled bank: the device check comes after every argument check
    with pytest.raises(SdaError):
        retrieve(torch.zeros(2, 8, 5), bank, k=5)
    with pytest.raises(SdaError):
        retrieve(torch.zeros(2, 8, 5), bank, k=5, labels=[3, 19])


def test_argument_errors_come_before_the_device(lib):
    from speech_decoding_amd import SpeechBank, retrieve
    with pytest.raises(ValueError):
        SpeechBank(0, 5)
    with pytest.raises(ValueError):
        SpeechBank(8, 5, dtype=torch.float64)
    bank = SpeechBank(8, 5)
    assert len(bank) == 0
    for bad in (torch.zeros(3, 9, 5), torch.zeros(3, 8, 6), torch.zeros(8, 5), torch.zeros(1, 3, 8, 5)):
        with pytest.raises(ValueError):
            bank.add(bad)
    Q = torch.zeros(2, 8, 5)
    with pytest.raises(ValueError, match="empty"):
        retrieve(Q, bank)
    bank._size = 20                      # stands for a filled bank
    for bad in (torch.zeros(2, 9, 5), torch.zeros(2, 8, 4), torch.zeros(8, 5), torch.zeros(0, 8, 5)):
        with pytest.raises(ValueError):
            retrieve(bad, bank, k=5)
    for k in (0, -3, 65, 21, 2.5):       # 1 ... min(64, M = 20)
        with pytest.raises(ValueError):
            retrieve(Q, bank, k=k)
    for labels in ([0, 20], [-1, 3], torch.tensor([5, 99]), np.array([20, 0])):
        with pytest.raises(IndexError):
            retrieve(Q, bank, k=5, labels=labels)
    for labels in ([1, 2, 3], [0.5, 1.0], torch.zeros(2, 1, dtype=torch.int64)):
        with pytest.raises(ValueError):
            retrieve(Q, bank, k=5, labels=labels)
    with pytest.raises(ValueError):
        retrieve(Q, bank, k=5, scratch_bytes=16)
    with pytest.raises(ValueError):
        retrieve(Q, "bank", k=5)


def test_blocking_plan_keeps_the_memory_bound(lib):
    """Scratch = one query block's scores over the bank + the K slices' partial sums, never above scratch_bytes; chunks are
    multiples of 64 columns (256 when the bank is split); the plan is a pure function of its arguments."""
    from speech_decoding_amd import lib as L
    from speech_decoding_amd.retrieval import plan_blocks
    lib.load()
    cases = [(96, 1000, 6784, 64 << 10), (96, 1000, 6784, 1 << 30), (1, 1000, 6784, 1 << 20), (40, 300, 4224, 32 << 10),
             (256, 32768, 385024, 1 << 30), (256, 32768, 385024, 64 << 20), (1000, 4096, 385024, 8 << 20)]
    for dtype in (torch.float32, torch.bfloat16, torch.float16):
        for N, M, K, scratch in cases:
            nb, mc, tiles256, ks = plan_blocks(N, M, K, dtype, scratch)
            assert plan_blocks(N, M, K, dtype, scratch) == (nb, mc, tiles256, ks)
            assert 1 <= nb <= N and mc % 64 == 0 and (mc >= M or mc % 256 == 0 or dtype == torch.float32)
            slab = 32 if (tiles256 or dtype == torch.float32) else 64
            assert 1 <= ks <= K // slab
            used = 4 * nb * L.pad_channels(M) + (4 * ks * nb * mc if ks > 1 else 0)
            assert used <= scratch, (N, M, K, scratch, dtype, nb, mc, ks, used)
    nb, mc, _, ks = plan_blocks(96, 1000, 6784, torch.bfloat16, 64 << 10)
    assert nb < 96 and mc < 1000          # the setting the GPU suite uses to force several query blocks and bank chunks


def test_retrieval_module_does_not_import_the_loss():
    """retrieval.py rests on ops alone: importing it brings in neither the loss module nor the encoder's engine.  Checked in a
    fresh process; the package's __init__ (which re-exports CLIPLoss and BrainEncoder) is stood in for by a bare package."""
    import subprocess
    import sys
    code = ("import sys, types\n"
            "pkg = types.ModuleType('speech_decoding_amd')\n"
            "pkg.__path__ = [%r]\n"
            "sys.modules['speech_decoding_amd'] = pkg\n"
            "import speech_decoding_amd.retrieval as R\n"
            "assert callable(R.retrieve) and 'speech_decoding_amd.ops' in sys.modules\n"
            "bad = [m for m in ('loss', 'engine', 'models', 'blocks') if 'speech_decoding_amd.' + m in sys.modules]\n"
            "assert not bad, bad\n" % os.path.join(ROOT, "speech_decoding_amd"))
    done = subprocess.run([sys.executable, "-c", code], cwd=ROOT, capture_output=True, text=True)
    assert done.returncode == 0, done.stderr
