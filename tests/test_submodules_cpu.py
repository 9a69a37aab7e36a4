"""CPU checks of the standalone submodules `SpatialAttention`, `SubjectBlock` and `ConvBlock`: a call on CPU tensors is refused
(there is no CPU path), their state_dict keys are the reference's, their compute dtype follows args / the encoder, and the C ABI
of sda_pack_rows_typed refuses bad arguments before any launch.  No kernel is launched here."""
import ctypes
import os

import numpy as np
import pytest
import torch

from oracle import brain_oracle as O
from tests import golden_io as G
from tests.builders import encoder_args

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def lib():
    from speech_decoding_amd import lib as L
    if not os.path.exists(L.LIB_PATH):
        import __graft_entry__ as g
        g.build()
    return L


def make_args(C=12, S=3, D1=16, D2=24, K=4, dtype="fp32"):
    return encoder_args(dict(S=S, D1=D1, D2=D2, F=32, K=K), O.synthetic_positions(C, seed=7), dtype)


def test_cpu_tensors_are_refused(lib):
    from speech_decoding.models import ConvBlock, SpatialAttention, SubjectBlock
    from speech_decoding_amd import SdaError
    args = make_args()
    state = np.random.get_state()
    with pytest.raises(SdaError, match="no CPU path"):
        SpatialAttention(args)(torch.randn(2, 12, 8))
    with pytest.raises(SdaError, match="no CPU path"):
        SubjectBlock(args)(torch.randn(2, 12, 8), torch.tensor([0, 2]))
    for k in range(5):
        with pytest.raises(SdaError, match="no CPU path"):
            ConvBlock(k, 16, 24)(torch.randn(2, 16 if k == 0 else 24, 8))
    after = np.random.get_state()
    assert after[0] == state[0] and np.array_equal(after[1], state[1]) and after[2:] == state[2:]   # nothing was drawn


def test_state_dict_keys_equal_the_reference(lib):
    from speech_decoding.models import ConvBlock, SpatialAttention, SubjectBlock
    npz = G.load("e2e_small.npz")
    C, S, D1, D2 = (int(v) for v in npz["dims"][:4])
    ref = [k[len("init/"):].replace("@re", "") for k in npz if k.startswith("init/") and not k.endswith("@im")]
    args = make_args(C, S, D1, D2)

    def under(prefix):
        return [k[len(prefix):] for k in ref if k.startswith(prefix)]
    assert list(SpatialAttention(args).state_dict()) == under("subject_block.spatial_attention.")
    assert list(SubjectBlock(args).state_dict()) == under("subject_block.")
    for k in range(5):
        assert list(ConvBlock(k, D1, D2).state_dict()) == under(f"conv_blocks.conv{k}.")


def test_compute_dtype_follows_args_and_the_encoder(lib, monkeypatch):
    from speech_decoding.models import BrainEncoder, ConvBlock, SpatialAttention, SubjectBlock
    monkeypatch.delenv("SDA_COMPUTE_DTYPE", raising=False)
    assert SpatialAttention(make_args(dtype="bf16")).compute_dtype == torch.bfloat16
    sb = SubjectBlock(make_args(dtype="fp16"))
    assert sb.compute_dtype == sb.spatial_attention.compute_dtype == torch.float16
    cb = ConvBlock(2, 16, 24)
    assert cb.compute_dtype == torch.float32
    assert cb.set_compute_dtype(torch.bfloat16) is cb and cb.compute_dtype == torch.bfloat16
    monkeypatch.setenv("SDA_COMPUTE_DTYPE", "bf16")
    assert ConvBlock(0, 16, 24).compute_dtype == torch.bfloat16
    monkeypatch.delenv("SDA_COMPUTE_DTYPE")
    enc = BrainEncoder(make_args(dtype="bf16"))
    blocks = [enc.subject_block, enc.subject_block.spatial_attention] + list(enc.conv_blocks)
    assert all(m.compute_dtype == torch.bfloat16 for m in blocks)
    enc.set_compute_dtype(torch.float16)
    assert enc.compute_dtype == torch.float16 and all(m.compute_dtype == torch.float16 for m in blocks)


def test_bad_inputs_raise_before_anything_runs(lib):
    from speech_decoding.models import ConvBlock, SpatialAttention, SubjectBlock
    args = make_args()
    with pytest.raises(AssertionError):
        SpatialAttention(args)(torch.randn(2, 11, 8))
    with pytest.raises(ValueError):
        SubjectBlock(args)(torch.randn(12, 8), torch.tensor([0]))
    with pytest.raises(RuntimeError, match="channels"):
        ConvBlock(1, 16, 24)(torch.randn(2, 16, 8))


def test_pack_rows_typed_is_exported_and_bound(lib):
    cdll = ctypes.CDLL(lib.LIB_PATH)
    assert hasattr(cdll, "sda_pack_rows_typed") and "sda_pack_rows_typed" in lib.SIGNATURES
    header = open(os.path.join(ROOT, "include", "sd_amd.h")).read()
    assert "int sda_pack_rows_typed(" in header
    assert lib.load().sda_abi_version() == lib.ABI_VERSION == 4


def test_pack_rows_typed_argument_validation_without_launch(lib):
    L = lib.load()
    buf = (ctypes.c_float * 4096)()
    p = ctypes.addressof(buf)                   # host memory: every call below must fail its checks before any launch
    F32, BF16, F16 = lib.F32, lib.BF16, lib.F16

    def pack(*a):
        return L.sda_pack_rows_typed(*a, None)
    assert pack(None, p, 2, 8, 8, 64, F32, BF16) == -1 and b"bad arguments" in L.sda_last_error()
    assert pack(p, None, 2, 8, 8, 64, F32, BF16) == -1 and b"bad arguments" in L.sda_last_error()
    assert pack(p, p, 2, 80, 8, 64, F32, F32) == -1 and b"bad arguments" in L.sda_last_error()       # Cp < C
    assert pack(p, p, 2, 8, 8, 96, F32, F32) == -1 and b"bad arguments" in L.sda_last_error()       # Cp not a multiple of 64
    assert pack(p, p, 0, 8, 8, 64, F32, F32) == -1 and b"bad arguments" in L.sda_last_error()
    assert pack(p, p, 2, 8, 0, 64, F32, F32) == -1 and b"bad arguments" in L.sda_last_error()
    assert pack(p, p, 2, 8, 8, 64, 7, F32) == -1 and b"unknown dtype" in L.sda_last_error()
    assert pack(p, p, 2, 8, 8, 64, F16, -1) == -1 and b"unknown dtype" in L.sda_last_error()
    for s, d in ((F32, F32), (BF16, F16), (F16, BF16)):
        assert pack(p, p, 2, 8, 8, 64, s, d) == -1 and b"device memory" in L.sda_last_error()


def test_ops_pack_rows_typed_refuses_host_tensors(lib):
    from speech_decoding_amd import SdaError, ops
    with pytest.raises(SdaError, match="device"):
        ops.pack_rows(torch.randn(2, 8, 8, dtype=torch.bfloat16), torch.zeros(lib.rows_alloc(2, 8), 64))
