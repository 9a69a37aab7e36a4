"""CPU checks of the MSELoss surface: the drop-in module exports what the reference's loss.py gives to
`from speech_decoding.utils.loss import *` (CLIPLoss, MSELoss, torch_exp, torch_log), the two clamped helpers, and the C ABI
of the MSE kernels (exported, bound, arguments refused without a launch).  No kernel is launched here."""
import ctypes
import os
import subprocess
import sys
import textwrap

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def lib():
    from speech_decoding_amd import lib as L
    if not os.path.exists(L.LIB_PATH):
        import __graft_entry__ as g
        g.build()
    return L


def test_star_import_gives_the_reference_names():
    code = textwrap.dedent("""
        from speech_decoding.utils.loss import *
        import speech_decoding_amd
        assert MSELoss is speech_decoding_amd.MSELoss and CLIPLoss is speech_decoding_amd.CLIPLoss
        assert torch_exp is speech_decoding_amd.torch_exp and torch_log is speech_decoding_amd.torch_log
        print(MSELoss.__module__, torch_exp.__module__, torch_log.__module__)
    """)
    out = subprocess.run([sys.executable, "-c", code], env=dict(os.environ, PYTHONPATH=ROOT), capture_output=True, text=True,
                         cwd="/tmp")
    assert out.returncode == 0, out.stderr[-2000:]
    assert out.stdout.split() == ["speech_decoding_amd.loss"] * 3


def test_star_import_overlays_a_reference_checkout(tmp_path):
    """With a reference-shaped tree later on the path, the loss names still resolve to this build."""
    ref = tmp_path / "ref" / "speech_decoding"
    (ref / "utils").mkdir(parents=True)
    (ref / "__init__.py").write_text("")
    (ref / "models.py").write_text("BrainEncoder = Classifier = 'reference'\n")
    (ref / "utils" / "loss.py").write_text("CLIPLoss = MSELoss = torch_exp = torch_log = 'reference'\n")
    (ref / "utils" / "reproducibility.py").write_text("def seed_worker(i): return 'reference'\n")
    code = textwrap.dedent("""
        from speech_decoding.utils.loss import *
        from speech_decoding.utils.reproducibility import seed_worker
        import speech_decoding_amd
        assert seed_worker(0) == 'reference'
        assert MSELoss is speech_decoding_amd.MSELoss and CLIPLoss is speech_decoding_amd.CLIPLoss
        assert torch_exp is speech_decoding_amd.torch_exp and torch_log is speech_decoding_amd.torch_log
        print('overlay ok')
    """)
    env = dict(os.environ, PYTHONPATH=os.pathsep.join([ROOT, str(tmp_path / "ref")]), PYTHONDONTWRITEBYTECODE="1")
    out = subprocess.run([sys.executable, "-c", code], env=env, capture_output=True, text=True, cwd=str(tmp_path))
    assert out.returncode == 0 and "overlay ok" in out.stdout, out.stderr[-2000:]


def test_torch_exp_clamps_from_above_at_ten():
    from speech_decoding_amd import torch_exp
    x = torch.tensor([-50.0, -1.0, 0.0, 2.5, 9.999, 10.0, 10.001, 11.0, 1e6, float("inf")])
    got = torch_exp(x)
    want = torch.exp(torch.tensor([-50.0, -1.0, 0.0, 2.5, 9.999, 10.0, 10.0, 10.0, 10.0, 10.0]))
    assert torch.equal(got, want)
    assert torch.isfinite(got).all()
    assert float(got[-1]) == pytest.approx(22026.465794806718, rel=1e-6)
    y = torch.tensor([3.0, 12.0], requires_grad=True)
    torch_exp(y).sum().backward()
    assert y.grad[0] == pytest.approx(float(torch.exp(torch.tensor(3.0)))) and float(y.grad[1]) == 0.0   # clamped: no gradient


def test_torch_log_clamps_from_below_at_1e_10():
    from speech_decoding_amd import torch_log
    x = torch.tensor([0.0, -3.0, 1e-12, 1e-10, 2e-10, 1.0, 7.5])
    got = torch_log(x)
    floor = torch.log(torch.tensor(1e-10))
    want = torch.stack([floor, floor, floor, floor, torch.log(torch.tensor(2e-10)), torch.tensor(0.0), torch.log(torch.tensor(7.5))])
    assert torch.equal(got, want)
    assert float(got[0]) == pytest.approx(-23.025850929940457, rel=1e-6)
    assert torch.isfinite(got).all()
    d = torch_log(torch.tensor([1e-10, 1e-11], dtype=torch.float64))
    assert float(d[0]) == float(d[1]) == pytest.approx(-23.025850929940457, rel=1e-12)


def test_mse_symbols_are_exported_and_bound(lib):
    cdll = ctypes.CDLL(lib.LIB_PATH)
    for name in ("sda_mse_forward", "sda_mse_backward"):
        assert hasattr(cdll, name)
        assert name in lib.SIGNATURES
    header = open(os.path.join(ROOT, "include", "sd_amd.h")).read()
    assert f"#define SDA_MSE_PARTIALS {lib.MSE_PARTIALS}" in header


def test_mse_argument_validation_without_launch(lib):
    L = lib.load()
    buf = (ctypes.c_double * 64)()
    p = ctypes.addressof(buf)                         # host memory: a validation failure must return before any launch
    loss = ctypes.addressof((ctypes.c_float * 4)())

    def fwd(*a):
        return L.sda_mse_forward(*a, None)

    def bwd(*a):
        return L.sda_mse_backward(*a, None)

    F32, BF16 = lib.F32, lib.BF16
    assert fwd(None, 0, F32, p, 0, F32, 2, 8, 8, 2, p, loss) == -1 and b"null operand" in L.sda_last_error()
    assert fwd(p, 0, F32, p, 0, F32, 0, 8, 8, 1, p, loss) == -1 and b"bad sizes" in L.sda_last_error()
    assert fwd(p, 0, F32, p, 0, F32, 2, 8, 8, 0, p, loss) == -1 and b"bad sizes" in L.sda_last_error()
    assert fwd(p, 0, 7, p, 0, F32, 2, 8, 8, 2, p, loss) == -1 and b"unknown dtype" in L.sda_last_error()
    assert fwd(p, 96, BF16, p, 0, F32, 2, 8, 8, 2, p, loss) == -1 and b"channel pitch" in L.sda_last_error()
    assert fwd(p, 64, BF16, p, 0, F32, 2, 80, 8, 2, p, loss) == -1 and b"channel pitch" in L.sda_last_error()
    assert fwd(p, 64, BF16, p, 128, BF16, 2, 8, 8, 2, p, loss) == -1 and b"different channel pitch" in L.sda_last_error()
    assert fwd(p + 4, 64, F32, p, 0, F32, 2, 8, 8, 2, p, loss) == -1 and b"aligned" in L.sda_last_error()
    assert fwd(p, 0, F32, p, 0, F32, 2, 8, 8, 2, None, loss) == -1 and b"null scratch" in L.sda_last_error()
    assert fwd(p, 0, F32, p, 0, F32, 2, 8, 8, 2, p, None) == -1
    assert bwd(p, 0, F32, p, 0, F32, 2, 8, 8, 2, p, None, None) == -1 and b"neither dz nor dy" in L.sda_last_error()
    assert bwd(p, 0, F32, p, 0, F32, 2, 8, 8, 2, None, p, None) == -1 and b"null dloss" in L.sda_last_error()
    assert bwd(p, 64, F32, p, 0, F32, 2, 8, 8, 2, p, p + 8, None) == -1 and b"aligned" in L.sda_last_error()
    assert bwd(p, 0, F32, None, 0, F32, 2, 8, 8, 2, p, p, None) == -1 and b"null operand" in L.sda_last_error()


def test_mse_loss_refuses_cpu_operands_and_mismatched_shapes(lib):
    from speech_decoding_amd import MSELoss, SdaError
    crit = MSELoss()
    assert crit.global_batch is True and list(crit.parameters()) == []
    with pytest.raises(SdaError, match="no CPU path"):
        crit(torch.randn(2, 8, 5), torch.randn(2, 8, 5))
    with pytest.raises(ValueError, match="one shape"):
        crit(torch.randn(2, 8, 5), torch.randn(2, 8, 4))
    with pytest.raises(ValueError, match="one shape"):
        crit(torch.randn(1, 8, 5), torch.randn(2, 8, 5))          # the reference would broadcast this with a warning
