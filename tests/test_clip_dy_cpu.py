"""CPU checks of CLIPLoss's gradient for its first argument (the speech embeddings): the reference-made fixture
tests/golden/clip_grad.npz agrees with this file's own float64 formula of dx, dy, dtemp and the loss, there is still no CPU
path when x requires a gradient, and the new C ABI entry points refuse bad arguments without a launch."""
import ctypes
import os

import numpy as np
import pytest
import torch

from tests import golden_io as G
from tests.builders import clip_loss

CASES = [("fast-mean", True, "mean"), ("fast-sum", True, "sum"), ("slow-mean", False, "mean"), ("slow-sum", False, "sum")]


def clip_formula(x, y, temp, fast, reduction):
    """(loss, dx, dy, dtemp) in float64 from the closed form: with s = exp(temp) (1 for fast=False), L = s * x^ y^T,
    D = softmax_row(L) + softmax_col(L) - 2 I and inv_norm = 1 / (2B) ("mean") or 1 / 2 ("sum"):
        dx_i = inv_norm * ( s / |x_i| * sum_j D_ij y^_j  -  (sum_j D_ij L_ij) x_i / |x_i|^2 )
        dy_j = inv_norm * ( s / |y_j| * sum_i D_ij x^_i  -  (sum_i D_ij L_ij) y_j / |y_j|^2 )
        dtemp = inv_norm * sum_ij D_ij L_ij  (0 for fast=False, which does not use temp)."""
    B = x.shape[0]
    X, Y = x.reshape(B, -1).double(), y.reshape(B, -1).double()
    nx, ny = X.norm(dim=1, keepdim=True), Y.norm(dim=1, keepdim=True)
    s = float(np.exp(float(temp))) if fast else 1.0
    Lg = s * (X / nx) @ (Y / ny).T
    inv_norm = 1.0 / (2 * B) if reduction == "mean" else 0.5
    lse_r, lse_c = torch.logsumexp(Lg, dim=1), torch.logsumexp(Lg, dim=0)
    diag = torch.diagonal(Lg)
    loss = inv_norm * float(((lse_r - diag) + (lse_c - diag)).sum())
    D = torch.softmax(Lg, dim=1) + torch.softmax(Lg, dim=0) - 2.0 * torch.eye(B, dtype=torch.float64)
    DL = D * Lg
    dx = inv_norm * (s / nx * (D @ (Y / ny)) - DL.sum(dim=1, keepdim=True) * X / nx ** 2)
    dy = inv_norm * (s / ny * (D.T @ (X / nx)) - DL.sum(dim=0).unsqueeze(1) * Y / ny ** 2)
    dtemp = inv_norm * float(DL.sum()) if fast else 0.0
    return loss, dx.reshape(x.shape), dy.reshape(y.shape), dtemp


def test_fixture_agrees_with_the_float64_formula():
    g = G.load("clip_grad.npz")
    shapes = g["shapes"]
    assert len(shapes) == 3 and 2 in shapes[:, 0] and any(int(F) % 64 for F in shapes[:, 1]) and any(int(T) % 2 for T in shapes[:, 2])
    for i in range(len(shapes)):
        x, y = torch.from_numpy(g[f"s{i}/x"]), torch.from_numpy(g[f"s{i}/y"])
        assert tuple(x.shape) == tuple(shapes[i])
        for name, fast, reduction in CASES:
            loss, dx, dy, dtemp = clip_formula(x, y, g["temps"][i], fast, reduction)
            k = f"s{i}/{name}"
            assert abs(float(g[f"{k}/loss"]) - loss) <= 1e-5 * abs(loss), (k, float(g[f"{k}/loss"]), loss)
            for got, want in ((g[f"{k}/dx"], dx), (g[f"{k}/dy"], dy)):
                err = float((torch.from_numpy(got).double() - want).abs().max())
                assert err <= 1e-5 * float(want.abs().max()), (k, err)
            assert abs(float(g[f"{k}/dtemp"][0]) - dtemp) <= 1e-5 * max(1.0, abs(dtemp)), (k, float(g[f"{k}/dtemp"][0]), dtemp)


def test_dx_of_the_formula_is_autograd_of_the_loss():
    """The closed form of dx (what the new kernels compute) is the derivative of the loss: float64 autograd of the same
    expression on a random draw, both argument orders."""
    gen = torch.Generator().manual_seed(5)
    x = torch.randn(4, 30, 7, generator=gen, dtype=torch.float64)
    y = torch.randn(4, 30, 7, generator=gen, dtype=torch.float64)
    for fast, reduction in ((True, "mean"), (False, "sum")):
        xl, yl = x.clone().requires_grad_(True), y.clone().requires_grad_(True)
        B = x.shape[0]
        X, Y = xl.reshape(B, -1), yl.reshape(B, -1)
        s = float(np.exp(1.2)) if fast else 1.0
        Lg = s * (X / X.norm(dim=1, keepdim=True)) @ (Y / Y.norm(dim=1, keepdim=True)).T
        t = torch.arange(B)
        ce = torch.nn.functional.cross_entropy
        loss = (ce(Lg, t, reduction=reduction) + ce(Lg.T, t, reduction=reduction)) / 2
        ax, ay = torch.autograd.grad(loss, [xl, yl])
        _, dx, dy, _ = clip_formula(x, y, 1.2, fast, reduction)
        assert float((ax - dx).abs().max()) <= 1e-12 * float(dx.abs().max())
        assert float((ay - dy).abs().max()) <= 1e-12 * float(dy.abs().max())


def test_cpu_operands_with_x_requiring_grad_raise():
    from speech_decoding_amd.lib import SdaError
    crit = clip_loss(1.0, "cpu")
    x = torch.randn(3, 16, 5, requires_grad=True)
    y = torch.randn(3, 16, 5, requires_grad=True)
    with pytest.raises(SdaError):
        crit(x, y)
    with pytest.raises(SdaError):
        crit(y, x)                          # swapped: still no CPU path


@pytest.fixture(scope="module")
def lib():
    from speech_decoding_amd import lib as L
    if not os.path.exists(L.LIB_PATH):
        import __graft_entry__ as g
        g.build()
    return L


def test_new_entry_points_refuse_bad_arguments_without_a_launch(lib):
    L = lib.load()
    p = ctypes.c_void_p(16)                 # never dereferenced: every call below fails its argument check
    # seg_pitch not a multiple of 64
    assert L.sda_clip_grad_y(p, p, p, p, p, 4, 0, p, 64, 4, 48, p, 4, 4, lib.BF16, None) == -1
    assert b"clip_grad_y" in L.sda_last_error()
    # columns do not cover the rows
    assert L.sda_clip_grad_y(p, p, p, p, p, 4, 0, p, 64, 4, 64, p, 100, 4, lib.BF16, None) == -1
    # fewer norms than local columns
    assert L.sda_clip_grad_y(p, p, p, p, p, 2, 0, p, 64, 4, 64, p, 4, 4, lib.F32, None) == -1
    assert L.sda_clip_grad_y(None, p, p, p, p, 4, 0, p, 64, 4, 64, p, 4, 4, lib.F32, None) == -1
    # a row range outside the batch
    assert L.sda_clip_grad_y_finish(p, 1, 8, p, p, 8, p, 0.5, 6, 4, p, p, None) == -1
    assert b"clip_grad_y_finish" in L.sda_last_error()
    assert L.sda_unpack_rows_typed(p, p, 2, 10, 5, 60, lib.BF16, lib.F32, None) == -1      # Cp not a multiple of 64
    assert L.sda_unpack_rows_typed(p, p, 2, 10, 5, 64, lib.BF16, 7, None) == -1            # unknown output dtype
