"""The descriptors the six GEMM wrappers of ops.py hand to sda_conv_gemm / sda_wgrad_gemm, field by field, and the conv route of
ops.splitk_plan.  The wrappers run on CPU tensors with the library replaced by a recorder that copies each descriptor and launches
nothing (the tile rules are still the library's).  The tables are the documentation of the forms: pointers as (operand, byte
offset), None = NULL, everything else as the integer the kernel reads.  They were recorded in the same way from the wrappers as
they were before ops.conv_args / ops.wgrad_args existed (each filled its struct by hand; what it left to zero-init is 0 / NULL)."""
import ctypes
import os

import pytest
import torch

from speech_decoding_amd import lib as L, ops

B, T = 2, 5
R, R1 = L.rows_alloc(B, T), L.rows_alloc(1, T)            # 218, 197
BF, F32, F16 = torch.bfloat16, torch.float32, torch.float16


@pytest.fixture
def sent(monkeypatch):
    """The list of descriptors the wrappers launch while the test runs: (entry point, copy of the struct)."""
    if not os.path.exists(L.LIB_PATH):
        import __graft_entry__ as g
        g.build()
    real, calls = L.load(), []

    class Recorder:
        def __getattr__(self, name):
            if name in ("sda_conv_tile_co", "sda_wgrad_tile_m"):
                return getattr(real, name)
            if name in ("sda_conv_gemm", "sda_wgrad_gemm"):
                return lambda ref, stream: calls.append((name, type(ref._obj).from_buffer_copy(ref._obj))) or 0
            return lambda *args: 0                                  # sda_reduce_slabs, sda_splitk_epilogue: not under test

    rec = Recorder()
    monkeypatch.setattr(L, "load", lambda: rec)
    monkeypatch.setattr(ops, "_need_cuda", lambda *ts: None)
    monkeypatch.setattr(ops, "_st", lambda: 0)
    return calls


def fields(call, entry, operands):
    """{field: value} of a recorded descriptor, addresses as (name of the operand tensor they point into, byte offset from its start)."""
    name, desc = call
    assert name == entry
    out = {}
    for f, ctype in desc._fields_:
        v = getattr(desc, f)
        if ctype is ctypes.c_void_p and v is not None:
            v = next((n, v - t.data_ptr()) for n, t in operands.items() if 0 <= v - t.data_ptr() < t.numel() * t.element_size())
        out[f] = v
    return out


def test_conv_row_layout(sent):
    t = dict(x=torch.zeros(R, 64, dtype=BF), w=torch.zeros(2, 3, 128, 64, dtype=BF), y=torch.zeros(R, 128, dtype=BF),
             bias=torch.zeros(128), res=torch.zeros(R, 128, dtype=BF), y_pre=torch.zeros(R, 128, dtype=BF),
             widx=torch.zeros(2, dtype=torch.int32))
    ops.conv_gemm(t["x"], t["w"], t["y"], B=B, T=T, KS=3, dil=2, bias=t["bias"], res=t["res"], y_pre=t["y_pre"], widx=t["widx"],
                  gelu=True, flags=L.CONV_SINGLE_TILE)
    assert len(sent) == 1 and fields(sent[0], "sda_conv_gemm", t) == dict(
        x=("x", 0), w=("w", 0), bias=("bias", 0), res=("res", 0), y=("y", 0), y_pre=("y_pre", 0), widx=("widx", 0), stats=None,
        partial=None, bn_x=None, bn_coef=None, glu_out=None, glu_gate=None, B=2, T=5, Cin_p=64, Cout_p=128, KS=3, dil=2, x_pitch=64,
        w_pitch=64, x_row0=16, x_sample_rows=21, x_rows_limit=218, w_rows_limit=128, ksplit=1, flags=4097, dtype=1)


def test_conv_row_layout_glu_backward_with_stats(sent):
    """y = [d value | d gate] is twice as wide as the conv's output channels."""
    t = dict(x=torch.zeros(R, 64), w=torch.zeros(1, 1, 64, 64), y=torch.zeros(R, 128), glu_out=torch.zeros(R, 64),
             glu_gate=torch.zeros(R, 64), stats=torch.zeros(B, 2, 128))
    ops.conv_gemm(t["x"], t["w"], t["y"], B=B, T=T, KS=1, dil=0, stats=t["stats"], glu_bwd=(t["glu_out"], t["glu_gate"]))
    assert len(sent) == 1 and fields(sent[0], "sda_conv_gemm", t) == dict(
        x=("x", 0), w=("w", 0), bias=None, res=None, y=("y", 0), y_pre=None, widx=None, stats=("stats", 0), partial=None, bn_x=None,
        bn_coef=None, glu_out=("glu_out", 0), glu_gate=("glu_gate", 0), B=2, T=5, Cin_p=64, Cout_p=64, KS=1, dil=0, x_pitch=64,
        w_pitch=64, x_row0=16, x_sample_rows=21, x_rows_limit=218, w_rows_limit=64, ksplit=1, flags=4, dtype=0)


def test_conv_split_k_matrix_mode(sent):
    """matmul_nt_splitk_into off the 256 x 256 tiles: plain (M, pitch) and (N, pitch) matrices, K slices into `partial`."""
    t = dict(xm=torch.zeros(5, 64), wm=torch.zeros(100, 64), partial=torch.zeros(2, 5, 128), out=torch.zeros(5, 128))
    ops.matmul_nt_splitk_into(t["xm"], t["wm"], 5, 100, 64, 64, False, 2, t["partial"], t["out"])
    assert len(sent) == 1 and fields(sent[0], "sda_conv_gemm", t) == dict(
        x=("xm", 0), w=("wm", 0), bias=None, res=None, y=None, y_pre=None, widx=None, stats=None, partial=("partial", 0), bn_x=None,
        bn_coef=None, glu_out=None, glu_gate=None, B=1, T=5, Cin_p=64, Cout_p=128, KS=1, dil=0, x_pitch=64, w_pitch=64, x_row0=0,
        x_sample_rows=0, x_rows_limit=5, w_rows_limit=100, ksplit=2, flags=0, dtype=0)


def test_conv_view_with_overlapping_rows_and_a_batch(sent):
    """gemm_view: raw addresses, x_pitch < K (an im2col view of a strided convolution), two problems 24 view rows apart; then its
    defaults (one problem, rows + ROW_PAD view rows, fully padded weights)."""
    t = dict(x=torch.zeros(4096, dtype=F16), w=torch.zeros(2, 128, 64, dtype=F16), y=torch.zeros(64, 128, dtype=F16),
             bias=torch.zeros(128), res=torch.zeros(64, 128, dtype=F16), widx=torch.zeros(2, dtype=torch.int32))
    ops.gemm_view(t["x"].data_ptr() + 32, t["w"].data_ptr(), t["y"].data_ptr(), rows=5, K=64, Cout_p=128, x_pitch=16, w_pitch=64,
                  x_row0=16, x_rows_limit=50, dtype=F16, bias=t["bias"], res_ptr=t["res"].data_ptr() + 256, gelu=True,
                  w_rows_limit=100, batch=2, sample_rows=24, widx=t["widx"])
    ops.gemm_view(t["x"].data_ptr(), t["w"].data_ptr(), t["y"].data_ptr(), rows=5, K=64, Cout_p=128, x_pitch=64, w_pitch=64,
                  x_row0=16, x_rows_limit=50, dtype=F16)
    assert len(sent) == 2 and fields(sent[0], "sda_conv_gemm", t) == dict(
        x=("x", 32), w=("w", 0), bias=("bias", 0), res=("res", 256), y=("y", 0), y_pre=None, widx=("widx", 0), stats=None,
        partial=None, bn_x=None, bn_coef=None, glu_out=None, glu_gate=None, B=2, T=5, Cin_p=64, Cout_p=128, KS=1, dil=0, x_pitch=16,
        w_pitch=64, x_row0=16, x_sample_rows=24, x_rows_limit=50, w_rows_limit=100, ksplit=1, flags=1, dtype=2)
    assert fields(sent[1], "sda_conv_gemm", t) == dict(
        x=("x", 0), w=("w", 0), bias=None, res=None, y=("y", 0), y_pre=None, widx=None, stats=None, partial=None, bn_x=None,
        bn_coef=None, glu_out=None, glu_gate=None, B=1, T=5, Cin_p=64, Cout_p=128, KS=1, dil=0, x_pitch=64, w_pitch=64, x_row0=16,
        x_sample_rows=21, x_rows_limit=50, w_rows_limit=128, ksplit=1, flags=0, dtype=2)


def test_conv_linear_rows_split_path(sent):
    """linear_rows with few frames: one row-layout sample, K slices into the scratch the epilogue kernel sums."""
    assert ops.k_slab(F32) == 32 and ops.k_slab(BF) == 64 and ops.k_slab(F16) == 64
    assert ops.linear_rows_ksplit(T, 128, 64, F32) == 2 and ops.linear_rows_ksplit(T, 128, 64, BF) == 1
    t = dict(x=torch.zeros(R1, 64), w=torch.zeros(1, 1, 128, 64), y=torch.zeros(R1, 128), bias=torch.zeros(128),
             res=torch.zeros(R1, 128), scratch=torch.zeros(2 * T * 128))
    ops.linear_rows(t["x"], t["w"], t["y"], T, bias=t["bias"], res=t["res"], gelu=True, scratch=t["scratch"])
    assert len(sent) == 1 and fields(sent[0], "sda_conv_gemm", t) == dict(
        x=("x", 0), w=("w", 0), bias=None, res=None, y=None, y_pre=None, widx=None, stats=None, partial=("scratch", 0), bn_x=None,
        bn_coef=None, glu_out=None, glu_gate=None, B=1, T=5, Cin_p=64, Cout_p=128, KS=1, dil=0, x_pitch=64, w_pitch=64, x_row0=16,
        x_sample_rows=21, x_rows_limit=197, w_rows_limit=128, ksplit=2, flags=0, dtype=0)


def test_wgrad_slabs_and_typed_output(sent):
    t = dict(dy=torch.zeros(R, 128, dtype=BF), x=torch.zeros(R, 64, dtype=BF), perm=torch.zeros(2, dtype=torch.int32),
             seg_start=torch.zeros(3, dtype=torch.int32))
    t["g"] = ops.wgrad_gemm(t["dy"], t["x"], B=B, T=T, KS=3, dil=1, perm=t["perm"], seg_start=t["seg_start"], nseg=2, flat_rows=True)
    assert t["g"].shape == (2, 3, 128, 64) and t["g"].dtype == F32
    assert len(sent) == 1 and fields(sent[0], "sda_wgrad_gemm", t) == dict(
        dy=("dy", 0), x=("x", 0), g=("g", 0), out_e=None, sub=None, rscale=None, out_scale=None, perm=("perm", 0),
        seg_start=("seg_start", 0), nseg=2, B=2, T=5, Cout_p=128, Cin_p=64, KS=3, dil=1, dy_pitch=128, x_pitch=64, out_pitch=0, row0=16,
        sample_rows=21, rows_limit=218, dy_zero_row=0, co_valid=0, dtype=1, acc_scale=None, flags=1)
    # matmul_tn_typed: G = columns 64 .. 191 of a (5 + 1 zero row, 192) coefficient matrix, 100 of its 128 columns real
    t = dict(G=torch.zeros(6, 192, dtype=BF), Ym=torch.zeros(5, 64, dtype=BF), out=torch.zeros(128, 64, dtype=BF),
             sub=torch.zeros(128, 64, dtype=BF), rscale=torch.zeros(128), acc_scale=torch.zeros(128), out_scale=torch.zeros(1))
    ops.matmul_tn_typed(t["G"][:, 64:192], t["Ym"], t["out"], t["sub"], t["rscale"], M_rows=5, N_valid=100, K_cols=64, pitch=64,
                        out_scale=t["out_scale"], acc_scale=t["acc_scale"])
    assert len(sent) == 2 and fields(sent[1], "sda_wgrad_gemm", t) == dict(
        dy=("G", 128), x=("Ym", 0), g=None, out_e=("out", 0), sub=("sub", 0), rscale=("rscale", 0), out_scale=("out_scale", 0),
        perm=None, seg_start=None, nseg=1, B=1, T=5, Cout_p=128, Cin_p=64, KS=1, dil=0, dy_pitch=192, x_pitch=64, out_pitch=64, row0=0,
        sample_rows=0, rows_limit=5, dy_zero_row=5, co_valid=100, dtype=1, acc_scale=("acc_scale", 0), flags=0)


def test_builders_set_every_field_from_addresses_alone():
    """ops.conv_args / ops.wgrad_args on their own: pure functions of addresses and integers (no tensor, no library, no device), the
    row layout as their defaults."""
    a = ops.conv_args(1024, 2048, 4096, B=B, T=T, Cin_p=64, Cout_p=128, KS=3, dil=1, x_pitch=64, w_pitch=64, x_rows_limit=R, dtype=L.BF16)
    assert [getattr(a, f) for f, _ in a._fields_] == [1024, 2048, None, None, 4096] + [None] * 8 + [2, 5, 64, 128, 3, 1, 64, 64, 16, 21, 218,
                                                                                           128, 1, 0, 1]
    g = ops.wgrad_args(1024, 2048, B=B, T=T, Cout_p=128, Cin_p=64, KS=3, dil=1, dy_pitch=128, x_pitch=64, rows_limit=R, dtype=L.F16, g=4096)
    assert [getattr(g, f) for f, _ in g._fields_] == [1024, 2048, 4096] + [None] * 6 + [1, 2, 5, 128, 64, 3, 1, 128, 64, 0, 16, 21, 218, 0, 0,
                                                                                      2, None, 0]


@pytest.mark.parametrize("dtype,M,N,K,ksplit", [
    (F32, 270, 256, 2048, 16),             # SpatialAttention's weights: a short contraction, capped at 16 slices
    (BF, 256, 256, 368640, 128),           # the loss's similarity matmul
    (BF, 64, 640, 4096, 16),
    (BF, 64, 640, 368640, 128)])           # 640 counted as four 160-channel tiles (the kernel's five 128-channel ones would give 103)
def test_splitk_plan_conv_route(monkeypatch, dtype, M, N, K, ksplit):
    monkeypatch.setattr(ops, "SIM_GEMM_TILES256", False)      # the conv route's arithmetic alone: no device is asked
    assert ops.splitk_tile_co(640) == 160 and ops.splitk_tile_co(256) == 128 and ops.splitk_tile_co(192) == 64
    assert ops.splitk_plan(dtype, M, N, K, K) == (False, ksplit)
