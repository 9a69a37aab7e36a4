"""Kernel-level tests of the wav2vec 2.0 embedder's HIP kernels (csrc/w2v2.hip) on a real MI355X: each of the seven kernels
launched directly, in fp32, bf16 and fp16, against float64 on the operands as the kernel reads them (rounded to the compute
dtype first), within test_kernels_gpu.tol(dtype).  Moves and in-order sums are compared bit for bit.  The inputs, references
and the proof that the designed attention / LayerNorm inputs catch a subtly wrong kernel are in tests/w2v2_cases.py and
tests/test_w2v2_kernels_cpu.py.

Template branch -> case that launches it (E = float / bf16 / fp16 everywhere; "chunks" = 16-byte chunks per row, Cp / 4 or Cp / 8):
  w2v_conv0_kernel<E, 2>       C = 64, 70, 130 (ceil(C / 64) <= 2)      test_conv0
  w2v_conv0_kernel<E, 8>       C = 512                                  test_conv0
  w2v_conv0_kernel<E, 16>      C = 1024                                 test_conv0
  layernorm_rows_kernel<E, 1>  fp32 Cp = 64, 128; 16-bit Cp = 64 .. 512 test_layernorm
  layernorm_rows_kernel<E, 2>  fp32 Cp = 512; 16-bit Cp = 1024          test_layernorm (fp16 on NI = 2: (1000, 1024), (1024, 1024))
  layernorm_rows_kernel<E, 4>  fp32 Cp = 1024; 16-bit Cp = 1088, 2048   test_layernorm
  the grid-stride loop of layernorm_rows (T > 4096 x 4 rows)            test_layernorm_more_rows_than_the_grid_covers
  group_split_kernel<E>, group_merge_add_kernel<E>                      test_group_split / test_group_merge_add / round trip
  attention_kernel<E>          NKQ = 4 (fp32) / 2 (16-bit)              test_attention
  splitk_epilogue_kernel<E>                                             test_splitk_epilogue
  mean4_kernel<E>                                                       test_mean4
and the three raw-GEMM forms Wav2Vec2Embedder._forward builds on ops.gemm_view: test_gemm_view_*."""
import math

import pytest
import torch
import torch.nn.functional as TF

from tests import w2v2_cases as W
from tests.test_kernels_gpu import tol

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
DTYPES = W.DTYPES
SENT = -7.0                  # sentinel: representable in every dtype
WORST = {}                   # (kernel, dtype) -> [max |error|, max error / tolerance], printed when the module is done


@pytest.fixture(scope="module")
def ops():
    from speech_decoding_amd import ops as _ops
    from speech_decoding_amd import lib
    lib.load()
    assert torch.cuda.is_available(), "these tests need the MI355X"
    yield _ops
    print("\nworst error per kernel and dtype (max |got - ref|, max |got - ref| / (atol + rtol |ref|)):")
    for (kern, dt), (e, r) in sorted(WORST.items(), key=lambda kv: (kv[0][0], str(kv[0][1]))):
        print(f"  {kern:24s} {str(dt):16s} {e:.3e}  {r:.3f}")


def check(kern, dtype, got, ref, what=""):
    """got within tol(dtype) of the float64 ref; the figures are recorded (and printed) before the assertion"""
    got, ref = got.double().cpu(), ref.double().cpu()
    ratio = W.tol_ratio(got, ref, **tol(dtype))
    err = float((got - ref).abs().max()) if math.isfinite(ratio) else float("inf")
    w = WORST.setdefault((kern, dtype), [0.0, 0.0])
    w[0], w[1] = max(w[0], err), max(w[1], ratio)
    print(f"{kern} {dtype} {what}: max err {err:.3e}, err / tol {ratio:.3f}")
    assert ratio <= 1.0, (kern, dtype, what, err, ratio)


def es(dtype):
    return 4 if dtype == torch.float32 else 2


def rows_alloc(T):
    from speech_decoding_amd import lib as L
    return L.rows_alloc(1, T)


def row_buf(T, Cp, dtype, fill=0.0):
    return torch.full((rows_alloc(T), Cp), fill, dtype=dtype, device=DEV)


def put(buf, T, x):
    """x (T, C) float32 on the CPU -> valid rows of a row-layout buffer, columns < C"""
    from speech_decoding_amd import lib as L
    buf[L.ROW_PAD:L.ROW_PAD + T, :x.shape[1]] = x.to(buf.dtype).to(DEV)
    return buf


def untouched(buf, T, C, value):
    """every element outside rows [ROW_PAD, ROW_PAD + T) x columns [0, C) still holds `value`"""
    from speech_decoding_amd import lib as L
    m = buf.detach().to("cpu", torch.float32, copy=True)
    m[L.ROW_PAD:L.ROW_PAD + T, :C] = value
    return bool((m == value).all())


# ---------------------------------------------------------------------------------------------------------------
# attention
# ---------------------------------------------------------------------------------------------------------------
def _run_attention(ops, qh, kh, vt_cpu, T, heads, dtype, layout):
    from speech_decoding_amd import lib as L
    PAD, W64 = L.ROW_PAD, heads * 64
    rl = lambda x: x.permute(1, 0, 2).reshape(T, W64)                      # head h in columns [64 h, 64 h + 64)
    if layout == "interleaved":                                           # q | k in one buffer at pitch 2 Hp, Hp > heads * 64
        Hp = W64 + 64
        qk = row_buf(T, 2 * Hp, dtype, fill=3.0)
        put(qk, T, rl(qh))
        qk[PAD:PAD + T, Hp:Hp + W64] = rl(kh).to(dtype).to(DEV)
        q_ptr, k_ptr, pitch, out_pitch, keep = qk.data_ptr(), qk.data_ptr() + Hp * es(dtype), 2 * Hp, Hp, qk
    else:                                                                 # separate buffers, tight pitch
        qb, kb = put(row_buf(T, W64, dtype, fill=3.0), T, rl(qh)), put(row_buf(T, W64, dtype, fill=3.0), T, rl(kh))
        q_ptr, k_ptr, pitch, out_pitch, keep = qb.data_ptr(), kb.data_ptr(), W64, W64, (qb, kb)
    vt = vt_cpu.to(dtype).to(DEV).contiguous()
    out = row_buf(T, out_pitch, dtype, fill=SENT)
    ops.w2v_attention(q_ptr, k_ptr, vt, out, T, heads, 64, pitch, 0.125)
    torch.cuda.synchronize()
    assert untouched(out, T, W64, SENT), "attention wrote outside its rows / columns"
    return out[PAD:PAD + T, :W64].float().cpu().reshape(T, heads, 64).permute(1, 0, 2)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("heads", W.ATT_HEADS)
@pytest.mark.parametrize("T", W.ATT_T)
def test_attention(ops, T, heads, dtype):
    for layout in ("interleaved", "separate"):
        Tp = W.ceil64(T) + (0 if layout == "interleaved" else 8)          # the second layout: V^T rows longer than the blocks
        for name, qh, kh, vh in W.attention_cases(T, heads):
            qh, kh, vh = W.q(qh, dtype), W.q(kh, dtype), W.q(vh, dtype)
            ref = W.attention_ref(qh, kh, vh, 0.125)
            got = _run_attention(ops, qh, kh, W.vt_with_tail(vh, Tp, W.TAIL), T, heads, dtype, layout)
            zero = _run_attention(ops, qh, kh, W.vt_with_tail(vh, Tp, 0.0), T, heads, dtype, layout)
            assert torch.equal(got, zero), (name, layout, "the V^T tail reached the result")
            check("w2v_attention", dtype, got, ref, f"T={T} heads={heads} {layout} {name}")


# ---------------------------------------------------------------------------------------------------------------
# LayerNorm
# ---------------------------------------------------------------------------------------------------------------
LN_SHAPES = [(64, 64), (70, 128), (512, 512), (1000, 1024), (1024, 1024)]
LN_SHAPES_16 = [(1030, 1088), (2048, 2048)]


def _ln_params(C, seed=0):
    g = torch.Generator().manual_seed(seed + C)
    return 1.0 + 0.5 * torch.randn(C, generator=g), 0.3 * torch.randn(C, generator=g)


def _run_layernorm(ops, x, gamma, beta, Cp, dtype, gelu, inplace):
    """x (T, C) float32, representable in dtype.  Pad channels of the input hold garbage, everything outside the valid rows a
    sentinel; returns the valid rows after checking pad channels (zero) and the other rows (untouched)."""
    from speech_decoding_amd import lib as L
    T, C = x.shape
    xb = row_buf(T, Cp, dtype, fill=SENT)
    xb[L.ROW_PAD:L.ROW_PAD + T] = 1000.0
    put(xb, T, x)
    yb = xb if inplace else row_buf(T, Cp, dtype, fill=SENT)
    ops.layernorm_rows(xb, yb, gamma.to(DEV), beta.to(DEV), T, C, W.LN_EPS, gelu=gelu)
    torch.cuda.synchronize()
    y = yb.float().cpu()
    valid = y[L.ROW_PAD:L.ROW_PAD + T]
    assert Cp == C or float(valid[:, C:].abs().max()) == 0.0, "output pad channels must be exactly zero"
    assert untouched(yb, T, Cp, SENT), "layernorm_rows wrote outside its rows"
    return valid[:, :C]


def _ln_shapes():
    return [(dt, C, Cp) for dt in DTYPES for C, Cp in LN_SHAPES + (LN_SHAPES_16 if dt != torch.float32 else [])]


@pytest.mark.parametrize("dtype,C,Cp", _ln_shapes())
def test_layernorm(ops, dtype, C, Cp):
    gamma, beta = _ln_params(C)
    g = torch.Generator().manual_seed(C)
    for T in (1, 3, 4, 5, 130):
        x = W.q(1.5 * torch.randn(T, C, generator=g) + 0.3, dtype)
        for gelu in (False, True):
            ref = W.layernorm_ref(x, gamma, beta, gelu=gelu)
            for inplace in (False, True):
                got = _run_layernorm(ops, x, gamma, beta, Cp, dtype, gelu, inplace)
                check("layernorm_rows", dtype, got, ref, f"C={C} Cp={Cp} T={T} gelu={gelu} inplace={inplace}")


@pytest.mark.parametrize("dtype,C,Cp", _ln_shapes())
def test_layernorm_offset_mean(ops, dtype, C, Cp):
    """Rows around 100: std 0.1, and (power-of-two widths) all but one value equal.  A one-pass variance fails these by
    more than 10x the tolerance (tests/test_w2v2_kernels_cpu.py)."""
    gamma, beta = _ln_params(C, seed=1)
    for kind in ("std0.1", "near_constant") if C & (C - 1) == 0 else ("std0.1",):
        x = W.offset_mean_rows(5, C, kind)
        assert torch.equal(W.q(x, dtype), x)
        ref = W.layernorm_ref(x, gamma, beta)
        for inplace in (False, True):
            got = _run_layernorm(ops, x, gamma, beta, Cp, dtype, False, inplace)
            check("layernorm_rows", dtype, got, ref, f"offset mean {kind} C={C} Cp={Cp} inplace={inplace}")


@pytest.mark.parametrize("dtype", DTYPES)
def test_layernorm_more_rows_than_the_grid_covers(ops, dtype):
    T, C, Cp = 16390, 64, 64                     # 4096 workgroups x 4 waves = 16384 rows per sweep
    gamma, beta = _ln_params(C, seed=2)
    x = W.q(torch.randn(T, C, generator=torch.Generator().manual_seed(7)) + torch.arange(T)[:, None] % 5, dtype)
    got = _run_layernorm(ops, x, gamma, beta, Cp, dtype, True, False)
    check("layernorm_rows", dtype, got, W.layernorm_ref(x, gamma, beta, gelu=True), f"T={T}")


# ---------------------------------------------------------------------------------------------------------------
# conv0
# ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("C,K,stride", [(64, 10, 5), (70, 10, 5), (512, 10, 5), (1024, 10, 5), (64, 1, 1), (130, 3, 2)])
def test_conv0(ops, dtype, C, K, stride):
    from speech_decoding_amd import lib as L
    Cp = L.pad_channels(C)
    g = torch.Generator().manual_seed(C + K)
    w = torch.randn(C, K, generator=g) / math.sqrt(K)
    bias = 0.5 * torch.randn(C, generator=g)
    gamma, beta = _ln_params(C, seed=3)
    for T in (1, 5, 131):
        n = (T - 1) * stride + K                                           # not one sample more than the last frame reads
        wave = torch.randn(n, generator=g)
        for b in (None, bias):
            y = row_buf(T, Cp, dtype)
            ops.w2v_conv0(wave.to(DEV), w.to(DEV), None if b is None else b.to(DEV), gamma.to(DEV), beta.to(DEV), y, T, C, K, stride)
            torch.cuda.synchronize()
            assert untouched(y, T, C, 0.0), "conv0 wrote pad channels or pad rows"
            got = y[L.ROW_PAD:L.ROW_PAD + T, :C].float()
            check("w2v_conv0", dtype, got, W.conv0_ref(wave, w, b, gamma, beta, stride), f"C={C} K={K} s={stride} T={T} bias={b is not None}")


# ---------------------------------------------------------------------------------------------------------------
# group_split / group_merge_add
# ---------------------------------------------------------------------------------------------------------------
GROUPS = [(1, 64), (4, 32), (16, 64), (4, 8), (2, 72)]


def _group_h(T, G, gw, dtype, seed):
    from speech_decoding_amd import lib as L
    Hp = L.pad_channels(G * gw) + 64
    h = W.q(torch.randn(T, G * gw, generator=torch.Generator().manual_seed(seed)), dtype)
    hb = row_buf(T, Hp, dtype, fill=9.0)                                   # garbage around the valid block: never moved
    return h, put(hb, T, h), Hp


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("G,gw", GROUPS)
def test_group_split_is_an_exact_move(ops, dtype, G, gw):
    from speech_decoding_amd import lib as L
    gwp, lead = L.pad_channels(gw), 8 + L.ROW_PAD
    for T in (1, 17, 130):
        h, hb, _ = _group_h(T, G, gw, dtype, T)
        xg = torch.zeros((G, lead + T + 16 + 2 * L.ROW_PAD, gwp), dtype=dtype, device=DEV)
        ops.w2v_group_split(hb, xg, T, gw, G, lead)
        want = torch.zeros(xg.shape)                                       # lead rows, rows after lead + T, columns gw .. gwp: zero
        want[:, lead:lead + T, :gw] = h.reshape(T, G, gw).permute(1, 0, 2)
        assert torch.equal(xg.float().cpu(), want), (G, gw, T)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("G,gw", GROUPS)
def test_group_merge_add(ops, dtype, G, gw):
    from speech_decoding_amd import lib as L
    PAD, gwp = L.ROW_PAD, L.pad_channels(gw)
    for T in (1, 17, 130):
        g = torch.Generator().manual_seed(100 + T)
        h, hb, Hp = _group_h(T, G, gw, dtype, T)
        yv = W.q(torch.randn(G, T, gw, generator=g), dtype)
        yg = torch.full((G, PAD + T + 3, gwp), 11.0, dtype=dtype, device=DEV)      # garbage in every row and column not read
        yg[:, PAD:PAD + T, :gw] = yv.to(dtype).to(DEV)
        bias = 0.5 * torch.randn(G * gw, generator=g)
        for b in (None, bias):
            for gelu in (False, True):
                out = row_buf(T, Hp, dtype, fill=SENT)
                ops.w2v_group_merge_add(hb, yg, out, T, gw, G, bias=None if b is None else b.to(DEV), gelu=gelu)
                torch.cuda.synchronize()
                assert untouched(out, T, G * gw, SENT)
                v = yv.double().permute(1, 0, 2).reshape(T, G * gw) + (0 if b is None else b.double())
                ref = h.double() + (TF.gelu(v) if gelu else v)
                check("w2v_group_merge_add", dtype, out[PAD:PAD + T, :G * gw].float(), ref, f"G={G} gw={gw} T={T} bias={b is not None} gelu={gelu}")


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("G,gw", GROUPS)
def test_group_split_then_merge_returns_h_exactly(ops, dtype, G, gw):
    from speech_decoding_amd import lib as L
    PAD, gwp = L.ROW_PAD, L.pad_channels(gw)
    for T in (1, 17, 130):
        h, hb, Hp = _group_h(T, G, gw, dtype, 50 + T)
        xg = torch.zeros((G, PAD + T + 2, gwp), dtype=dtype, device=DEV)
        ops.w2v_group_split(hb, xg, T, gw, G, PAD)                         # lead = ROW_PAD: xg has the geometry merge reads
        a = ops.w2v_group_merge_add(row_buf(T, Hp, dtype), xg, row_buf(T, Hp, dtype, fill=SENT), T, gw, G)     # 0 + split(h)
        b = ops.w2v_group_merge_add(hb, torch.zeros_like(xg), row_buf(T, Hp, dtype, fill=SENT), T, gw, G)      # h + 0
        for out in (a, b):
            assert torch.equal(out[PAD:PAD + T, :G * gw].float().cpu(), h), (G, gw, T)
            assert untouched(out, T, G * gw, SENT)


# ---------------------------------------------------------------------------------------------------------------
# split-K epilogue, mean of four
# ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("T,Cp", [(1, 64), (129, 64), (1, 320), (129, 320)])
def test_splitk_epilogue(ops, dtype, T, Cp):
    from speech_decoding_amd import lib as L
    lib, PAD = L.load(), L.ROW_PAD
    g = torch.Generator().manual_seed(T + Cp)
    bias_v = torch.randn(Cp, generator=g).to(DEV)
    res_b = put(row_buf(T, Cp, dtype), T, torch.randn(T, Cp, generator=g))
    for ksplit in (1, 2, 7):
        part = torch.randn(ksplit, T, Cp, generator=g).to(DEV)
        for bias in (None, bias_v):
            for res in (None, res_b):
                for gelu in (False, True):
                    y = row_buf(T, Cp, dtype, fill=SENT)
                    L.check(lib.sda_splitk_epilogue(ops._p(part), ksplit, ops._p(bias), ops._p(res), ops._p(y), T, Cp, int(gelu),
                                                    ops.dt_code(dtype), ops._st()), "splitk_epilogue")
                    torch.cuda.synchronize()
                    assert untouched(y, T, Cp, SENT)
                    got = y[PAD:PAD + T]
                    v = bias.expand(T, Cp).clone() if bias is not None else torch.zeros(T, Cp, device=DEV)
                    for s in range(ksplit):                                # the kernel's order: bias, slab 0, slab 1, ...
                        v = v + part[s]
                    r = 0 if res is None else res[PAD:PAD + T].float()
                    what = f"T={T} Cp={Cp} ksplit={ksplit} bias={bias is not None} res={res is not None}"
                    if gelu:
                        check("splitk_epilogue", dtype, got.float(), TF.gelu(v.double()) + (r if res is None else r.double()), what)
                    else:                                                  # the same float32 adds, rounded once: bit-identical
                        assert torch.equal(got, (v + r).to(dtype)), what


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("C,Cp", [(50, 64), (64, 64), (200, 320)])
def test_mean4(ops, dtype, C, Cp):
    from speech_decoding_amd import lib as L
    for T in (1, 130):
        g = torch.Generator().manual_seed(T + C)
        bufs = [put(row_buf(T, Cp, dtype, fill=13.0), T, torch.randn(T, C, generator=g)) for _ in range(4)]
        got = ops.w2v_mean4(*bufs, T, C)
        a, b, c, d = (x[L.ROW_PAD:L.ROW_PAD + T, :C].float() for x in bufs)
        assert got.shape == (T, C) and got.dtype == torch.float32
        assert torch.equal(got, (((a + b) + c) + d) / 4.0), (C, Cp, T)


# ---------------------------------------------------------------------------------------------------------------
# the three gemm_view forms of Wav2Vec2Embedder._forward
# ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("k,s", [(3, 2), (2, 2)])
def test_gemm_view_strided_conv_on_overlapping_rows(ops, dtype, k, s):
    from speech_decoding_amd import lib as L
    PAD, C, Cp = L.ROW_PAD, 64, 64
    g = torch.Generator().manual_seed(10 * k + s)
    w = W.q(torch.randn(C, C, k, generator=g) / math.sqrt(C * k), dtype)   # [co][ci][tap]
    bias = 0.5 * torch.randn(C, generator=g)
    we = torch.zeros(C, k, Cp)
    we[:, :, :C] = w.permute(0, 2, 1)                                      # row co = [tap][ci padded]
    wp = we.reshape(C, k * Cp).to(dtype).to(DEV).contiguous()
    for T_out in (1, 37):
        T_in = (T_out - 1) * s + k
        x = W.q(torch.randn(T_in, C, generator=g), dtype)
        prev, cur = put(row_buf(T_in, Cp, dtype), T_in, x), row_buf(T_out, Cp, dtype)
        x_view = prev.data_ptr() - PAD * (s - 1) * Cp * es(dtype)          # view row PAD + t = rows PAD + s t ... + k - 1 of prev
        ops.gemm_view(x_view, wp.data_ptr(), cur.data_ptr(), rows=T_out, K=k * Cp, Cout_p=Cp, x_pitch=s * Cp, w_pitch=k * Cp,
                      x_row0=PAD, x_rows_limit=PAD + T_out, dtype=dtype, bias=bias.to(DEV))
        torch.cuda.synchronize()
        ref = TF.conv1d(x.double().t()[None], w.double(), bias.double(), stride=s)[0].t()
        assert ref.shape == (T_out, C)
        check("gemm_view strided conv", dtype, cur[PAD:PAD + T_out, :C].float(), ref, f"k={k} s={s} T_out={T_out}")
        assert untouched(cur, T_out, Cp, 0.0)


@pytest.mark.parametrize("dtype", DTYPES)
def test_gemm_view_swapped_roles_writes_v_transposed(ops, dtype):
    from speech_decoding_amd import lib as L
    PAD, H, Hp, T, Tp = L.ROW_PAD, 192, 192, 70, 128
    g = torch.Generator().manual_seed(5)
    wv = W.q(torch.randn(H, H, generator=g) / math.sqrt(H), dtype)
    x = W.q(torch.randn(T, H, generator=g), dtype)
    a = put(row_buf(T, Hp, dtype), T, x)
    wd = wv.to(dtype).to(DEV).contiguous()
    vt = torch.full((H, Tp), SENT, dtype=dtype, device=DEV)
    ops.gemm_view(wd.data_ptr(), a.data_ptr() + PAD * Hp * es(dtype), vt.data_ptr(), rows=H, K=Hp, Cout_p=Tp, x_pitch=Hp, w_pitch=Hp,
                  x_row0=0, x_rows_limit=H, dtype=dtype)
    torch.cuda.synchronize()
    got = vt.float().cpu()
    assert bool(torch.isfinite(got).all())                                 # columns >= T: whatever the rows behind frame T - 1 give
    check("gemm_view V^T", dtype, got[:, :T], wv.double() @ x.double().t(), "H=192 T=70 Tp=128")


@pytest.mark.parametrize("dtype", DTYPES)
def test_gemm_view_batched_groups_are_the_grouped_positional_conv(ops, dtype):
    from speech_decoding_amd import lib as L
    PAD, G, K, gw, T = L.ROW_PAD, 4, 16, 32, 37
    H, gwp = G * gw, L.pad_channels(gw)
    g = torch.Generator().manual_seed(6)
    w = W.q(torch.randn(H, gw, K, generator=g) / math.sqrt(gw * K), dtype)  # Conv1d(H, H, K, groups = G).weight
    wg = torch.zeros(G, gwp, K, gwp)
    wg[:, :gw, :, :gw] = w.view(G, gw, gw, K).permute(0, 1, 3, 2)          # per group [co][tap][ci padded]
    wd = wg.reshape(G, gwp, K * gwp).to(dtype).to(DEV).contiguous()
    h = W.q(torch.randn(T, H, generator=g), dtype)
    hb = put(row_buf(T, L.pad_channels(H), dtype), T, h)
    lead = K // 2 + PAD
    grows = lead + T + K + 2 * PAD
    # a view row is K buffer rows long and whole 128-row tiles are fetched with the row index clamped to the last buffer row:
    # K - 1 rows behind the last group are read (for outputs never stored), so they are allocated
    store = torch.zeros((G * grows + K) * gwp, dtype=dtype, device=DEV)
    xg = store[:G * grows * gwp].view(G, grows, gwp)
    yg = torch.zeros_like(xg)
    ops.w2v_group_split(hb, xg, T, gw, G, lead)
    ops.gemm_view(xg.data_ptr(), wd.data_ptr(), yg.data_ptr(), rows=T, K=K * gwp, Cout_p=gwp, x_pitch=gwp, w_pitch=K * gwp, x_row0=PAD,
                  x_rows_limit=G * grows, dtype=dtype, batch=G, sample_rows=grows, widx=torch.arange(G, dtype=torch.int32, device=DEV))
    torch.cuda.synchronize()
    got = yg[:, PAD:PAD + T, :gw].float().cpu().permute(1, 0, 2).reshape(T, H)
    check("gemm_view grouped conv", dtype, got, W.grouped_same_pad_ref(h, w, G), f"G={G} K={K} gw={gw} T={T}")
    assert float(yg[:, PAD:PAD + T, gw:].float().abs().max()) == 0.0       # zero weight rows: pad channels of a group stay zero


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_positional_conv_workspace_owns_the_rows_its_gemm_reads(dtype):
    """The batched GEMM over ws["xg"] reads up to K - 1 buffer rows behind the last group (see the test above): the
    embedder's workspace must own them, whatever else the allocator has placed there."""
    from oracle import wav2vec2_oracle as O
    from speech_decoding_amd.wav2vec2 import Wav2Vec2Config, Wav2Vec2Embedder
    kw = dict(conv_dim=(64,) * 7, hidden_size=128, num_attention_heads=2, intermediate_size=256, num_hidden_layers=4,
              num_conv_pos_embeddings=16, num_conv_pos_embedding_groups=4)
    emb = Wav2Vec2Embedder(O.random_state_dict(O.W2V2Config(**kw), 0), Wav2Vec2Config(**kw), dtype=dtype, device=DEV)
    for T in (1, 12, 300):
        xg = emb._workspace(T, [T] * 7)["xg"]
        K = kw["num_conv_pos_embeddings"]
        assert xg.is_contiguous() and xg.shape[0] == 4 and xg.shape[2] == emb.gwp
        owned = xg.untyped_storage().nbytes() - xg.storage_offset() * xg.element_size()
        assert owned >= (xg.numel() + (K - 1) * emb.gwp) * xg.element_size(), (T, owned)
        assert float(xg.float().abs().max()) == 0.0
