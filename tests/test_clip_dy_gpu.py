"""CLIPLoss's gradient for its first argument (the speech embeddings) on the MI355X: the reference's own numbers
(tests/golden/clip_grad.npz), every dY GEMM route and dtype against float64 autograd on the same rounded operands, every
argument form (plain tensors of each dtype, the row-layout output of a second BrainEncoder with its buffer contract, swapped
arguments), unchanged bits and launches for everything else, prefetch and ring-slot rules, and a few joint training steps of
a speech module, the encoder and temp against CPU float64 autograd."""
import pytest
import torch

pytestmark = pytest.mark.gpu

from oracle import brain_oracle as O      # noqa: E402
from tests import builders as TB          # noqa: E402
from tests import golden_io as G           # noqa: E402
from tests.parity import rel_l2            # noqa: E402

DEV = "cuda:0"
DT = {"fp32": torch.float32, "bf16": torch.bfloat16, "fp16": torch.float16}
GRAD_REL_L2 = {"fp32": 1e-5, "bf16": 6e-2, "fp16": 8e-3}      # every gradient 6e-2 / 8e-3 in the 16-bit modes
CASES = [("fast-mean", True, "mean"), ("fast-sum", True, "sum"), ("slow-mean", False, "mean"), ("slow-sum", False, "sum")]
TOY = dict(TB.TOY, B=6)


def clip(reduction="mean", temp=2.0):
    return TB.clip_loss(temp, DEV, reduction)


def ref_clip(x, y, temp, fast=True, reduction="mean"):
    """float64 autograd of the reference's formula on the given values: (loss, dx, dy, dtemp)."""
    x = x.detach().double().cpu().requires_grad_(True)
    y = y.detach().double().cpu().requires_grad_(True)
    t = torch.tensor([float(temp)], dtype=torch.float64, requires_grad=True)
    B = x.shape[0]
    X, Y = x.reshape(B, -1), y.reshape(B, -1)
    lg = (X / X.norm(dim=1, keepdim=True)) @ (Y / Y.norm(dim=1, keepdim=True)).T
    if fast:
        lg = lg * torch.exp(t)
    tgt = torch.arange(B)
    ce = torch.nn.functional.cross_entropy
    loss = (ce(lg, tgt, reduction=reduction) + ce(lg.T, tgt, reduction=reduction)) / 2
    dx, dy, dt = torch.autograd.grad(loss, [x, y, t], allow_unused=True)
    return loss.detach(), dx, dy, (dt if dt is not None else torch.zeros(1, dtype=torch.float64))


def packed(x, dtype):
    """(B, F, T) -> the rows view of a fresh row-layout buffer of `dtype` whose BUFFER is the leaf (what an encoder hands out)."""
    from speech_decoding_amd import lib as L, ops
    B, F, T = x.shape
    buf = ops.new_rows(B, T, L.pad_channels(F), dtype, DEV)
    ops.pack_rows(x.to(DEV).float(), buf)
    buf.requires_grad_(True)
    return buf, ops.rows_view(buf, B, F, T)


def is_rows_view(t):
    from speech_decoding_amd import ops
    return ops.rows_base(t, *t.shape, t.dtype) is not None


def randn(*shape, seed):
    return torch.randn(*shape, generator=torch.Generator().manual_seed(seed))


# ------------------------------------------------------------------------------------------------------------------------------
# 1. the reference's numbers
# ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", [c[0] for c in CASES])
def test_golden_fixture_fp32(case):
    _, fast, reduction = next(c for c in CASES if c[0] == case)
    g = G.load("clip_grad.npz")
    for i in range(len(g["shapes"])):
        crit = clip(reduction, float(g["temps"][i]))
        x = torch.from_numpy(g[f"s{i}/x"]).to(DEV).requires_grad_(True)
        y = torch.from_numpy(g[f"s{i}/y"]).to(DEV).requires_grad_(True)
        loss = crit(x, y, fast=fast)
        loss.backward()
        k = f"s{i}/{case}"
        want = float(g[f"{k}/loss"])
        assert abs(float(loss) - want) <= 1e-4 * abs(want), (k, float(loss), want)
        for got, key in ((x.grad, "dx"), (y.grad, "dy")):
            ref = torch.from_numpy(g[f"{k}/{key}"])
            assert got.dtype == torch.float32 and tuple(got.shape) == tuple(ref.shape)
            err = float((got.cpu() - ref).abs().max())
            assert err <= 1e-4 * float(ref.abs().max()), (k, key, err)
        dt = float(g[f"{k}/dtemp"][0])
        if fast:
            assert abs(float(crit.temp.grad) - dt) <= 1e-4 * max(1.0, abs(dt)), (k, float(crit.temp.grad), dt)
        else:
            assert crit.temp.grad is None                  # fast=False does not use temp (as the reference)


# ------------------------------------------------------------------------------------------------------------------------------
# 2. every dY GEMM route and dtype against float64 on the same rounded operands
# ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", ["fp32", "bf16", "fp16"])
@pytest.mark.parametrize("B", [6, 288], ids=["streaming", "tiles"])
def test_routes_and_dtypes_against_float64(B, dtype):
    from speech_decoding_amd import lib as L
    F, T = 64, 40                                           # 56 rows of 64 channels: whole 256-element tiles
    row_elems = L.rows_tp(T) * L.pad_channels(F)
    served = bool(L.load().sda_clip_dz_supported(B, B, row_elems, L.F32 if dtype == "fp32" else L.BF16))
    assert served == (dtype != "fp32")                     # 16-bit: clip_dz (B <= 256) / clip_dz_tiles; fp32: wgrad_gemm
    x = randn(B, F, T, seed=B).to(DT[dtype]).to(DEV).requires_grad_(True)
    y = randn(B, F, T, seed=B + 1).to(DT[dtype]).to(DEV).requires_grad_(True)
    crit = clip("mean", 2.5)
    loss = crit(x, y)
    dx, dy, dt = torch.autograd.grad(loss, [x, y, crit.temp])
    assert dx.dtype == DT[dtype] and dx.is_contiguous() and tuple(dx.shape) == (B, F, T)
    lr, dxr, dyr, dtr = ref_clip(x, y, 2.5)
    bound = GRAD_REL_L2[dtype]
    assert rel_l2(dx, dxr) <= bound, rel_l2(dx, dxr)
    assert rel_l2(dy, dyr) <= bound, rel_l2(dy, dyr)
    assert abs(float(loss) - float(lr)) <= (1e-5 if dtype == "fp32" else 1e-2) * abs(float(lr))
    if dtype == "fp32":
        assert abs(float(dt) - float(dtr)) <= 1e-4 * max(1.0, abs(float(dtr)))


def test_fp16_loss_scale_reaches_dx():
    """dloss arrives as the GEMM epilogue's out_scale: (s * loss).backward() gives s * dx."""
    x = randn(6, 64, 30, seed=1).half().to(DEV).requires_grad_(True)
    y = randn(6, 64, 30, seed=2).half().to(DEV)
    crit = clip()
    (dx1,) = torch.autograd.grad(crit(x, y), [x])
    (dx8,) = torch.autograd.grad(crit(x, y) * 8.0, [x])
    assert rel_l2(dx8, dx1.float() * 8.0) <= 1e-3          # (exact but where 16-bit subnormals round differently)
    assert float(dx8.float().abs().max()) > 4.0 * float(dx1.float().abs().max())


# ------------------------------------------------------------------------------------------------------------------------------
# 3. every argument form
# ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("xdtype", ["fp32", "bf16", "fp16"])
def test_plain_x_of_each_dtype_gets_its_own_dtype(xdtype):
    B, F, T = 5, 70, 33
    x = randn(B, F, T, seed=3).to(DT[xdtype]).to(DEV).requires_grad_(True)
    y = randn(B, F, T, seed=4).to(DEV).requires_grad_(True)          # compute dtype: y's (fp32)
    crit = clip("sum", 1.0)
    dx, dy = torch.autograd.grad(crit(x, y), [x, y])
    assert dx.dtype == DT[xdtype] and dx.is_contiguous()
    _, dxr, dyr, _ = ref_clip(x, y, 1.0, reduction="sum")
    assert rel_l2(dx, dxr) <= {"fp32": 1e-5, "bf16": 8e-3, "fp16": 1e-3}[xdtype]
    assert rel_l2(dy, dyr) <= 1e-5


def test_swapped_arguments():
    """loss(Z, Y): the encoder's row-layout output first, a plain tensor second; the compute dtype is the second argument's."""
    B, F, T = 6, 64, 40
    _, Zv = packed(randn(B, F, T, seed=5), torch.bfloat16)
    Y = randn(B, F, T, seed=6).bfloat16().to(DEV).requires_grad_(True)
    crit = clip()
    dZ, dY = torch.autograd.grad(crit(Zv, Y), [Zv, Y])
    assert is_rows_view(dZ) and dZ.dtype == torch.bfloat16                # first argument: its own row layout back
    assert dY.dtype == torch.bfloat16
    _, dzr, dyr, _ = ref_clip(Zv, Y, 2.0)
    assert rel_l2(dZ, dzr) <= GRAD_REL_L2["bf16"] and rel_l2(dY, dyr) <= GRAD_REL_L2["bf16"]
    # a first argument in another dtype than the second: packed, and its gradient comes back as a plain tensor of its dtype
    Yf = Y.detach().float().requires_grad_(True)
    dZ2, dY2 = torch.autograd.grad(crit(Zv, Yf), [Zv, Yf])
    assert dZ2.dtype == torch.bfloat16 and dZ2.is_contiguous() and not is_rows_view(dZ2)
    assert rel_l2(dZ2, dzr) <= 8e-3 and rel_l2(dY2, dyr) <= 1e-5          # fp32 compute, one rounding of dZ to bf16


@pytest.mark.parametrize("dtype", ["bf16", "fp32"])
def test_rows_dx_buffer_contract_on_poisoned_memory(dtype):
    from speech_decoding_amd import lib as L
    from speech_decoding_amd import ops
    B, F, T = 5, 100, 45
    Cp = L.pad_channels(F)
    _, x = packed(randn(B, F, T, seed=7), DT[dtype])
    _, y = packed(randn(B, F, T, seed=8), DT[dtype])
    crit = clip()
    for _ in range(2):
        nbytes = L.rows_alloc(B, T) * Cp * torch.finfo(DT[dtype]).bits // 8
        junk = torch.full((nbytes // 4,), float("nan"), dtype=torch.float32, device=DEV)
        del junk                                  # the backward's buffer comes back out of this NaN-filled block
        (dx,) = torch.autograd.grad(crit(x, y), [x])
        assert is_rows_view(dx)
        buf = ops.rows_base(dx, B, F, T, DT[dtype]).float().cpu()
        Tp = L.rows_tp(T)
        valid = torch.zeros(buf.shape[0], dtype=torch.bool)
        for b in range(B):
            valid[b * Tp + L.ROW_PAD: (b + 1) * Tp] = True
        assert bool(torch.isfinite(buf).all())
        assert bool((buf[~valid] == 0).all())                      # pad rows and the slack behind the last sample
        assert bool((buf[valid][:, F:] == 0).all())               # pad channels
        assert not bool(torch.signbit(buf[:, F:]).any())           # +0, not -0
        _, dxr, _, _ = ref_clip(x, y, 2.0)
        assert rel_l2(dx, dxr) <= GRAD_REL_L2[dtype]


def build_encoder(P, d, seed_drop=4):
    enc = TB.build_encoder(P, d, DEV)
    enc.set_drop_centre(seed_drop)
    return enc


def test_two_brain_encoders_brain_to_brain():
    """Two trainable towers: the first argument is a second BrainEncoder's row-layout output; its dY goes back into that
    encoder zero-copy, and the encoder's parameter gradients equal a separate backward of the same dY."""
    d = TOY
    _, P1, X1, _, subj = TB.toy_problem(d, d["B"])
    _, P2, X2, _, _ = TB.toy_problem(d, d["B"], param_seed=12, batch_seed=13)
    enc1, enc2 = build_encoder(P1, d), build_encoder(P2, d)
    crit = clip()
    Z = enc1(X1.to(DEV), subj)
    Y = enc2(X2.to(DEV), subj)
    assert is_rows_view(Y) and is_rows_view(Z)
    loss = crit(Y, Z)
    dY, dZ = torch.autograd.grad(loss, [Y, Z], retain_graph=True)
    assert is_rows_view(dY)
    _, dyr, dzr, _ = ref_clip(Y, Z, 2.0)
    assert rel_l2(dY, dyr) <= 1e-5 and rel_l2(dZ, dzr) <= 1e-5
    loss.backward()
    g_joint = {n: p.grad.clone() for n, p in enc2.named_parameters()}
    assert all(bool(torch.isfinite(torch.view_as_real(g) if g.is_complex() else g).all()) for g in g_joint.values())
    enc2b = build_encoder(P2, d)
    Yb = enc2b(X2.to(DEV), subj)
    Yb.backward(dY.detach())
    for n, p in enc2b.named_parameters():
        a, b = g_joint[n], p.grad
        a, b = (torch.view_as_real(a), torch.view_as_real(b)) if a.is_complex() else (a, b)
        assert float((a - b).abs().max()) <= 1e-6 * float(b.abs().max()) + 1e-12, n


# ------------------------------------------------------------------------------------------------------------------------------
# 4. bits and launches
# ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", ["bf16", "fp32"])
def test_dz_dtemp_loss_bits_do_not_depend_on_x_requiring_grad(dtype):
    B, F, T = 6, 64, 40
    xv = randn(B, F, T, seed=21).to(DEV)
    _, Z = packed(randn(B, F, T, seed=22), DT[dtype])
    outs = []
    for want_x in (False, True, True):
        crit = clip()
        x = xv.clone().requires_grad_(want_x)
        loss = crit(x, Z)
        grads = torch.autograd.grad(loss, [Z, crit.temp] + ([x] if want_x else []))
        outs.append((loss.detach().clone(), grads[0].detach().clone(), grads[1].clone(), grads[2].clone() if want_x else None))
    for o in outs[1:]:
        assert torch.equal(o[0], outs[0][0]) and torch.equal(o[1], outs[0][1]) and torch.equal(o[2], outs[0][2])
    assert torch.equal(outs[1][3], outs[2][3])                     # two identical calls: identical dx bits


def test_x_without_grad_never_calls_the_new_entry_points(monkeypatch):
    from speech_decoding_amd import clip as clip_schedule, ops

    def boom(*a, **k):
        raise AssertionError("speech-side gradient kernel called although x needs no gradient")

    for mod, name in ((ops, "clip_grad_y"), (ops, "clip_grad_y_finish"), (ops, "unpack_rows"), (clip_schedule, "clip_backward_y")):
        monkeypatch.setattr(mod, name, boom)
    x = randn(6, 64, 40, seed=31).to(DEV)
    y = randn(6, 64, 40, seed=32).to(DEV).requires_grad_(True)
    crit = clip()
    crit(x, y).backward()
    assert y.grad is not None and crit.temp.grad is not None
    xl = x.clone().requires_grad_(True)
    with torch.no_grad():                                    # (an evaluation pass: a leaf that requires a gradient, no graph)
        assert torch.equal(crit(xl, y), crit(x, y))


def test_ring_slot_rule_covers_dx():
    """A backward later than `ring_depth` forwards raises even when only x needs a gradient (dY reads the packed rows)."""
    from speech_decoding_amd.lib import SdaError
    y = randn(6, 64, 40, seed=41).to(DEV)
    crit = clip()
    xs = [randn(6, 64, 40, seed=42 + k).to(DEV).requires_grad_(True) for k in range(3)]
    losses = [crit(x, y) for x in xs]
    with pytest.raises(SdaError, match="recycled"):
        losses[0].backward()
    losses[2].backward()                                     # the newest is fine
    assert xs[2].grad is not None


def test_prefetch_equals_no_prefetch():
    B, F, T = 6, 64, 40
    xv = randn(B, F, T, seed=51).to(DEV)
    yv = randn(B, F, T, seed=52).to(DEV)
    res = []
    for pre in (False, True):
        crit = clip()
        x, y = xv.clone().requires_grad_(True), yv.clone().requires_grad_(True)
        if pre:
            crit.prefetch(x, torch.float32)
        loss = crit(x, y)
        res.append((loss.detach(),) + torch.autograd.grad(loss, [x, y, crit.temp]))
        crit.drain()
    for a, b in zip(*res):
        assert torch.equal(a, b)


# ------------------------------------------------------------------------------------------------------------------------------
# 5. joint training: a speech module, the encoder and temp
# ------------------------------------------------------------------------------------------------------------------------------
def test_joint_adam_steps_match_cpu_float64():
    d = TOY
    loc, P, X, _, subj = TB.toy_problem(d, d["B"])
    M = randn(d["B"], 20, d["T"], seed=61)                  # a Mel-spectrogram-like speech input
    torch.manual_seed(0)
    speech = torch.nn.Sequential(torch.nn.Conv1d(20, d["F"], 3, padding=1), torch.nn.GELU(), torch.nn.Conv1d(d["F"], d["F"], 1))
    speech64 = torch.nn.Sequential(torch.nn.Conv1d(20, d["F"], 3, padding=1), torch.nn.GELU(), torch.nn.Conv1d(d["F"], d["F"], 1))
    speech64.load_state_dict(speech.state_dict())
    speech64 = speech64.double()
    enc = build_encoder(P, d)
    speech = speech.to(DEV)
    crit = clip("mean", 2.0)
    lr = 3e-4
    opt = torch.optim.Adam(list(speech.parameters()) + list(enc.parameters()) + list(crit.parameters()), lr=lr)
    # the same steps in float64 on the CPU through the oracle's encoder
    leaves = {k: (v.detach().to(torch.complex128) if v.is_complex() else v.detach().double()).clone().requires_grad_(True)
              for k, v in P.items() if (v.is_floating_point() or v.is_complex())
              and not k.endswith(("running_mean", "running_var", ".cos", ".sin"))}
    Q = {k: (v.to(torch.complex128) if v.is_complex() else v.double()) if (v.is_floating_point() or v.is_complex()) else v
         for k, v in P.items()}
    t64 = torch.tensor([2.0], dtype=torch.float64, requires_grad=True)
    opt64 = torch.optim.Adam(list(speech64.parameters()) + list(leaves.values()) + [t64], lr=lr)
    Md, Xd = M.to(DEV), X.to(DEV)
    for step in range(3):
        enc.set_drop_centre(4)
        Y = speech(Md)
        loss = crit(Y, enc(Xd, subj))
        opt.zero_grad()
        loss.backward()
        opt.step()
        Q.update(leaves)
        Z64 = O.brain_encoder_forward(Q, X.double(), subj, training=True, loc=loc.double(), drop_centre=4)
        l64, _ = O.clip_loss(speech64(M.double()), Z64, t64)
        opt64.zero_grad()
        l64.backward()
        opt64.step()
        assert abs(float(loss) - float(l64)) <= (1e-4 if step == 0 else 2e-3) * abs(float(l64)), (step, float(loss), float(l64))
    lim = 3 * 4 * lr                                         # Adam moves noise-gradient entries by about lr per step
    for (n, p), p64 in zip(speech.named_parameters(), speech64.parameters()):
        assert float((p.detach().cpu().double() - p64.detach()).abs().max()) < lim, n
    sd = enc.state_dict()
    for k, v in leaves.items():
        got, ref = sd[k].cpu(), v.detach()
        if ref.is_complex():
            got, ref = torch.view_as_real(got), torch.view_as_real(ref)
        assert float((got.double() - ref).abs().max()) < lim, k
    assert abs(float(crit.temp) - float(t64)) < lim
    assert float(crit.temp) != 2.0                           # temp moved
