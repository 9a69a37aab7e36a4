"""CPU checks of X's gradient through BrainEncoder: the committed fixture (the reference's own BrainEncoder + CLIPLoss, autograd
on X, tests/golden/encoder_dx.npz) agrees with the oracle's float64 autograd, and sda_input_grad refuses bad arguments without
launching anything."""
import ctypes

import pytest
import torch

from oracle import brain_oracle as O
from tests import golden_io as G
from tests.builders import TOY, encoder_args


def fixture_case(npz, i):
    """(dims, loc, P, X, Y, subj, centre) of fixture shape i; P rebuilt from the stored seeds and checked against its sums."""
    C, S, D1, D2, F, K, T, B = (int(v) for v in npz[f"s{i}/dims"])
    loc_seed, param_seed, _ = (int(v) for v in npz["seeds"])
    loc = O.synthetic_positions(C, seed=loc_seed)
    P = O.seeded_params(C, S, D1, D2, F, K, seed=param_seed, loc=loc)
    for key, v in P.items():
        if f"s{i}/psum/{key}" in npz:
            got = float(torch.view_as_real(v).double().sum() if v.is_complex() else v.double().sum())
            assert got == pytest.approx(float(npz[f"s{i}/psum/{key}"]), rel=1e-12, abs=1e-12), key
    X, Y = torch.from_numpy(npz[f"s{i}/X"]), torch.from_numpy(npz[f"s{i}/Y"])
    subj = torch.from_numpy(npz[f"s{i}/subject_idxs"])
    return dict(C=C, S=S, D1=D1, D2=D2, F=F, K=K, T=T, B=B), loc, P, X, Y, subj, int(npz[f"s{i}/drop_centre"])


def oracle_dx(P, X, Y, subj, loc, centre, temp, training):
    """float64 autograd of the oracle encoder + CLIP loss with respect to X: (loss, Z, dX)."""
    Q = {k: (v.to(torch.complex128) if v.is_complex() else v.double()) if (v.is_floating_point() or v.is_complex()) else v
         for k, v in P.items()}
    Xd = X.double().requires_grad_(True)
    Z = O.brain_encoder_forward(Q, Xd, subj, training=training, loc=loc.double(), drop_centre=centre if training else None)
    loss, _ = O.clip_loss(Y.double(), Z, torch.tensor([temp], dtype=torch.float64))
    (dX,) = torch.autograd.grad(loss, [Xd])
    return loss.detach(), Z.detach(), dX


@pytest.mark.parametrize("mode", ["train", "eval"])
@pytest.mark.parametrize("i", [0, 1])
def test_fixture_dx_matches_float64_oracle(i, mode):
    npz = G.load("encoder_dx.npz")
    d, loc, P, X, Y, subj, centre = fixture_case(npz, i)
    assert (d["C"] < 64) == (i == 0)                          # s0 composes the SubjectBlock, s1 (C = Cp) runs the three convs
    if mode == "eval":
        P.update(G.state_from(npz, f"s{i}/eval/state/"))
    loss, Z, dX = oracle_dx(P, X, Y, subj, loc, centre, float(npz["temp"]), mode == "train")
    want = torch.from_numpy(npz[f"s{i}/{mode}/dX"]).double()
    assert abs(float(loss) - float(npz[f"s{i}/{mode}/loss"])) <= 1e-5 * abs(float(loss))
    zref = torch.from_numpy(npz[f"s{i}/{mode}/Z"]).double()
    assert float((Z - zref).abs().max()) <= 1e-4 * float(zref.abs().max())
    scale = float(dX.abs().max())
    assert scale > 0
    assert float((want - dX).abs().max()) <= 1e-4 * scale, (i, mode, float((want - dX).abs().max()), scale)
    if mode == "train":                                       # dropped sensors get exactly zero
        dropped = O.dropout_mask(loc, centre, 0.1) == 0
        assert int(dropped.sum()) >= 2
        assert float(want[:, dropped].abs().max()) == 0.0


def test_input_grad_rejects_bad_arguments_without_launch():
    from speech_decoding_amd import lib
    L = lib.load()
    buf = (ctypes.c_char * 4096 * 4)()                        # host memory that no kernel may ever see: every call below must fail
    p = ctypes.cast(buf, ctypes.c_void_p).value
    p = (p + 15) // 16 * 16
    ok = dict(G=p, g_pitch=64, W=p, widx=None, nW=1, Kp=64, Cp=64, B=2, C=20, T=10, dtype=lib.F32, out=p, out_dtype=lib.F32)

    def call(**kw):
        a = dict(ok, **kw)
        return L.sda_input_grad(a["G"], a["g_pitch"], a["W"], a["widx"], a["nW"], a["Kp"], a["Cp"], a["B"], a["C"], a["T"],
                                a["dtype"], a["out"], a["out_dtype"], None)

    cases = [(dict(G=None), b"null"), (dict(W=None), b"null"), (dict(out=None), b"null"),
             (dict(dtype=3), b"dtype"), (dict(out_dtype=-1), b"dtype"),
             (dict(B=0), b"sizes"), (dict(C=0), b"sizes"), (dict(T=0), b"sizes"), (dict(nW=0), b"sizes"),
             (dict(Kp=48), b"multiple"), (dict(Cp=96), b"multiple"), (dict(C=65), b"multiple"), (dict(g_pitch=32), b"pitch"),
             (dict(G=p + 4), b"aligned"), (dict(W=p + 8), b"aligned"), (dict(nW=3), b"indices")]
    for kw, msg in cases:
        assert call(**kw) == -1, kw
        assert msg in L.sda_last_error(), (kw, L.sda_last_error())


def test_x_of_another_dtype_requiring_grad_is_refused_before_any_launch():
    """float64 X with requires_grad: a clear error at forward time (the dtype check comes before the device check)."""
    from speech_decoding_amd import lib
    from speech_decoding_amd.models import BrainEncoder

    d = TOY
    enc = BrainEncoder(encoder_args(d, O.synthetic_positions(d["C"], seed=1)))
    X = torch.zeros(2, d["C"], 8, dtype=torch.float64, requires_grad=True)
    with pytest.raises(lib.SdaError, match="float64"):
        enc(X, torch.zeros(2, dtype=torch.int64))
