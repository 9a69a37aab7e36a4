"""The time-lagged ridge baseline on MI355X: `sda_lagged_cov_f32` (csrc/lagged_cov.hip) with torch.equal on integer operands,
its memory contract under NaN guards, the fp32 summation bound on real operands and bitwise repeatability; then
speech_decoding_amd.ridge.LaggedRidge — accumulators, coefficients, predictions and held-out retrieval — against the float64
reference of tests/ridge_cases.py fed the same fp32-rounded inputs."""
import numpy as np
import pytest
import torch

from tests import ridge_cases as RC

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
CASES = [pytest.param(*c[:5], id=f"B{c[0]}-C{c[1]}-F{c[2]}-T{c[3]}-L{c[4]}") for c in RC.KERNEL_CASES]


def _guarded(layout):
    """The lag-layout array on the device as the head of a larger allocation whose tail is NaN: a read past `rows` shows"""
    rows, Cp = layout.shape
    store = torch.full((rows + 32, Cp), float("nan"), dtype=torch.float32, device=DEV)
    store[:rows] = torch.from_numpy(layout.astype(np.float32)).to(DEV)
    return store[:rows]


def _run(a, b, L):
    """(slabs, their fixed-order fp32 sum) of both products' kernel call, the slabs pre-filled with NaN"""
    from speech_decoding_amd import ops
    n = ops.lagged_cov_slices(a.shape[0], L, a.shape[1], b.shape[1])
    out = torch.full((n, L, a.shape[1], b.shape[1]), float("nan"), dtype=torch.float32, device=DEV)
    assert ops.lagged_cov(a, b, L, L - 1, out=out) is out
    return out, ops.reduce_slabs(out)


@pytest.mark.parametrize("B,C,F,T,L", CASES)
def test_integer_operands_are_exact(B, C, F, T, L):
    X, Y = RC.ints((B, C, T), 8, 100 * L + C), RC.ints((B, F, T), 8, 100 * L + F + 1)
    a, b = RC.lag_layout(X, L - 1), RC.lag_layout(Y, L - 1)
    assert 64 * a.shape[0] < 2 ** 24                                 # every partial sum is an exact fp32 integer
    assert RC.slice_rule(a.shape[0], L, a.shape[1], b.shape[1])[0] == (5 if T == 211 else 1)
    ad, bd = _guarded(a), _guarded(b)
    for p, q, pd, qd in ((a, a, ad, ad), (a, b, ad, bd)):
        slabs, total = _run(pd, qd, L)
        assert bool(torch.isfinite(slabs).all())                     # every element of every slab was written, nothing read past the end
        ref = torch.from_numpy(RC.lagged_cov(p, q, L))
        assert ref.abs().max() > 0
        if p is q and L > 1:
            assert not torch.equal(ref[L - 1], ref[L - 1].transpose(0, 1))        # asymmetric blocks: a transposition shows
        assert torch.equal(total.cpu().to(torch.int64), ref)
        assert torch.equal(slabs.sum(dim=0, dtype=torch.float64).cpu().to(torch.int64), ref)


@pytest.mark.parametrize("B,C,F,T,L", CASES)
def test_real_operands_stay_inside_the_summation_bound_and_repeat_bitwise(B, C, F, T, L):
    rng = np.random.RandomState(7 * L + B)
    X, Y = rng.randn(B, C, T).astype(np.float32), (rng.randn(B, F, T) + 3.0).astype(np.float32)
    a, b = RC.lag_layout(X, L - 1), RC.lag_layout(Y, L - 1)
    ad, bd = _guarded(a), _guarded(b)
    for p, q, pd, qd in ((a, a, ad, ad), (a, b, ad, bd)):
        slabs, total = _run(pd, qd, L)
        assert bool(torch.isfinite(slabs).all())
        ref = RC.lagged_cov(p.astype(np.float64), q.astype(np.float64), L)
        lim = RC.cov_bound(p, q, L, slabs.shape[0])
        err = np.abs(total.cpu().numpy().astype(np.float64) - ref)
        print(f"B {B} C {C} F {F} T {T} L {L}: max err / bound = {(err / np.maximum(lim, 1e-300)).max():.3e}")
        assert (err <= lim).all()
        err64 = np.abs(slabs.sum(dim=0, dtype=torch.float64).cpu().numpy() - ref)
        assert (err64 <= lim).all()
        again, _ = _run(pd, qd, L)
        assert torch.equal(again, slabs)                             # no atomics, fixed order: the same bits


def test_wrapper_refuses_what_the_kernel_cannot_take():
    from speech_decoding_amd import SdaError, ops
    a = torch.zeros((126, 64), dtype=torch.float32, device=DEV)
    with pytest.raises(SdaError, match="zero rows"):
        ops.lagged_cov(a, a, 6, 4)
    with pytest.raises(SdaError, match="multiples of 64"):
        ops.lagged_cov(a[:, :32], a, 6, 5)
    with pytest.raises(SdaError, match="rows"):
        ops.lagged_cov(a, a[:100], 6, 5)
    with pytest.raises(SdaError, match="out must be"):
        ops.lagged_cov(a, a, 6, 5, out=torch.zeros(3, device=DEV))


# ------------------------------------------------------------------------------------------------------------ the module
L_E2E, N_TRAIN = 6, 48


@pytest.fixture(scope="module")
def world():
    """The planted world, its float64 reference fit on the first 48 segments and the module's fit of the same segments"""
    from speech_decoding_amd.ridge import LaggedRidge
    X, Y, _ = RC.planted_world()
    Xd, Yd = torch.from_numpy(X.astype(np.float32)).to(DEV), torch.from_numpy(Y.astype(np.float32)).to(DEV)
    ridge = LaggedRidge(5, 7, n_lags=L_E2E, device=DEV)
    ridge.partial_fit(Xd[:N_TRAIN], Yd[:N_TRAIN]).solve(RC.ALPHAS)
    W, ybar = RC.fit(X[:N_TRAIN], Y[:N_TRAIN], L_E2E, RC.ALPHAS)
    return dict(X=X, Y=Y, Xd=Xd, Yd=Yd, ridge=ridge, W=W, ybar=ybar)


def test_accumulators_match_the_reference(world):
    X, Y, ridge = world["X"][:N_TRAIN], world["Y"][:N_TRAIN], world["ridge"]
    A, R, s, sum_y, n = RC.moments(X, Y, L_E2E)
    a, b = RC.lag_layout(X, L_E2E - 1), RC.lag_layout(Y, L_E2E - 1)
    slabs = RC.slice_rule(a.shape[0], L_E2E, 64, 64)[0]
    assert ridge.n == n and ridge.A.dtype == ridge.R.dtype == ridge.s.dtype == ridge.sum_y.dtype == torch.float64
    assert (np.abs(ridge.A.cpu().numpy() - A) <= RC.cov_bound(a, a, L_E2E, slabs)[:, :5, :5]).all()
    assert (np.abs(ridge.R.cpu().numpy() - R) <= RC.cov_bound(a, b, L_E2E, slabs)[:, :5, :7]).all()
    assert np.abs(ridge.s.cpu().numpy() - s).max() <= 1e-12 * np.abs(X).sum()
    assert np.abs(ridge.sum_y.cpu().numpy() - sum_y).max() <= 1e-12 * np.abs(Y).sum()


def test_coefficients_stay_inside_the_perturbation_bound(world):
    X, Y, ridge = world["X"][:N_TRAIN], world["Y"][:N_TRAIN], world["ridge"]
    slabs = RC.slice_rule(N_TRAIN * (37 + L_E2E - 1), L_E2E, 64, 64)[0]
    assert ridge.alphas_ == RC.ALPHAS and tuple(ridge.coef_.shape) == (3, L_E2E, 5, 7) and ridge.coef_.dtype == torch.float32
    assert ridge.solver_ in ("device", "host")
    print(f"LaggedRidge.solve ran on the {ridge.solver_}")
    for i, alpha in enumerate(RC.ALPHAS):
        lim = 4 * RC.coef_bound(X, Y, L_E2E, alpha, slabs, world["W"][i])
        err = np.linalg.norm(ridge.coef_[i].cpu().numpy().astype(np.float64) - world["W"][i])
        print(f"alpha {alpha:g}: ||coef - ref||_F = {err:.3e}, bound {lim:.3e}, ||ref||_F = {np.linalg.norm(world['W'][i]):.3e}")
        assert err <= lim
    assert np.abs(ridge.intercept_.cpu().numpy() - world["ybar"]).max() <= 2 * RC.U * np.abs(world["ybar"]).max()


def test_predict_is_the_reference_convolution(world):
    X, ridge = world["X"][N_TRAIN:], world["ridge"]
    Z = ridge.predict(world["Xd"][N_TRAIN:])
    assert tuple(Z.shape) == (3, 16, 7, 37) and Z.dtype == torch.float32
    coef, ybar = ridge.coef_.cpu().numpy().astype(np.float64), ridge.intercept_.cpu().numpy().astype(np.float64)
    for i in range(3):
        ref = RC.predict(X, coef[i], ybar)
        # the window GEMM's bound: 1.01 K u sum |x w| over the K = L C taps that can be non-zero, one more step for the intercept
        lim = 1.01 * (L_E2E * 5 + 1) * RC.U * RC.predict(np.abs(X), np.abs(coef[i]), np.abs(ybar))
        err = np.abs(Z[i].cpu().numpy().astype(np.float64) - ref)
        print(f"alpha {RC.ALPHAS[i]:g}: max err / bound = {(err / lim).max():.3e}")
        assert (err <= lim).all()
        assert torch.equal(ridge.predict(world["Xd"][N_TRAIN:], alpha=i), Z[i])
    Xh = world["Xd"][N_TRAIN:].to(torch.bfloat16)
    assert torch.equal(ridge.predict(Xh), ridge.predict(Xh.float()))  # 16-bit segments are widened by the pack, nothing else


def test_held_out_segments_are_decoded_at_every_alpha(world):
    from speech_decoding_amd import SpeechBank
    ridge = world["ridge"]
    bank = SpeechBank.from_tensor(world["Yd"][N_TRAIN:])
    labels = torch.arange(16, device=DEV)
    results = ridge.score(world["Xd"][N_TRAIN:], bank, labels, k=10)
    assert len(results) == 3 and ridge.best_alpha_ == 0
    for alpha, r in zip(RC.ALPHAS, results):
        assert r.accuracy(1) == 1.0, alpha


def test_two_halves_accumulate_what_one_call_does():
    """Integer-valued segments: every fp32 sum inside the kernel is exact whatever the slices (they differ between one call
    and two), so what is left is the float64 accumulation, held to 1e-12."""
    from speech_decoding_amd.ridge import LaggedRidge
    X = torch.from_numpy(RC.ints((48, 5, 37), 8, 1).astype(np.float32)).to(DEV)
    Y = torch.from_numpy(RC.ints((48, 7, 37), 8, 2).astype(np.float32)).to(DEV)
    one = LaggedRidge(5, 7, n_lags=L_E2E, device=DEV).partial_fit(X, Y)
    two = LaggedRidge(5, 7, n_lags=L_E2E, device=DEV).partial_fit(X[:20], Y[:20]).partial_fit(X[20:], Y[20:])
    assert one.n == two.n == 48 * 37
    for name in ("A", "R", "s", "sum_y"):
        p, q = getattr(one, name), getattr(two, name)
        assert float(p.abs().max()) > 0 and float((p - q).abs().max()) <= 1e-12 * float(p.abs().max()), name
    A, R, s, sum_y, _ = RC.moments(X.cpu().numpy().astype(np.float64), Y.cpu().numpy().astype(np.float64), L_E2E)
    assert np.array_equal(one.A.cpu().numpy(), A) and np.array_equal(one.R.cpu().numpy(), R)
    assert np.array_equal(one.s.cpu().numpy(), s) and np.array_equal(one.sum_y.cpu().numpy(), sum_y)


def test_ridge_baseline_runs_on_train_py_data():
    """ridge_baseline.run on train.py's synthetic pool (Y = P X + 0.5 eps, an instantaneous map of unit variance: the
    prediction's cosine with its own segment is near sqrt(1 / 1.25) = 0.89, with another segment's 0 +- 1 / sqrt(F T) = 0.05, so
    every one of the 16 test segments must come out first)."""
    import ridge_baseline
    from speech_decoding_amd import load_config
    args = load_config(overrides=["dataset=Gwilliams2022", "num_subjects=2", "num_channels=6", "F=8", "preprocs.last4layers=False",
                                  "preprocs.seq_len_sec=0.5", "preprocs.baseline_len_sec=0.1", "batch_size=16",
                                  "synthetic_segments=80", "split_ratio=0.8", "ridge.n_lags=4", "ridge.alphas=[0.1,10]"])
    lines = []
    row, ridge = ridge_baseline.run(args, log=lambda *parts: lines.append("".join(parts)))
    assert ridge.n_lags == 4 and ridge.alphas_ == (0.1, 10.0) and row["train_batches"] == 4 and row["train_segments"] == 64
    assert row["testTop1acc"] == 1.0 and row["testTop10acc"] == 1.0
    assert len(lines) == 1 and "testTop10acc: 1.000" in lines[0] and "test l:" in lines[0]


@pytest.mark.parametrize("kind,extra", [("resident", []), ("tracks", ["compute_dtype=bf16"]), ("continuous", ["dataset=Brennan2018"])])
def test_ridge_baseline_takes_every_data_kind(kind, extra):
    """train.py's other feeds hand out row views, 16-bit windows of resident tracks and chunks of one continuous recording: the
    baseline fits, solves and decodes each of them (their stand-in data carry no planted lagged map: no accuracy is claimed)."""
    import ridge_baseline
    from speech_decoding_amd import load_config
    args = load_config(overrides=["dataset=Gwilliams2022", "num_subjects=2", "num_channels=6", "F=8", "preprocs.last4layers=False",
                                  "preprocs.seq_len_sec=0.5", "preprocs.baseline_len_sec=0.1", "batch_size=16",
                                  "synthetic_segments=80", "ridge.n_lags=4", "ridge.alphas=[0.1,10]", f"data={kind}"] + extra)
    lines = []
    row, ridge = ridge_baseline.run(args, log=lambda *parts: lines.append("".join(parts)))
    assert ridge.n > 0 and row["alpha"] in (0.1, 10.0) and np.isfinite(row["test_loss"]) and bool(torch.isfinite(ridge.coef_).all())
    assert 0.0 <= row["testTop1acc"] <= row["testTop10acc"] <= 1.0 and len(lines) == 1
