"""CPU checks of the time-lagged ridge baseline (speech_decoding_amd/ridge.py, csrc/lagged_cov.hip): the float64 reference of
tests/ridge_cases.py against the explicit zero-extended design matrix and sklearn's Ridge, planted recovery, that an fp32
emulation of the kernel stays inside the summation bound the GPU test applies and every planted bug misses it by 10x or more,
and the refusals of the C entry points and of the Python layer.  No kernel is launched here."""
import os

import numpy as np
import pytest
import torch

from tests import ridge_cases as RC

SMALL = dict(B=3, C=5, F=7, T=37, L=6)


@pytest.fixture(scope="module")
def lib():
    from speech_decoding_amd import lib as L
    if not os.path.exists(L.LIB_PATH):
        import __graft_entry__ as g
        g.build()
    return L


def _segments(seed=0, silent_head=False, B=3, C=5, F=7, T=37, L=6):
    rng = np.random.default_rng(seed)
    X = rng.standard_normal((B, C, T))
    if silent_head:
        X[:, :, :L - 1] = 0
    W = rng.standard_normal((L, C, F))
    return X, RC.predict(X, W, np.zeros(F)), W


@pytest.mark.parametrize("silent_head", [False, True])
def test_reference_assembly_is_the_design_matrix_gram(silent_head):
    X, Y, _ = _segments(0, silent_head)
    Y = Y + np.arange(1, 8)[None, :, None]                          # feature offsets: the centring term is exercised
    L = SMALL["L"]
    A, R, s, sum_y, n = RC.moments(X, Y, L)
    ybar = sum_y / n
    Phi, Yt = RC.design(X, L), RC.target(Y, L, ybar)
    assert Phi.shape == (3 * (37 + L - 1), L * 5)
    assert np.abs(RC.assemble(A) - Phi.T @ Phi).max() < 1e-12
    assert np.abs((R - s[:, :, None] * ybar[None, None, :]).reshape(L * 5, 7) - Phi.T @ Yt).max() < 1e-11
    # the lag-layout contraction the kernel runs is the same set of sums
    a, b = RC.lag_layout(X, L - 1), RC.lag_layout(Y, L - 1)
    assert np.abs(RC.lagged_cov(a, a, L)[:, :5, :5] - A).max() < 1e-12
    assert np.abs(RC.lagged_cov(a, b, L)[:, :5, :7] - R).max() < 1e-12


@pytest.mark.parametrize("alpha", [1e-9, 1.0, 100.0])
def test_reference_solution_is_sklearn_ridge(alpha):
    from sklearn.linear_model import Ridge
    X, Y, _ = _segments(1)
    Y = Y + 0.1 * np.random.default_rng(2).standard_normal(Y.shape) + np.arange(7)[None, :, None]
    L = SMALL["L"]
    W, ybar = RC.fit(X, Y, L, [alpha])
    sk = Ridge(alpha=alpha, fit_intercept=False, solver="cholesky").fit(RC.design(X, L), RC.target(Y, L, ybar)).coef_.T
    assert np.abs(W[0].reshape(L * 5, 7) - sk).max() < 1e-10 * max(1.0, np.abs(sk).max())


def test_silent_head_recovers_the_planted_map():
    """With the first L - 1 steps silent the zero-extended rows carry no feature, and with every segment present in both signs
    the mean of y is zero: the planted map is then the exact minimiser, and the fit finds it."""
    X, _, Wp = _segments(3, silent_head=True)
    X = np.concatenate([X, -X])
    Y = RC.predict(X, Wp, np.zeros(7))
    W, ybar = RC.fit(X, Y, SMALL["L"], [1e-9])
    assert np.abs(ybar).max() < 1e-12 and np.abs(W[0] - Wp).max() < 1e-8
    assert np.abs(RC.predict(X, W[0], ybar) - Y).max() < 1e-8


def test_reference_decodes_the_planted_world():
    X, Y, _ = RC.planted_world()
    W, ybar = RC.fit(X[:48], Y[:48], 6, RC.ALPHAS)
    for i in range(len(RC.ALPHAS)):
        top1, margin = RC.cosine_top1(RC.predict(X[48:], W[i], ybar), Y[48:])
        assert top1 == 1.0 and margin >= 0.47, (RC.ALPHAS[i], top1, margin)


def _real_case(B, C, F, T, L, seed):
    rng = np.random.RandomState(seed)
    X, Y = rng.randn(B, C, T).astype(np.float32), (rng.randn(B, F, T) + 3.0).astype(np.float32)
    return RC.lag_layout(X, L - 1, C), RC.lag_layout(Y, L - 1, F)


CPU_CASES = [(3, 5, 7, 37, 6), (2, 3, 4, 211, 9)]                   # one slice with a partial chunk; two slices, a lag group + 1


@pytest.mark.parametrize("B,C,F,T,L", CPU_CASES)
def test_fp32_emulation_stays_inside_the_bound_and_planted_bugs_do_not(B, C, F, T, L):
    a, b = _real_case(B, C, F, T, L, 10 * L + B)
    slabs = RC.slice_rule(a.shape[0], L, 64, 64)[0]
    assert slabs == (1 if T == 37 else 2)
    for p, q in ((a, a), (a, b)):
        ref, lim = RC.lagged_cov(p.astype(np.float64), q.astype(np.float64), L), RC.cov_bound(p, q, L, slabs)
        err = np.abs(RC.emulate(p, q, L) - ref)
        assert (err <= lim).all(), (err / lim).max()
    ref, lim = RC.lagged_cov(a.astype(np.float64), b.astype(np.float64), L), RC.cov_bound(a, b, L, slabs)
    refA, limA = RC.lagged_cov(a.astype(np.float64), a.astype(np.float64), L), RC.cov_bound(a, a, L, slabs)
    for mutant in RC.KERNEL_MUTANTS:
        if mutant == "group_tail_dropped" and L % RC.GROUP == 0:
            continue
        if mutant == "transposed_blocks":                           # only the Gram blocks are square
            miss = (np.abs(RC.emulate(a, a, L, mutant) - refA) / limA).max()
        else:
            miss = (np.abs(RC.emulate(a, b, L, mutant) - ref) / lim).max()
        assert np.nan_to_num(miss, nan=np.inf) >= 10, (mutant, miss)


def test_estimator_bugs_miss_the_accumulator_tolerance():
    """n and s_l are float64 sums: the GPU suite holds them to 1e-12 of sum |x| (and n exactly).  Counting the pad rows in n or
    leaving s_l without its head correction misses that by far more than 10x, and moves the coefficients."""
    X, Y, _ = _segments(5)
    Y = Y + np.arange(1, 8)[None, :, None]
    _, _, s, _, n = RC.moments(X, Y, 6)
    W, _ = RC.fit(X, Y, 6, [1.0])
    tol = 1e-12 * np.abs(X).sum()
    _, _, s_m, _, n_m = RC.moments(X, Y, 6, "s_without_head")
    assert n_m == n and np.abs(s_m[0] - s[0]).max() == 0 and np.abs(s_m[1:] - s[1:]).max() >= 10 * tol
    _, _, s_m, _, n_m = RC.moments(X, Y, 6, "pad_rows_in_n")
    assert np.array_equal(s_m, s) and n_m - n == 3 * 5 >= 10 * 1e-12 * n
    for mutant in RC.ESTIMATOR_MUTANTS:
        assert np.linalg.norm(RC.fit(X, Y, 6, [1.0], mutant)[0] - W) > 1e-3 * np.linalg.norm(W), mutant


def test_coefficient_bound_is_finite_and_small_in_the_planted_world():
    X, Y, _ = RC.planted_world()
    for alpha in RC.ALPHAS:
        W, _ = RC.fit(X[:48], Y[:48], 6, [alpha])
        lim = 4 * RC.coef_bound(X[:48], Y[:48], 6, alpha, 1, W[0])
        assert 0 < lim < 0.02 * np.linalg.norm(W[0]), (alpha, lim)   # gamma_m with m = 2017 rows is 1.2e-4: a worst-case bound


def test_slice_rule_is_the_librarys(lib):
    L = lib.load()
    for rows, lags, Ap, Bp in [(37, 1, 64, 64), (126, 6, 64, 64), (159, 17, 128, 64), (1080, 6, 64, 64), (1095, 9, 128, 64),
                               (107264, 60, 256, 256), (107264, 60, 256, 1024), (107264, 60, 256, 128), (5000, 3, 64, 192)]:
        n, length = RC.slice_rule(rows, lags, Ap, Bp)
        assert L.sda_lagged_cov_slices(rows, lags, Ap, Bp) == n
        assert L.sda_lagged_cov_scratch_floats(rows, lags, Ap, Bp) == n * lags * Ap * Bp
        assert length % RC.CHUNK == 0 and (n - 1) * length < rows <= n * length
    assert RC.slice_rule(1080, 6, 64, 64) == (5, 256)                # the GPU suite's several-slices case, last slice partial


def test_c_entry_points_refuse_bad_arguments_without_launch(lib):
    L = lib.load()
    assert L.sda_abi_version() == lib.ABI_VERSION == 4              # additions only: the ABI version stays
    p = 4096                                           # a non-null address that is never dereferenced: every call is refused
    ok = dict(a=p, ap=64, b=p, bp=128, rows=126, L=6, H=5, Ap=64, Bp=128, out=p)

    def call(**kw):
        v = dict(ok, **kw)
        return L.sda_lagged_cov_f32(v["a"], v["ap"], v["b"], v["bp"], v["rows"], v["L"], v["H"], v["Ap"], v["Bp"], v["out"], None)
    for name in ("a", "b", "out"):
        assert call(**{name: None}) == -1 and b"null" in L.sda_last_error()
    for name in ("rows", "L", "Ap", "Bp"):
        for bad in (0, -1):
            assert call(**{name: bad}) == -1 and b"positive" in L.sda_last_error()
            sizes = dict(ok, **{name: bad})
            assert L.sda_lagged_cov_slices(sizes["rows"], sizes["L"], sizes["Ap"], sizes["Bp"]) == -1
            assert L.sda_lagged_cov_scratch_floats(sizes["rows"], sizes["L"], sizes["Ap"], sizes["Bp"]) == -1
    for name in ("Ap", "Bp"):
        assert call(**{name: 96, name.lower(): 96}) == -1 and b"multiples of 64" in L.sda_last_error()
    assert call(ap=60) == -1 and b"pitch" in L.sda_last_error()
    assert call(bp=64) == -1 and b"pitch" in L.sda_last_error()
    assert call(H=4) == -1 and b"zero rows" in L.sda_last_error()
    assert call(ap=66) == -1 and b"aligned" in L.sda_last_error()
    assert call(a=p + 4) == -1 and b"aligned" in L.sda_last_error()
    assert call(rows=2 ** 61, ap=2 ** 40) == -1 and b"indexing" in L.sda_last_error()


def test_python_layer_refuses_host_tensors_and_bad_shapes(lib):
    from speech_decoding_amd import SdaError, ops
    from speech_decoding_amd.ridge import LaggedRidge
    x = torch.zeros(10, 64)
    with pytest.raises(SdaError, match="device"):
        ops.lagged_cov(x, x, 2, 1)
    with pytest.raises(SdaError, match="no CPU path"):
        LaggedRidge(5, 7, n_lags=6, device="cpu")
    with pytest.raises(ValueError, match="positive"):
        LaggedRidge(5, 0, n_lags=6)
