"""The NumPy mirror of sparse GP regression (tests/sgpr_ref.py) held to the dense definition, to the exact log marginal
likelihood and to its own evaluation in np.longdouble; and the Python-surface refusals that need no device."""
import numpy as np
import pytest

import ard_ref as R
import sgpr_ref as S

EPS = np.finfo(np.float64).eps


def _problem(N, d, m):
    X, y = R.problem(N, d, seed=100 + d)
    return X, y, S.inducing(X, m)


@pytest.mark.parametrize("method", ["vfe", "fitc"])
def test_against_the_dense_definition(method):
    """N = 300: the whitened value is log N(y | 0, Q_ff + Lambda) (minus the trace term for VFE) and the whitened
    prediction is the dense one.  The dense route solves with K_uu + j I and then with C = Q_ff + Lambda, whose smallest
    eigenvalue is >= s, so its relative error is bounded by cond(K_uu + j I) eps |Q_ff| / s <= cond eps N sigma^2 / s;
    the whitened route's own error is orders below that (test_against_longdouble)."""
    N, d, m, noise = S.CASES[0]
    X, y, Z = _problem(N, d, m)
    Xs = X[:40] + 0.05
    ref = S.fit(X, y, Z, S.SIGMA, S.ELL, noise, method=method, Xs=Xs)
    den = S.dense(X, y, Z, S.SIGMA, S.ELL, noise, method=method, Xs=Xs)
    rtol = ref["cond"] * EPS * N * S.SIGMA ** 2 / noise
    e_val = abs(ref["value"] - den["value"]) / ref["scale"]
    e_mu = np.max(np.abs(ref["mean"] - den["mean"])) / max(1.0, np.max(np.abs(y)))
    e_var = np.max(np.abs(ref["var"] - den["var"])) / S.SIGMA ** 2
    print("%s cond %.2e bound %.2e: value %.2e mean %.2e var %.2e" % (method, ref["cond"], rtol, e_val, e_mu, e_var))
    assert rtol < 1e-3                      # the bound itself must mean something
    assert e_val <= rtol and e_mu <= rtol and e_var <= rtol
    if method == "vfe":                     # the last term of the mirror IS the trace term
        assert abs(-ref["terms"][-1] - den["trace"]) <= rtol * max(1.0, den["trace"])
    assert np.all(ref["var"] > 0) and np.all(ref["var"] <= S.SIGMA ** 2 * (1 + 1e-12))


@pytest.mark.parametrize("N,d,m,noise", S.CASES)
def test_vfe_is_a_lower_bound_of_the_exact_lml(oracle, N, d, m, noise):
    X, y, Z = _problem(N, d, m)
    exact = oracle.compute_mar_likelihood(X, None, y, S.SIGMA, S.ELL, noise)
    vfe = S.fit(X, y, Z, S.SIGMA, S.ELL, noise, method="vfe")
    print("N=%d m=%d: bound %.6f exact %.6f" % (N, m, vfe["value"], float(exact)))
    assert vfe["value"] <= float(exact)


def test_vfe_with_every_point_inducing_reaches_the_exact_lml(oracle):
    """Z = X: Q_ff = K (K + j I)^-1 K differs from K by O(j), so the bound is tight to O(j / s) of its scale"""
    X, y = R.problem(130, 2, seed=102)
    exact = float(oracle.compute_mar_likelihood(X, None, y, S.SIGMA, S.ELL, 1e-2))
    vfe = S.fit(X, y, X, S.SIGMA, S.ELL, 1e-2, method="vfe")
    assert vfe["value"] <= exact
    assert exact - vfe["value"] <= 130 * S.JITTER / 1e-2 * vfe["scale"]


@pytest.mark.parametrize("method", ["vfe", "fitc"])
@pytest.mark.parametrize("N,d,m,noise", S.CASES + [S.MID])
def test_against_longdouble(N, d, m, noise, method):
    """every input of the GPU tests: float64 agrees with np.longdouble (hand-written Cholesky and substitution) to
    1e-11 of the sum of the absolute terms, ten times inside the GPU bar"""
    if np.finfo(np.longdouble).eps >= EPS:
        pytest.skip("np.longdouble is no wider than float64 on this platform")
    X, y, Z = _problem(N, d, m)
    f64 = S.fit(X, y, Z, S.SIGMA, S.ELL, noise, method=method)
    ld = S.fit(X, y, Z, S.SIGMA, S.ELL, noise, method=method, dtype=np.longdouble)
    err = abs(float(ld["value"] - np.longdouble(f64["value"]))) / f64["scale"]
    print("N=%d d=%d m=%d %s cond %.2e: |f64 - longdouble| / scale %.2e" % (N, d, m, method, f64["cond"], err))
    assert err <= 1e-11


def test_plain_factorisation_matches_lapack():
    rng = np.random.default_rng(5)
    M = rng.standard_normal((40, 40))
    A = M @ M.T + 40 * np.eye(40)
    L = S.chol_plain(A)
    assert np.allclose(L, np.linalg.cholesky(A), rtol=1e-13, atol=1e-13)
    Bm = rng.standard_normal((40, 7))
    assert np.allclose(L @ S.solve_lower_plain(L, Bm), Bm, rtol=1e-12, atol=1e-12)


def test_choose_inducing():
    from gaussian_process_amd import choose_inducing
    X, _ = R.problem(200, 3, seed=1)
    Z = choose_inducing(X, 50, seed=4)
    assert Z.shape == (50, 3) and Z.flags.c_contiguous
    rows = {tuple(r) for r in X}
    assert all(tuple(z) in rows for z in Z) and len({tuple(z) for z in Z}) == 50
    assert np.array_equal(Z, choose_inducing(X, 50, seed=4))
    assert not np.array_equal(Z, choose_inducing(X, 50, seed=5))
    for bad in (0, 201):
        with pytest.raises(ValueError):
            choose_inducing(X, bad)


def test_refusals_that_need_no_device():
    """an unknown method and m > N raise before any context exists"""
    from gaussian_process_amd import sparse_prediction
    from gaussian_process_amd.gp import sparse_args
    X, y = R.problem(30, 2, seed=2)
    with pytest.raises(ValueError, match="method must be one of"):
        sparse_prediction(X, X[:5], y, X[:10], 1.0, 1.0, 1e-2, method="dtc")
    with pytest.raises(ValueError, match="number of inducing inputs"):
        sparse_prediction(X, X[:5], y, np.vstack([X, X[:1]]), 1.0, 1.0, 1e-2)
    with pytest.raises(ValueError, match="d="):
        sparse_args(X, X[:10, :1], "vfe")
    assert sparse_args(X, X[:10], "fitc")[2] == 1 and sparse_args(X, X[:10], "vfe")[2] == 0
