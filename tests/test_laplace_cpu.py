"""The Laplace classifier's NumPy mirror (tests/laplace_ref.py) against scikit-learn's GaussianProcessClassifier
(tests/golden/laplace/*.npz, written by scripts/make_laplace_golden.py), its stationarity at the mode, the prediction's
quadrature against a dense reference, and the reference helpers of GP_binary_classification.py.  No GPU.

Tolerances against sklearn were measured on these fixtures (largest over the four): sklearn stops one Newton iterate
earlier (its test is lml - lml_prev < 1e-10) and keeps that iterate's W, so
  log q 2.4e-11 relative, f^ 1.1e-9 of max|f^|, pi(f^) 9.4e-11, latent mean 2.8e-9 of its max, latent variance
  7.3e-10 sigma^2 (all from blobs_N300_d1, the case with the largest last step), and the probability 2.9e-4, because
  sklearn's predict_proba uses an erf mixture for the integral.
The bounds below leave a factor of about ten over the measurement (the probability: 1e-3)."""
import glob
import os

import numpy as np
import pytest

import laplace_ref as R
from conftest import GOLDEN
from gaussian_process_amd import GP_binary_classification as G

CASES = sorted(glob.glob(os.path.join(GOLDEN, "laplace", "*.npz")))


def test_fixtures_are_present_and_apart_from_the_regression_cases():
    names = sorted(os.path.basename(f)[:-4] for f in CASES)
    assert names == ["blobs_N1024_d8", "blobs_N300_d1", "moons_N2000_d2", "moons_N50_d2"]
    assert not glob.glob(os.path.join(GOLDEN, "*laplace*.npz"))


@pytest.mark.parametrize("path", CASES, ids=lambda p: os.path.basename(p)[:-4])
def test_mirror_matches_sklearn(path):
    g = np.load(path)
    sigma, l = float(g["sigma"]), float(g["l"])
    fit = R.laplace_fit(g["X"], g["y"], sigma, l)
    assert fit["converged"] and 1 <= fit["iters"] <= 20
    lml = float(g["log_marginal_likelihood"])
    assert abs(fit["log_q"] - lml) <= 2e-10 * abs(lml)
    f_ref = g["f_cached"]
    assert np.max(np.abs(fit["f"] - f_ref)) <= 1e-8 * np.max(np.abs(f_ref))
    assert np.max(np.abs(R.expit(fit["f"]) - g["pi"])) <= 1e-9
    assert np.max(np.abs(fit["s"] - g["W_sr"])) <= 1e-9
    f_mean, f_var, prob, label = R.laplace_predict(fit, g["X"], g["Xs"], sigma, l)
    assert np.max(np.abs(f_mean - g["f_mean"])) <= 3e-8 * np.max(np.abs(g["f_mean"]))
    assert np.max(np.abs(f_var - g["f_var"])) <= 1e-8 * sigma ** 2
    assert np.max(np.abs(prob - g["prob"])) <= 1e-3
    np.testing.assert_array_equal(G.label_function(f_mean), label)
    np.testing.assert_array_equal(label[np.abs(g["prob"] - .5) > 1e-3],
                                  np.where(g["prob"] >= .5, 1, -1)[np.abs(g["prob"] - .5) > 1e-3])


@pytest.mark.parametrize("path", CASES, ids=lambda p: os.path.basename(p)[:-4])
def test_mode_is_stationary(path):
    """At the mode f^ = K grad log p(y|f^) (GPML eq. 3.17)."""
    g = np.load(path)
    fit = R.laplace_fit(g["X"], g["y"], float(g["sigma"]), float(g["l"]))
    f = fit["f"]
    assert np.max(np.abs(f - fit["K"] @ fit["grad"])) <= 1e-8 * np.max(np.abs(f))


def test_halving_and_iteration_cap():
    """max_iter caps the Newton steps and reports no convergence; the halving rule keeps Psi from dropping."""
    g = np.load(CASES[-1])
    fit = R.laplace_fit(g["X"], g["y"], float(g["sigma"]), float(g["l"]), max_iter=1)
    assert fit["iters"] == 1 and not fit["converged"]
    fit0 = R.laplace_fit(g["X"], g["y"], float(g["sigma"]), float(g["l"]), max_iter=0)
    assert fit0["iters"] == 0 and np.all(fit0["f"] == 0) and fit0["log_q"] < fit["log_q"]


@pytest.mark.parametrize("sig2", [1e-4, 0.25, 1.0, 2.25, 9.0, 25.0, 400.0])
def test_quadrature_error_below_1e12(sig2):
    """The trapezoid rule against a 4e5-point rule over [-12, 12] for every V <= sigma^2 (here V from 0 to sigma^2)."""
    mu = np.array([-30.0, -6.0, -2.0, -0.3, 0.0, 0.4, 1.5, 5.0, 30.0])
    for frac in (0.0, 1e-6, 0.1, 0.5, 1.0):
        var = np.full(mu.shape, frac * sig2)
        got = R.expit_gauss(mu, var, sig2)
        h = 24.0 / 400000
        t = -12.0 + h * np.arange(400001)
        w = h * np.exp(-0.5 * t * t) / np.sqrt(2 * np.pi)
        w[0] *= .5
        w[-1] *= .5
        z = mu[:, None] + np.sqrt(var)[:, None] * t[None, :]
        ref = np.array([np.dot(R.expit(row), w) for row in z])
        assert np.max(np.abs(got - ref)) < 1e-12, (sig2, frac, np.max(np.abs(got - ref)))


def test_quadrature_node_count():
    t1, _ = R.quad_nodes(1.0)
    t2, _ = R.quad_nodes(100.0)
    assert len(t1) <= 100 and len(t2) > len(t1) and len(t2) < 2000


def test_reference_helpers():
    f = np.array([-800.0, -3.0, 0.0, 2.0, 800.0])
    from scipy.special import expit
    np.testing.assert_allclose(G.pi_function(f), expit(f), rtol=1e-15, atol=1e-300)
    assert G.label_function(0.0) == 1 and G.label_function(-1e-300) == -1
    np.testing.assert_array_equal(G.label_function(f), [-1, -1, 1, 1, 1])
    z = np.array([-3.0, 0.0, 4.0])
    np.testing.assert_allclose(G.log_likelihood(z), -np.log(1 + np.exp(-z)), rtol=1e-13)
    assert G.log_likelihood(-800.0) == -800.0
    y = np.array([1.0, -1.0, 1.0])
    np.testing.assert_allclose(G.deriv_log_likelihood(y, z), (y + 1) / 2 - 1 / (1 + np.exp(-y * z)), rtol=1e-15)
    p = 1 / (1 + np.exp(-z))
    np.testing.assert_allclose(G.sec_deriv_log_likelihood(z), -p * (1 - p), rtol=1e-15)
