"""The softmax classifier's NumPy mirror (tests/softmax_ref.py) against three anchors that share no code with it -- the
dense log-determinant over all C N latent values, the stationarity of the mode, and the binary classifier's mirror and
scikit-learn fixtures through the identity "C = 2 is the binary classifier with kernel 2 K" -- and the helpers and label
checks of GP_multi_classification.py.  No GPU.

Measured with this file (largest over its cases): log q against the dense determinant 3.7e-16 relative; stationarity
5.1e-12 of max|F| at N <= 300 and 3.8e-10 at N = 1000; sum_c F 4.7e-14 of max|F|; smallest eigenvalue of a Sigma 0.13;
C = 2 against the binary mirror: log q 2.7e-15, F_0 - F_1 1.4e-13, mu_0 - mu_1 2.0e-11, variance 2.3e-14 of 2 sigma^2."""
import glob
import os

import numpy as np
import pytest

import laplace_ref as RB
import softmax_ref as R
from conftest import GOLDEN
from gaussian_process_amd import GP_multi_classification as G
from gaussian_process_amd import _lib

CASES = [(60, 2, 3, 1.0, 1.0), (300, 2, 3, 2.0, 0.8), (257, 8, 5, 1.5, 3.0)]
IDS = ["N%d_C%d" % (c[0], c[2]) for c in CASES]
SKLEARN = sorted(glob.glob(os.path.join(GOLDEN, "laplace", "*.npz")))

_fits = {}


def fitted(case):
    if case not in _fits:
        N, d, C, sigma, l = case
        X, lab, Xs = R.blobs(N, d, C, N)
        _fits[case] = (X, lab, Xs, R.fit(X, lab, C, sigma, l))
    return _fits[case]


def binary_problem(N, d, seed, n=300):
    """the problems of tests/test_laplace_gpu.py: two Gaussian blobs with overlapping tails, labels +-1"""
    rng = np.random.default_rng(seed)
    y = np.where(rng.random(N + n) < 0.5, -1.0, 1.0)
    X = rng.standard_normal((N + n, d)) * 1.5 + y[:, None] * (1.0 / np.sqrt(d))
    return X[:N], y[:N], X[N:]


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_log_q_matches_the_dense_determinant(case):
    """log q = Psi - 1/2 log|I + K_blk W| with W = diag(pi) - Pi Pi^T built densely (C N <= 1500)"""
    N, d, C, sigma, l = case
    ft = fitted(case)[3]
    assert ft["converged"] and 1 <= ft["iters"] <= 30
    P = ft["P"]
    Pi = np.vstack([np.diag(P[c]) for c in range(C)])
    W = np.diag(P.ravel()) - Pi @ Pi.T
    sign, logdet = np.linalg.slogdet(np.eye(C * N) + np.kron(np.eye(C), ft["K"]) @ W)
    dense = ft["psi"] - 0.5 * logdet
    assert sign == 1.0
    print("log q vs dense:", abs(ft["log_q"] - dense) / abs(dense))
    assert abs(ft["log_q"] - dense) <= 1e-12 * abs(dense)


@pytest.mark.parametrize("case", CASES + [(1000, 2, 4, 3.0, 0.7)], ids=IDS + ["N1000_C4"])
def test_mode_is_stationary_and_sums_to_zero(case):
    """At the mode F = (Y - P) K; the latent values of a point sum to 0 over the classes (the prior is shared)."""
    ft = fitted(case)[3]
    F = ft["F"]
    assert ft["converged"]
    stat = np.max(np.abs(F - ft["G"] @ ft["K"])) / np.max(np.abs(F))
    sumf = np.max(np.abs(F.sum(axis=0))) / np.max(np.abs(F))
    print("stationarity %.2e  sum_c F %.2e" % (stat, sumf))
    assert stat <= 1e-8
    assert sumf <= 1e-12


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_latent_covariance_is_positive_definite(case):
    N, d, C, sigma, l = case
    X, lab, Xs, ft = fitted(case)
    mu, Sig = R.predict(ft, X, Xs, sigma, l)
    assert np.array_equal(Sig, np.swapaxes(Sig, 1, 2))
    mineig = min(np.linalg.eigvalsh(s).min() for s in Sig)
    print("smallest eigenvalue", mineig)
    assert mineig > 0


def two_class_gaps(X, y, Xs, sigma_b, l):
    """softmax mirror with C = 2 and sigma_b / sqrt(2) against quantities of the binary problem with sigma_b"""
    lab = np.where(y > 0, 0, 1)
    sigma = sigma_b / np.sqrt(2)
    ft = R.fit(X, lab, 2, sigma, l)
    mu, Sig = R.predict(ft, X, Xs, sigma, l)
    return ft, ft["F"][0] - ft["F"][1], mu[:, 0] - mu[:, 1], Sig[:, 0, 0] + Sig[:, 1, 1] - 2 * Sig[:, 0, 1], mu, Sig


@pytest.mark.parametrize("N,d,sigma,l", [(300, 1, 2.0, 1.0), (1024, 8, 1.5, 3.0)], ids=["N300", "N1024"])
def test_two_classes_are_the_binary_classifier_with_kernel_2K(N, d, sigma, l):
    """f = F_0 - F_1 has the prior 2 K and the likelihood expit(+-f): softmax_ref.fit(X, labels, 2, sigma, l) is
    laplace_ref.laplace_fit(X, y, sigma sqrt(2), l) with label 0 <-> y = +1"""
    X, y, Xs = binary_problem(N, d, N)
    sb = sigma * np.sqrt(2)
    ft, f, m, v, _, _ = two_class_gaps(X, y, Xs, sb, l)
    b = RB.laplace_fit(X, y, sb, l)
    bm, bv, bp, _ = RB.laplace_predict(b, X, Xs, sb, l)
    gaps = (abs(ft["log_q"] - b["log_q"]) / abs(b["log_q"]), np.max(np.abs(f - b["f"])) / np.max(np.abs(b["f"])),
            np.max(np.abs(m - bm)) / np.max(np.abs(bm)), np.max(np.abs(v - bv)) / (2 * sigma ** 2))
    print("log q %.1e  f %.1e  mean %.1e  var %.1e" % gaps)
    assert ft["converged"] and b["converged"]
    assert gaps[0] <= 1e-12
    assert gaps[1] <= 1e-10
    assert gaps[2] <= 1e-9
    assert gaps[3] <= 1e-11


@pytest.mark.parametrize("path", SKLEARN, ids=lambda p: os.path.basename(p)[:-4])
def test_two_classes_match_sklearn(path):
    """the scikit-learn fixtures of the binary classifier through the same identity, held to the bounds
    tests/test_laplace_cpu.py uses for them"""
    g = np.load(path)
    sb, l = float(g["sigma"]), float(g["l"])
    ft, f, m, v, _, _ = two_class_gaps(g["X"], g["y"], g["Xs"], sb, l)
    assert ft["converged"]
    lml = float(g["log_marginal_likelihood"])
    assert abs(ft["log_q"] - lml) <= 2e-10 * abs(lml)
    assert np.max(np.abs(f - g["f_cached"])) <= 1e-8 * np.max(np.abs(g["f_cached"]))
    assert np.max(np.abs(m - g["f_mean"])) <= 3e-8 * np.max(np.abs(g["f_mean"]))
    assert np.max(np.abs(v - g["f_var"])) <= 1e-8 * sb ** 2


def test_probabilities():
    """Rows sum to 1; normals = 0 gives softmax(mu*); and for C = 2 with S = 20000 seeded draws the first column is the
    binary mirror's quadrature int expit(z) N(z | f_mean, f_var) dz within 4 / sqrt(S) = 0.028 (a [0, 1] variable has a
    standard error of at most 0.5 / sqrt(S): 8 standard errors).  Measured gap with these seeds: 3.3e-3."""
    case = CASES[2]
    N, d, C, sigma, l = case
    X, lab, Xs, ft = fitted(case)
    mu, Sig = R.predict(ft, X, Xs, sigma, l)
    z = np.random.default_rng(5).standard_normal((1000, C))
    p = R.proba(mu, Sig, z)
    assert np.max(np.abs(p.sum(axis=1) - 1)) <= 1e-14 and np.all(p > 0)
    np.testing.assert_allclose(R.proba(mu, Sig, np.zeros((3, C))), G.softmax(mu.T).T, rtol=1e-14)

    S = 20000
    Xb, y, Xbs = binary_problem(300, 1, 300)
    sb = 2.0 * np.sqrt(2)
    ft2, f, m, v, mu2, Sig2 = two_class_gaps(Xb, y, Xbs, sb, 1.0)
    p2 = R.proba(mu2, Sig2, np.random.default_rng(11).standard_normal((S, 2)))
    quad = RB.expit_gauss(m, v, sb ** 2)
    gap = np.max(np.abs(p2[:, 0] - quad))
    print("Monte-Carlo gap", gap)
    assert gap <= 4 / np.sqrt(S)


def test_clamped_cholesky():
    """a semi-definite Sigma is legitimate: its zero pivot and that column become 0, the rest is the usual factor"""
    a = np.array([[4.0, 2.0, 2.0], [2.0, 1.0, 1.0], [2.0, 1.0, 5.0]])
    L = R.chol_clamped(a)
    np.testing.assert_array_equal(L[:, 1], 0.0)
    np.testing.assert_allclose(L @ L.T, a, atol=1e-15)
    spd = np.array([[2.0, 0.5], [0.5, 1.0]])
    np.testing.assert_allclose(R.chol_clamped(spd), np.linalg.cholesky(spd), rtol=1e-15)


def test_reference_helpers():
    f = np.array([[-800.0, 3.0, 800.0, 0.0], [800.0, 1.0, 800.0, 0.0], [0.0, -2.0, -800.0, 0.0]])
    P = G.softmax(f)
    assert np.all(np.isfinite(P)) and np.max(np.abs(P.sum(axis=0) - 1)) <= 1e-15
    np.testing.assert_allclose(P[:, 1], np.exp(f[:, 1]) / np.exp(f[:, 1]).sum(), rtol=1e-15)
    np.testing.assert_array_equal(P[:, 0], [0.0, 1.0, 0.0])
    np.testing.assert_array_equal(P[:, 2], [0.5, 0.5, 0.0])
    np.testing.assert_allclose(G.softmax(f[:, 1]), P[:, 1], rtol=1e-15)
    C, n = f.shape
    pv, pm = G.compute_pi(f.ravel(), C, n)
    assert pv.shape == (C * n,) and pm.shape == (C * n, n)
    for c in range(C):
        for i in range(n):
            assert pv[c * n + i] == P[c, i]
            assert pm[i * C + c, i] == P[c, i]
    assert np.count_nonzero(pm) <= C * n and pm.sum() == pytest.approx(n)


@pytest.mark.parametrize("bad", [-1, 3, 1.5, np.nan])
def test_bad_labels_refused_on_the_host(bad):
    """before any device call: without a GPU a context cannot even be created"""
    X = np.zeros((6, 2))
    lab = np.array([0, 1, 2, 0, 1, bad], dtype=np.float64)
    with pytest.raises(ValueError):
        G.laplace_fit(X, lab, n_classes=3)


@pytest.mark.parametrize("n_classes", [0, 1, _lib.SOFTMAX_MAX_CLASSES + 1, 2.5])
def test_bad_class_counts_refused_on_the_host(n_classes):
    with pytest.raises(ValueError):
        G.laplace_fit(np.zeros((4, 2)), [0, 1, 0, 1], n_classes=n_classes)
    with pytest.raises(ValueError):
        G.laplace_fit(np.zeros((4, 2)), [0, 0, 0, 0])               # one class: n_classes defaults to 1


def test_class_limit_matches_the_header():
    from conftest import ROOT
    src = open(os.path.join(ROOT, "include", "gpmi.h")).read()
    assert "#define GPMI_SOFTMAX_MAX_CLASSES %d\n" % _lib.SOFTMAX_MAX_CLASSES in src
    assert _lib.SOFTMAX_MAX_CLASSES >= 10 and _lib.ABI_VERSION == 4
