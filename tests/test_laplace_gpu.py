"""Binary GP classification on the MI355X (gpmi_laplace_fit / gpmi_laplace_predict_resident) against the NumPy mirror
of tests/laplace_ref.py and the scikit-learn fixtures of tests/golden/laplace, its bitwise reproducibility, and the
separation of the Laplace state from the regression state."""
import glob
import os
import warnings

import numpy as np
import pytest

import laplace_ref as R
from conftest import GOLDEN

pytestmark = pytest.mark.gpu

FIXTURES = sorted(glob.glob(os.path.join(GOLDEN, "laplace", "*.npz")))


def problem(N, d, seed, n=300):
    """two Gaussian blobs with overlapping tails, labels +-1"""
    rng = np.random.default_rng(seed)
    y = np.where(rng.random(N + n) < 0.5, -1.0, 1.0)
    X = rng.standard_normal((N + n, d)) * 1.5 + y[:, None] * (1.0 / np.sqrt(d))
    return X[:N], y[:N], X[N:]


SIZES = [(50, 2, 1.0, 0.7), (300, 1, 2.0, 1.0), (1024, 8, 1.5, 3.0), (2000, 2, 3.0, 0.8), (4096, 8, 1.0, 2.5),
         (8192, 8, 2.0, 3.0)]


@pytest.mark.parametrize("N,d,sigma,l", SIZES, ids=["N%d" % s[0] for s in SIZES])
def test_gpu_matches_mirror(ctx, N, d, sigma, l):
    X, y, Xs = problem(N, d, N)
    log_q, f_hat, iters, conv = ctx.laplace_fit(X, y, sigma, l)
    ref = R.laplace_fit(X, y, sigma, l)
    assert conv and ref["converged"]
    assert abs(iters - ref["iters"]) <= 1
    assert np.max(np.abs(f_hat - ref["f"])) <= 1e-9 * np.max(np.abs(ref["f"]))
    assert abs(log_q - ref["log_q"]) <= 1e-11 * abs(ref["log_q"])
    f_mean, f_var, prob = ctx.laplace_predict(Xs)
    m, v, p, lab = R.laplace_predict(ref, X, Xs, sigma, l)
    assert np.max(np.abs(f_mean - m)) <= 1e-9 * np.max(np.abs(m))
    assert np.max(np.abs(f_var - v)) <= 1e-10 * sigma ** 2
    assert np.max(np.abs(prob - p)) <= 1e-10
    from gaussian_process_amd import GP_binary_classification as G
    np.testing.assert_array_equal(G.predict_label(Xs, ctx=ctx), lab)


@pytest.mark.parametrize("path", FIXTURES, ids=lambda p: os.path.basename(p)[:-4])
def test_gpu_matches_sklearn(ctx, path):
    """the bounds of tests/test_laplace_cpu.py (measured there for the mirror)"""
    g = np.load(path)
    sigma, l = float(g["sigma"]), float(g["l"])
    from gaussian_process_amd import GP_binary_classification as G
    log_q, f_hat, iters, conv = G.laplace_fit(g["X"], g["y"], sigma, l, ctx=ctx)
    assert conv
    lml = float(g["log_marginal_likelihood"])
    assert abs(log_q - lml) <= 2e-10 * abs(lml)
    assert np.max(np.abs(f_hat - g["f_cached"])) <= 1e-8 * np.max(np.abs(g["f_cached"]))
    f_mean, f_var, prob = G.predict_latent(g["Xs"], ctx=ctx)
    assert np.max(np.abs(f_mean - g["f_mean"])) <= 3e-8 * np.max(np.abs(g["f_mean"]))
    assert np.max(np.abs(f_var - g["f_var"])) <= 1e-8 * sigma ** 2
    assert np.max(np.abs(prob - g["prob"])) <= 1e-3
    np.testing.assert_array_equal(G.predict_proba(g["Xs"], ctx=ctx), prob)


def test_two_fits_same_bits(ctx):
    X, y, Xs = problem(2000, 8, 7)
    a = ctx.laplace_fit(X, y, 1.5, 2.0)
    pa = ctx.laplace_predict(Xs)
    b = ctx.laplace_fit(X, y, 1.5, 2.0)
    pb = ctx.laplace_predict(Xs)
    assert a[0] == b[0] and a[2] == b[2]
    assert np.array_equal(a[1], b[1])
    for u, v in zip(pa, pb):
        assert np.array_equal(u, v)


def test_iteration_cap_warns(ctx):
    X, y, _ = problem(300, 2, 3)
    with pytest.warns(RuntimeWarning):
        log_q, f_hat, iters, conv = ctx.laplace_fit(X, y, 2.0, 1.0, max_iter=1)
    assert iters == 1 and not conv
    ref = R.laplace_fit(X, y, 2.0, 1.0, max_iter=1)
    assert np.max(np.abs(f_hat - ref["f"])) <= 1e-9 * np.max(np.abs(ref["f"]))
    assert abs(log_q - ref["log_q"]) <= 1e-11 * abs(ref["log_q"])


def test_bad_labels_and_kinds_refused(ctx):
    X, y, _ = problem(300, 2, 4)
    with pytest.raises(ValueError):
        ctx.laplace_fit(X, (y + 1) / 2, 1.0, 1.0)          # {0, 1}
    with pytest.raises(ValueError):
        ctx.laplace_fit(X, y * 1.0000001, 1.0, 1.0)
    try:
        for kind, p0, p1 in (("lin", 0.5, 0.0), ("per", 2.0, 1.0)):
            ctx.set_kernel(kind, p0, p1)
            with pytest.raises(ValueError):
                ctx.laplace_fit(X[:, :1], y, 1.0, 1.0)
        ctx.set_kernel("co2", np.ones(11))
        with pytest.raises(ValueError):
            ctx.laplace_fit(X, y, 1.0, 1.0)
    finally:
        ctx.set_kernel("rbf")


def test_states_do_not_mix(ctx):
    X, y, Xs = problem(1024, 4, 5)
    ctx.fit(X, y, 1.0, 1.5, 1e-3)                           # regression fit -> no Laplace state
    with pytest.raises(ValueError):
        ctx.laplace_predict(Xs)
    ctx.laplace_fit(X, y, 1.0, 1.5)                         # Laplace fit -> no regression factor
    with pytest.raises(ValueError):
        ctx.predict(Xs)
    with pytest.raises(ValueError):
        ctx.alpha()
    with pytest.raises(ValueError):
        ctx.lml_grad()
    ctx.set_test(Xs)
    with pytest.raises(ValueError):
        ctx.post_chol(1e-6)
    with pytest.raises(ValueError):
        ctx.post_sample(1e-6, np.ones((Xs.shape[0], 2)))
    ctx.laplace_predict(Xs)                                 # still resident after the refusals


def test_regression_after_laplace_same_bits(ctx):
    X, y, Xs = problem(2000, 8, 6)
    yr = y + 0.1 * np.sin(X[:, 0])
    lml0 = ctx.fit(X, yr, 1.2, 2.0, 1e-3)
    mu0, var0 = ctx.predict(Xs, want_sd=False)
    al0 = ctx.alpha()
    ctx.laplace_fit(X, y, 1.2, 2.0)
    ctx.laplace_predict(Xs)
    lml1 = ctx.fit(X, yr, 1.2, 2.0, 1e-3)
    mu1, var1 = ctx.predict(Xs, want_sd=False)
    al1 = ctx.alpha()
    assert lml0 == lml1
    assert np.array_equal(mu0, mu1) and np.array_equal(var0, var1) and np.array_equal(al0, al1)
