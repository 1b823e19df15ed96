"""Edges of both classifiers on the MI355X that the end-to-end tests do not reach: test sets of one point, on either
side of the 128-row tile, larger than a tile and as large as the training set; the largest C * np_ sweep; one draw, and
draw counts on either side of and far beyond the 256 threads of softmax_sample_kernel; a kernel matrix of zeros, where
every pivot of the C x C Cholesky clamps; max_iter = 0 and tol = 0; and a small fit after a large one on the same
context, held bit for bit to a fresh context.  Mirrors: tests/laplace_ref.py, tests/softmax_ref.py; bounds: those of
tests/test_laplace_gpu.py and tests/test_softmax_gpu.py."""
import functools

import numpy as np
import pytest

import laplace_ref as LR
import softmax_ref as SR

pytestmark = pytest.mark.gpu

N, D, SIGMA, ELL = 257, 8, 1.5, 3.0              # Np = 384, the last tile holds one real row
SIZES = [1, 127, 128, 129, 300, N]               # N: as many test points as training points, other points


def binary_problem(n_train, d, seed, n=300):
    """the problems of tests/test_laplace_gpu.py"""
    rng = np.random.default_rng(seed)
    y = np.where(rng.random(n_train + n) < 0.5, -1.0, 1.0)
    X = rng.standard_normal((n_train + n, d)) * 1.5 + y[:, None] * (1.0 / np.sqrt(d))
    return X[:n_train], y[:n_train], X[n_train:]


@functools.lru_cache(maxsize=None)
def binary_case():
    X, y, Xs = binary_problem(N, D, N)
    return X, y, Xs, LR.laplace_fit(X, y, SIGMA, ELL)


@functools.lru_cache(maxsize=None)
def softmax_case(C):
    X, lab, Xs = SR.blobs(N, D, C, N + C, n=300)
    return X, lab, Xs, SR.fit(X, lab, C, SIGMA, ELL)


def hold_binary_prediction(got, want, sigma=SIGMA):
    f_mean, f_var, prob = got
    m, v, p = want[:3]
    assert f_mean.shape == m.shape and f_var.shape == v.shape and prob.shape == p.shape
    assert np.max(np.abs(f_mean - m)) <= 1e-9 * np.max(np.abs(m))
    assert np.max(np.abs(f_var - v)) <= 1e-10 * sigma ** 2
    assert np.max(np.abs(prob - p)) <= 1e-10


def hold_softmax_prediction(got, m, S, p, sigma=SIGMA):
    mu, cov, prob = got
    assert mu.shape == m.shape and cov.shape == S.shape and prob.shape == p.shape
    assert np.max(np.abs(mu - m)) <= 1e-9 * np.max(np.abs(m))
    assert np.max(np.abs(cov - S)) <= 1e-10 * sigma ** 2
    assert np.max(np.abs(prob - p)) <= 1e-10


# ---- test-set sizes ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", SIZES)
def test_binary_test_set_sizes(ctx, n):
    X, y, Xs, ref = binary_case()
    ctx.laplace_fit(X, y, SIGMA, ELL)
    got = ctx.laplace_predict(Xs[:n])
    hold_binary_prediction(got, LR.laplace_predict(ref, X, Xs[:n], SIGMA, ELL))


@pytest.mark.parametrize("n,C", [(n, 5) for n in SIZES] + [(129, 10)], ids=lambda v: str(v))
def test_softmax_test_set_sizes(ctx, n, C):
    """C = 10, n = 129: the largest sweep, C * np_ = 2560 rows"""
    X, lab, Xs, ref = softmax_case(C)
    z = np.random.default_rng(n).standard_normal((200, C))
    ctx.softmax_fit(X, lab, C, SIGMA, ELL)
    got = ctx.softmax_predict(Xs[:n], z)
    m, S = SR.predict(ref, X, Xs[:n], SIGMA, ELL)
    hold_softmax_prediction(got, m, S, SR.proba(m, S, z))


# ---- draw counts -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("S", [1, 255, 256, 257, 1000])
def test_softmax_draw_counts(ctx, S):
    C = 5
    X, lab, Xs, ref = softmax_case(C)
    z = np.random.default_rng(S).standard_normal((S, C))
    ctx.softmax_fit(X, lab, C, SIGMA, ELL)
    mu, cov, prob = ctx.softmax_predict(Xs[:50], z)
    m, Sg = SR.predict(ref, X, Xs[:50], SIGMA, ELL)
    assert np.max(np.abs(prob - SR.proba(m, Sg, z))) <= 1e-10
    assert np.max(np.abs(prob.sum(axis=1) - 1.0)) <= 1e-12


# ---- K = 0: every pivot of the C x C Cholesky clamps ----------------------------------------------------------------------
@pytest.mark.parametrize("C,S", [(3, 1), (4, 1000), (3, 257)], ids=["C3_S1", "C4_S1000", "C3_S257"])
def test_softmax_zero_covariance(ctx, C, S):
    """sigma = 0: K = 0, so F = 0, log q = N log(1 / C), mu* = 0 and Sigma = 0 exactly; chol(Sigma) clamps every pivot to
    L = 0 and every draw gives softmax(0) = 1 / C.  The mean over the draws is exact where the partial sums k / C are
    representable -- one draw, or C = 4 -- and within S roundings of the sum otherwise (C = 3 with 257 draws).  The
    Newton step moves A but not F = A K, so Psi repeats and the fit stops after one step, as the mirror does."""
    X, lab, Xs = SR.blobs(N, D, C, 11)
    z = np.random.default_rng(S).standard_normal((S, C))
    log_q, F, iters, conv = ctx.softmax_fit(X, lab, C, 0.0, ELL)
    mu, cov, prob = ctx.softmax_predict(Xs, z)
    ref = SR.fit(X, lab, C, 0.0, ELL)
    m, Sg = SR.predict(ref, X, Xs, 0.0, ELL)
    assert not ref["F"].any() and not m.any() and not Sg.any()
    assert conv and ref["converged"] and iters == ref["iters"] == 1
    assert F.shape == (C, N) and not F.any()
    assert abs(log_q - N * np.log(1.0 / C)) <= 1e-13 * N * np.log(C)
    assert abs(ref["log_q"] - N * np.log(1.0 / C)) <= 1e-13 * N * np.log(C)
    assert not mu.any() and not cov.any()
    p = SR.proba(m, Sg, z)
    if S == 1 or C == 4:
        assert np.all(prob == 1.0 / C) and np.all(p == 1.0 / C)
    else:
        assert np.max(np.abs(prob - 1.0 / C)) <= S * 2.0 ** -53 and np.max(np.abs(p - 1.0 / C)) <= S * 2.0 ** -53


# ---- max_iter = 0, tol = 0 ---------------------------------------------------------------------------------------------
def test_binary_no_newton_step(ctx):
    X, y, Xs, _ = binary_case()
    with pytest.warns(RuntimeWarning):
        log_q, f_hat, iters, conv = ctx.laplace_fit(X, y, SIGMA, ELL, max_iter=0)
    got = ctx.laplace_predict(Xs)
    ref = LR.laplace_fit(X, y, SIGMA, ELL, max_iter=0)
    assert iters == 0 and not conv and ref["iters"] == 0 and not ref["converged"]
    assert f_hat.shape == (N,) and not f_hat.any()
    assert abs(log_q - ref["log_q"]) <= 1e-11 * abs(ref["log_q"])
    hold_binary_prediction(got, LR.laplace_predict(ref, X, Xs, SIGMA, ELL))


def test_softmax_no_newton_step(ctx):
    C = 5
    X, lab, Xs, _ = softmax_case(C)
    z = np.random.default_rng(0).standard_normal((200, C))
    with pytest.warns(RuntimeWarning):
        log_q, F, iters, conv = ctx.softmax_fit(X, lab, C, SIGMA, ELL, max_iter=0)
    got = ctx.softmax_predict(Xs, z)
    ref = SR.fit(X, lab, C, SIGMA, ELL, max_iter=0)
    assert iters == 0 and not conv and ref["iters"] == 0 and not ref["converged"]
    assert F.shape == (C, N) and not F.any()
    assert abs(log_q - ref["log_q"]) <= 1e-11 * abs(ref["log_q"])
    m, S = SR.predict(ref, X, Xs, SIGMA, ELL)
    hold_softmax_prediction(got, m, S, SR.proba(m, S, z))


def test_binary_zero_tolerance_runs_to_the_cap(ctx):
    """tol = 0 stops on Psi repeating exactly and halves on any fall, so the problem must still be climbing at the cap:
    problem(257, 2, 257) with sigma = 3, l = 0.8 gains 2.9e-7 in its fifth step (Psi = -123, one rounding 1.4e-14)"""
    X, y, _ = binary_problem(N, 2, N)
    with pytest.warns(RuntimeWarning):
        log_q, f_hat, iters, conv = ctx.laplace_fit(X, y, 3.0, 0.8, tol=0.0, max_iter=5)
    ref = LR.laplace_fit(X, y, 3.0, 0.8, tol=0.0, max_iter=5)
    assert all(d > 1e-7 for dec in ref["decisions"] for d, _ in dec)
    assert iters == 5 and not conv and ref["iters"] == 5 and not ref["converged"]
    assert np.max(np.abs(f_hat - ref["f"])) <= 1e-9 * np.max(np.abs(ref["f"]))


def test_softmax_zero_tolerance_runs_to_the_cap(ctx):
    """blobs(257, 2, 3, 257) with sigma = 3, l = 0.8 gains 2.3e-3 in its fifth step (see the binary test)"""
    X, lab, _ = SR.blobs(N, 2, 3, N)
    with pytest.warns(RuntimeWarning):
        log_q, F, iters, conv = ctx.softmax_fit(X, lab, 3, 3.0, 0.8, tol=0.0, max_iter=5)
    ref = SR.fit(X, lab, 3, 3.0, 0.8, tol=0.0, max_iter=5)
    assert all(d > 1e-7 for dec in ref["decisions"] for d, _ in dec)
    assert iters == 5 and not conv and ref["iters"] == 5 and not ref["converged"]
    assert np.max(np.abs(F - ref["F"])) <= 1e-9 * np.max(np.abs(ref["F"]))


# ---- stale device state --------------------------------------------------------------------------------------------------
def small_softmax_calls(c):
    X, lab, Xs = SR.blobs(129, D, 3, 5, n=300)
    z = np.random.default_rng(5).standard_normal((100, 3))
    return [c.softmax_fit(X, lab, 3, SIGMA, ELL), c.softmax_predict(Xs, z), c.softmax_predict(Xs[:1], z)]


def small_binary_calls(c):
    X, y, Xs = binary_problem(129, D, 5)
    return [c.laplace_fit(X, y, SIGMA, ELL), c.laplace_predict(Xs), c.laplace_predict(Xs[:1])]


def flat(calls):
    return [np.asarray(v) for call in calls for v in call]


@pytest.mark.parametrize("kind", ["softmax", "binary"])
def test_small_fit_after_a_large_one_same_bits_as_a_fresh_context(ctx, kind):
    """N = 1100 (C = 5, predicted at 300 points) leaves its contents in the padding of every buffer the N = 129 (C = 3)
    fit and its predictions at 300 points and then 1 point reuse; a context that has seen nothing else gives the
    reference bits"""
    from gaussian_process_amd import GPContext
    if kind == "softmax":
        X, lab, Xs = SR.blobs(1100, D, 5, 1100, n=300)
        ctx.softmax_fit(X, lab, 5, SIGMA, ELL)
        ctx.softmax_predict(Xs, np.random.default_rng(1).standard_normal((300, 5)))
        small = small_softmax_calls
    else:
        X, y, Xs = binary_problem(1100, D, 1100)
        ctx.laplace_fit(X, y, SIGMA, ELL)
        ctx.laplace_predict(Xs)
        small = small_binary_calls
    got = flat(small(ctx))
    fresh = GPContext(0)
    try:
        want = flat(small(fresh))
    finally:
        fresh.close()
    assert len(got) == len(want)
    for g, w in zip(got, want):
        assert g.shape == w.shape and np.array_equal(g, w)
