"""gpmi_laplace_grad on the MI355X: against the NumPy mirror (tests/laplace_grad_ref.py) and the scikit-learn fixtures
(tests/golden/laplace_grad) under the bars of tests/test_laplace_grad_cpu.py (50 x the mirror's own response to rounding
in K, floored at 1e-11; read its docstring), null pointers, bitwise reproducibility, that the call only reads the fit,
the refusals, and tune_hyperparms_classification.  Every fit runs with tol = 1e-13: the formula holds at the mode."""
import os
import warnings

import numpy as np
import pytest

import laplace_grad_ref as G
from conftest import GOLDEN
from test_laplace_grad_cpu import (CASES, FIT_TOL, FIXTURE_DISTANCE, FIXTURES, ROUNDING, fixture_case, gpu_bar, make_case,
                                   n2000_case, problem)

pytestmark = pytest.mark.gpu


@pytest.fixture(autouse=True)
def isotropic_rbf_afterwards(ctx):
    yield
    ctx.set_kernel("rbf")
    ctx.set_lengthscales(None)


def gpu_flat(ctx):
    d_r, d_l, d_sigma = ctx.laplace_grad()
    return np.concatenate([d_r, [d_l, d_sigma]])


def compare(ctx, tag, X, y, sigma, l, r, ref, ref_log_q, bar):
    log_q, _, iters, conv = ctx.laplace_fit(X, y, sigma, l, tol=FIT_TOL, lengthscales=r)
    g = gpu_flat(ctx)
    err = float(np.max(np.abs(g - ref)) / np.max(np.abs(ref)))
    print("%s: gpu - reference %.3g (bar %.3g), %d Newton steps, log q %.3g apart"
          % (tag, err, bar, iters, abs(log_q - ref_log_q) / abs(ref_log_q)))
    assert conv
    assert np.all(np.isfinite(g))
    assert err <= bar


@pytest.mark.parametrize("name", list(CASES))
def test_gpu_matches_mirror(ctx, name):
    X, y, sigma, l, r = make_case(name)
    ref = G.log_q_and_gradient(X, y, sigma, l, r, tol=FIT_TOL)
    assert ref["fit"]["converged"]
    compare(ctx, name, X, y, sigma, l, r, G.flat(ref), ref["log_q"], gpu_bar(ROUNDING[name]))


def test_gpu_matches_mirror_N2000(ctx):
    """several row blocks of the inverse and the product, on the inputs of tests/golden/laplace/moons_N2000_d2"""
    X, y, sigma, l, r = n2000_case()
    ref = G.log_q_and_gradient(X, y, sigma, l, r, tol=FIT_TOL)
    compare(ctx, "moons_N2000_d2", X, y, sigma, l, r, G.flat(ref), ref["log_q"], gpu_bar(ROUNDING["moons_N2000_d2_ard"]))


@pytest.mark.parametrize("path", FIXTURES, ids=lambda p: os.path.basename(p)[:-4])
def test_gpu_matches_sklearn(ctx, path):
    name = os.path.basename(path)[:-4]
    X, y, sigma, l, r, ref, lml = fixture_case(path)
    compare(ctx, name, X, y, sigma, l, r, ref, lml, gpu_bar(ROUNDING[name]) + FIXTURE_DISTANCE[name])


def test_python_conventions(ctx):
    """log_q_and_gradient: absolute lengthscales (common l = 1), or a scalar giving one derivative"""
    from gaussian_process_amd import GP_binary_classification as B
    X, y, sigma, l, r = make_case("N129_d3_ard")
    ref = G.log_q_and_gradient(X, y, sigma, 1.0, l * r, tol=FIT_TOL)
    log_q, d_ls, d_sigma = B.log_q_and_gradient(X, y, sigma, l * r, ctx=ctx)
    bar = gpu_bar(ROUNDING["N129_d3_ard"])
    scale = np.max(np.abs(G.flat(ref)))
    assert d_ls.shape == (3,) and np.max(np.abs(d_ls - ref["d_r"])) <= bar * scale and abs(d_sigma - ref["d_sigma"]) <= bar * scale
    assert abs(log_q - ref["log_q"]) <= 1e-11 * abs(ref["log_q"])
    ref = G.log_q_and_gradient(X, y, sigma, l, None, tol=FIT_TOL)
    log_q, d_l, d_sigma = B.log_q_and_gradient(X, y, sigma, l, ctx=ctx)
    bar = gpu_bar(ROUNDING["N129_d3_iso"])
    scale = np.max(np.abs(G.flat(ref)))
    assert np.ndim(d_l) == 0 and abs(d_l - ref["d_l"]) <= bar * scale and abs(d_sigma - ref["d_sigma"]) <= bar * scale
    assert np.array_equal(ctx.laplace_grad()[0] * 0, np.zeros(3))        # still resident, isotropic


def test_null_pointers_accepted(ctx):
    import ctypes as C
    X, y, sigma, l, r = make_case("N129_d3_ard")
    ctx.laplace_fit(X, y, sigma, l, tol=FIT_TOL, lengthscales=r)
    full = gpu_flat(ctx)
    lib, h = ctx._lib, ctx._h
    assert lib.gpmi_laplace_grad(h, None, None, None) == 0
    ds, dl = C.c_double(), C.c_double()
    assert lib.gpmi_laplace_grad(h, None, None, C.byref(ds)) == 0 and ds.value == full[-1]
    assert lib.gpmi_laplace_grad(h, None, C.byref(dl), None) == 0 and dl.value == full[-2]
    d_r = np.empty(3)
    assert lib.gpmi_laplace_grad(h, d_r.ctypes.data_as(C.POINTER(C.c_double)), None, None) == 0
    assert np.array_equal(d_r, full[:3])
    assert lib.gpmi_laplace_grad(None, None, None, None) != 0


def test_two_calls_same_bits_and_the_fit_is_only_read(ctx):
    X, y, sigma, l, r = make_case("N300_d8_ard")
    Xs = problem(200, 8, 77)[0]
    ctx.laplace_fit(X, y, sigma, l, tol=FIT_TOL, lengthscales=r)
    before = ctx.laplace_predict(Xs)
    a = gpu_flat(ctx)
    b = gpu_flat(ctx)
    assert np.array_equal(a, b)
    after = ctx.laplace_predict(Xs)
    for u, v in zip(before, after):
        assert np.array_equal(u, v)
    assert np.array_equal(gpu_flat(ctx), a)                               # and after a prediction
    assert ctx.timers()["grad"] > 0.0
    # a fresh fit of the same problem: the same bits again
    ctx.laplace_fit(X, y, sigma, l, tol=FIT_TOL, lengthscales=r)
    assert np.array_equal(gpu_flat(ctx), a)


def test_regression_gradient_keeps_its_bits(ctx):
    X, y, sigma, l, r = make_case("N300_d8_ard")
    yr = y + 0.1 * np.sin(X[:, 0])
    ctx.fit(X, yr, 1.2, 2.0, 1e-3, lengthscales=r)
    g0 = ctx.lml_grad_ard()
    ctx.laplace_fit(X, y, sigma, l, tol=FIT_TOL, lengthscales=r)
    ctx.laplace_grad()
    ctx.fit(X, yr, 1.2, 2.0, 1e-3, lengthscales=r)
    g1 = ctx.lml_grad_ard()
    assert np.array_equal(g0[0], g1[0]) and g0[1:] == g1[1:]


def refused(ctx):
    with pytest.raises(ValueError, match="no Laplace fit resident"):
        ctx.laplace_grad()


def test_refusals_leave_the_context_as_it_was(ctx):
    X, y, sigma, l, _ = make_case("N129_d3_iso")
    Xs = problem(64, 3, 78)[0]
    ctx.set_train(X, y)                                                   # no fit at all
    refused(ctx)
    ctx.fit(X, y, 1.0, 1.5, 1e-3)                                         # a regression fit
    al = ctx.alpha()
    refused(ctx)
    assert np.array_equal(ctx.alpha(), al)
    ctx.lml_grad_ard()
    ctx.softmax_fit(X, np.where(y > 0, 0, 1), 2, 1.0, 1.5)                # a softmax fit
    mu = ctx.softmax_predict(Xs)[0]
    refused(ctx)
    assert np.array_equal(ctx.softmax_predict(Xs)[0], mu)
    ctx.sparse_fit(X, y, X[:32].copy(), 1.0, 1.5, 1e-2)                   # a sparse fit
    sm = ctx.sparse_predict(Xs, want_sd=False)[0]
    refused(ctx)
    assert np.array_equal(ctx.sparse_predict(Xs, want_sd=False)[0], sm)
    ctx.laplace_fit(X, y, sigma, l, tol=FIT_TOL)
    g = gpu_flat(ctx)
    ctx.set_lengthscales([1.0, 2.0, 0.5])                                 # drops the fit
    refused(ctx)
    with pytest.raises(ValueError):
        ctx.laplace_predict(Xs)
    ctx.set_lengthscales(None)
    ctx.laplace_fit(X, y, sigma, l, tol=FIT_TOL, lengthscales=None)
    assert np.array_equal(gpu_flat(ctx), g)
    ctx.set_kernel("matern32")                                            # drops the fit
    refused(ctx)
    ctx.set_kernel("rbf")
    refused(ctx)
    ctx.laplace_fit(X, y, sigma, l, tol=FIT_TOL)
    assert np.array_equal(gpu_flat(ctx), g)


def test_tuner_on_two_blobs(ctx):
    """from a poor start (l = 5): log q never decreases along the accepted steps, ends above its start, and the ascent
    ends with a gradient norm (w.r.t. the logarithms) below tol or at max_iter with a warning"""
    from gaussian_process_amd import GP_binary_classification as B
    X, y = problem(300, 2, 11)
    Xs = problem(100, 2, 79)[0]
    max_iter, tol = 100, 1e-6
    with warnings.catch_warnings(record=True) as w:
        warnings.simplefilter("always")
        ls, sigma, log_q, trace = B.tune_hyperparms_classification(X, y, sigma=1.0, lengthscales=5.0, max_iter=max_iter,
                                                                   tol=tol, ctx=ctx)
    d_r, _, d_sigma = ctx.laplace_grad()                                  # the best fit is resident
    gnorm = float(np.linalg.norm(np.concatenate([d_r * ls, [d_sigma * sigma]])))
    print("tuner: %d steps, log q %.6f -> %.6f, lengthscales %s sigma %.4f, gradient norm %.3g"
          % (len(trace) - 1, trace[0], trace[-1], ls, sigma, gnorm))
    assert np.all(np.diff(trace) >= 0)
    assert trace[-1] > trace[0] and log_q == trace[-1]
    warned = any(issubclass(x.category, RuntimeWarning) for x in w)
    assert gnorm < tol or (len(trace) - 1 == max_iter and warned)
    p = B.predict_proba(Xs, ctx=ctx)                                      # follows directly
    assert p.shape == (100,) and np.all((p > 0) & (p < 1))
    ref = G.log_q_and_gradient(X, y, sigma, 1.0, ls, tol=FIT_TOL)
    assert abs(log_q - ref["log_q"]) <= 1e-11 * abs(ref["log_q"])
