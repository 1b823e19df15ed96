"""gpmi_softmax_grad on the MI355X: against the NumPy mirror (tests/softmax_grad_ref.py) under the bars of
tests/test_softmax_grad_cpu.py (50 x the mirror's own response to rounding in K, floored at 1e-11; read its docstring),
against gpmi_laplace_grad at C = 2, null pointers, bitwise reproducibility, that the call only reads the fit, that the
other gradients keep their bits, the refusals, and GP_multi_classification's log_q_and_gradient and tuner.  Every fit
runs with tol = 1e-13: the formula holds at the mode."""
import warnings

import numpy as np
import pytest

import softmax_grad_ref as G
import softmax_ref as S
from test_softmax_grad_cpu import CASES, FIT_TOL, ROUNDING, c2_case, gpu_bar, make_case, n2000_case

pytestmark = pytest.mark.gpu


@pytest.fixture(autouse=True)
def isotropic_rbf_afterwards(ctx):
    yield
    ctx.set_kernel("rbf")
    ctx.set_lengthscales(None)


def gpu_flat(ctx):
    d_r, d_l, d_sigma = ctx.softmax_grad()
    return np.concatenate([d_r, [d_l, d_sigma]])


def compare(ctx, tag, X, lab, C, sigma, l, r, bar):
    ref = G.log_q_and_gradient(X, lab, C, sigma, l, r, tol=FIT_TOL)
    assert ref["fit"]["converged"]
    log_q, _, iters, conv = ctx.softmax_fit(X, lab, C, sigma, l, tol=FIT_TOL, lengthscales=r)
    g = gpu_flat(ctx)
    rf = G.flat(ref)
    err = float(np.max(np.abs(g - rf)) / np.max(np.abs(rf)))
    print("%s: gpu - mirror %.3g (bar %.3g), %d Newton steps, log q %.3g apart"
          % (tag, err, bar, iters, abs(log_q - ref["log_q"]) / abs(ref["log_q"])))
    assert conv
    assert np.all(np.isfinite(g))
    assert err <= bar


@pytest.mark.parametrize("name", list(CASES))
def test_gpu_matches_mirror(ctx, name):
    X, lab, C, sigma, l, r = make_case(name)
    compare(ctx, name, X, lab, C, sigma, l, r, gpu_bar(ROUNDING[name]))


def test_gpu_matches_mirror_N2000(ctx):
    """several row blocks of the sweeps and the products, on the inputs of tests/golden/laplace/moons_N2000_d2"""
    X, lab, C, sigma, l, r = n2000_case()
    assert sorted(set(lab.tolist())) == [0, 1, 2]
    compare(ctx, "moons_N2000_d2_C3", X, lab, C, sigma, l, r, gpu_bar(ROUNDING["moons_N2000_d2_C3_ard"]))


def test_two_classes_equal_the_binary_gradient(ctx):
    """the softmax model with kernel K at C = 2 is the binary model with kernel 2 K: sigma sqrt(2), d_sigma times sqrt(2)"""
    X, lab, y, sigma, l, r = c2_case()
    log_q, _, _, conv = ctx.softmax_fit(X, lab, 2, sigma, l, tol=FIT_TOL, lengthscales=r)
    a = gpu_flat(ctx)
    assert conv
    log_qb, _, _, convb = ctx.laplace_fit(X, y, np.sqrt(2.0) * sigma, l, tol=FIT_TOL, lengthscales=r)
    d_r, d_l, d_sigma = ctx.laplace_grad()
    assert convb
    b = np.concatenate([d_r, [d_l, d_sigma * np.sqrt(2.0)]])
    err = float(np.max(np.abs(a - b)) / np.max(np.abs(b)))
    bar = gpu_bar(ROUNDING["c2_softmax"]) + gpu_bar(ROUNDING["c2_binary"])
    print("C = 2: softmax - binary on the GPU %.3g (bar %.3g), log q %.3g apart" % (err, bar, abs(log_q - log_qb) / abs(log_qb)))
    assert err <= bar


def test_null_pointers_accepted(ctx):
    import ctypes as C
    X, lab, nc, sigma, l, r = make_case("N129_d3_C4_ard")
    ctx.softmax_fit(X, lab, nc, sigma, l, tol=FIT_TOL, lengthscales=r)
    full = gpu_flat(ctx)
    lib, h = ctx._lib, ctx._h
    dp = C.POINTER(C.c_double)
    for want_r in (False, True):
        for want_l in (False, True):
            for want_s in (False, True):
                d_r = np.full(3, np.nan)
                dl, ds = C.c_double(np.nan), C.c_double(np.nan)
                assert lib.gpmi_softmax_grad(h, d_r.ctypes.data_as(dp) if want_r else None, C.byref(dl) if want_l else None,
                                             C.byref(ds) if want_s else None) == 0
                assert not want_r or np.array_equal(d_r, full[:3])
                assert not want_l or dl.value == full[-2]
                assert not want_s or ds.value == full[-1]
    assert lib.gpmi_softmax_grad(None, None, None, None) != 0


def test_two_calls_same_bits_and_the_fit_is_only_read(ctx):
    X, lab, C, sigma, l, r = make_case("N300_d8_C10_ard")
    Xs = S.blobs(200, 8, 10, 77)[0]
    z = np.random.default_rng(3).standard_normal((16, C))
    ctx.softmax_fit(X, lab, C, sigma, l, tol=FIT_TOL, lengthscales=r)
    before = ctx.softmax_predict(Xs, z)
    a = gpu_flat(ctx)
    b = gpu_flat(ctx)
    assert np.array_equal(a, b)
    after = ctx.softmax_predict(Xs, z)
    for u, v in zip(before, after):
        assert np.array_equal(u, v)
    assert np.array_equal(gpu_flat(ctx), a)                               # and after a prediction
    assert ctx.timers()["grad"] > 0.0
    # a fresh fit of the same problem: the same bits again, and the prediction's too
    ctx.softmax_fit(X, lab, C, sigma, l, tol=FIT_TOL, lengthscales=r)
    assert np.array_equal(gpu_flat(ctx), a)
    for u, v in zip(before, ctx.softmax_predict(Xs, z)):
        assert np.array_equal(u, v)


def test_other_gradients_keep_their_bits(ctx):
    X, lab, C, sigma, l, r = make_case("N300_d8_C10_ard")
    yr = np.sin(X[:, 0]) + 0.1 * lab
    yb = np.where(lab < 5, -1.0, 1.0)
    ctx.fit(X, yr, 1.2, 2.0, 1e-3, lengthscales=r)
    g0 = ctx.lml_grad_ard()
    ctx.laplace_fit(X, yb, sigma, l, tol=FIT_TOL, lengthscales=r)
    b0 = ctx.laplace_grad()
    ctx.softmax_fit(X, lab, C, sigma, l, tol=FIT_TOL, lengthscales=r)
    ctx.softmax_grad()
    ctx.fit(X, yr, 1.2, 2.0, 1e-3, lengthscales=r)
    g1 = ctx.lml_grad_ard()
    ctx.laplace_fit(X, yb, sigma, l, tol=FIT_TOL, lengthscales=r)
    b1 = ctx.laplace_grad()
    assert np.array_equal(g0[0], g1[0]) and g0[1:] == g1[1:]
    assert np.array_equal(b0[0], b1[0]) and b0[1:] == b1[1:]


def refused(ctx):
    with pytest.raises(ValueError, match=r"no softmax fit resident \(call gpmi_softmax_fit\)"):
        ctx.softmax_grad()


def test_refusals_leave_the_context_as_it_was(ctx):
    X, lab, C, sigma, l, _ = make_case("N129_d3_C4_iso")
    y = np.where(lab < 2, -1.0, 1.0)
    Xs = S.blobs(64, 3, 4, 78)[0]
    ctx.set_train(X, y)                                                   # no fit at all
    refused(ctx)
    ctx.fit(X, y, 1.0, 1.5, 1e-3)                                         # a regression fit
    al = ctx.alpha()
    refused(ctx)
    assert np.array_equal(ctx.alpha(), al)
    ctx.laplace_fit(X, y, sigma, l)                                       # a binary Laplace fit
    fm = ctx.laplace_predict(Xs)[0]
    refused(ctx)
    assert np.array_equal(ctx.laplace_predict(Xs)[0], fm)
    ctx.sparse_fit(X, y, X[:32].copy(), 1.0, 1.5, 1e-2)                   # a sparse fit
    sm = ctx.sparse_predict(Xs, want_sd=False)[0]
    refused(ctx)
    assert np.array_equal(ctx.sparse_predict(Xs, want_sd=False)[0], sm)
    ctx.softmax_fit(X, lab, C, sigma, l, tol=FIT_TOL)
    g = gpu_flat(ctx)
    ctx.set_lengthscales([1.0, 2.0, 0.5])                                 # drops the fit
    refused(ctx)
    ctx.set_lengthscales(None)
    ctx.softmax_fit(X, lab, C, sigma, l, tol=FIT_TOL, lengthscales=None)
    assert np.array_equal(gpu_flat(ctx), g)
    ctx.set_kernel("matern32")                                            # drops the fit
    refused(ctx)
    ctx.set_kernel("rbf")
    refused(ctx)
    ctx.softmax_fit(X, lab, C, sigma, l, tol=FIT_TOL)
    assert np.array_equal(gpu_flat(ctx), g)


def test_python_conventions(ctx):
    """log_q_and_gradient: absolute lengthscales (common l = 1), or a scalar giving one derivative"""
    from gaussian_process_amd import GP_multi_classification as M
    X, lab, C, sigma, l, r = make_case("N129_d3_C4_ard")
    ref = G.log_q_and_gradient(X, lab, C, sigma, 1.0, l * r, tol=FIT_TOL)
    log_q, d_ls, d_sigma = M.log_q_and_gradient(X, lab, sigma, l * r, n_classes=C, ctx=ctx)
    bar = gpu_bar(ROUNDING["N129_d3_C4_ard"])
    scale = np.max(np.abs(G.flat(ref)))
    assert d_ls.shape == (3,) and np.max(np.abs(d_ls - ref["d_r"])) <= bar * scale and abs(d_sigma - ref["d_sigma"]) <= bar * scale
    assert abs(log_q - ref["log_q"]) <= 1e-11 * abs(ref["log_q"])
    ref = G.log_q_and_gradient(X, lab, C, sigma, l, None, tol=FIT_TOL)
    log_q, d_l, d_sigma = M.log_q_and_gradient(X, lab, sigma, l, ctx=ctx)
    bar = gpu_bar(ROUNDING["N129_d3_C4_iso"])
    scale = np.max(np.abs(G.flat(ref)))
    assert np.ndim(d_l) == 0 and abs(d_l - ref["d_l"]) <= bar * scale and abs(d_sigma - ref["d_sigma"]) <= bar * scale
    assert np.array_equal(ctx.softmax_grad()[0] * 0, np.zeros(3))        # still resident, isotropic


def test_tuner_on_three_blobs(ctx):
    """from a poor start (l = 5): log q never decreases along the accepted steps, ends above its start, and the ascent
    ends with a gradient norm (w.r.t. the logarithms) below tol or at max_iter with a warning"""
    from gaussian_process_amd import GP_multi_classification as M
    X, lab, Xs = S.blobs(300, 2, 3, 11, n=100)
    max_iter, tol = 40, 1e-6
    with warnings.catch_warnings(record=True) as w:
        warnings.simplefilter("always")
        ls, sigma, log_q, trace = M.tune_hyperparms_classification(X, lab, sigma=1.0, lengthscales=5.0, max_iter=max_iter,
                                                                   tol=tol, ctx=ctx)
    d_r, _, d_sigma = ctx.softmax_grad()                                  # the best fit is resident
    gnorm = float(np.linalg.norm(np.concatenate([d_r * ls, [d_sigma * sigma]])))
    print("tuner: %d steps, log q %.6f -> %.6f, lengthscales %s sigma %.4f, gradient norm %.3g"
          % (len(trace) - 1, trace[0], trace[-1], ls, sigma, gnorm))
    assert np.all(np.diff(trace) >= 0)
    assert trace[-1] > trace[0] and log_q == trace[-1]
    warned = any(issubclass(x.category, RuntimeWarning) for x in w)
    assert gnorm < tol or (len(trace) - 1 == max_iter and warned)
    p = M.predict_proba(Xs, n_samples=64, ctx=ctx)                        # follows directly
    assert p.shape == (100, 3) and np.all((p > 0) & (p < 1)) and np.allclose(p.sum(axis=1), 1.0)
    ref = S.fit(X / ls, lab, 3, sigma, 1.0, tol=FIT_TOL)
    assert abs(log_q - ref["log_q"]) <= 1e-11 * abs(ref["log_q"])
