"""gpmi_lml_grad_co2 on the GPU: the LML gradient of the CO2 composite kernel (kind 3) against the NumPy mirror of
tests/co2_grad_ref.py, its state rules, and CO2_example.py's gradient functions on top of it.  The bars are the
project's existing ones: GRAD_RTOL times each component's cancellation scale for the gradient, 1e-9 for the LML (the CO2
bar of tests/test_parity_gpu.py)."""
import ctypes as C

import numpy as np
import pytest

import co2_grad_ref as R
from conftest import golden

pytestmark = pytest.mark.gpu

GRAD_RTOL = 1e-8      # tests/test_parity_gpu.py: relative to the two terms the trace cancels
LML_RTOL = 1e-9       # tests/test_parity_gpu.py: the CO2 fit
D_BIG = 40            # above the 32 dimensions grad_co2_kernel stages in LDS: X is read from global memory


@pytest.fixture(scope="module")
def cctx():
    """a context of this module's own: the kernel kind is context state, and the session's shared one stays on 'rbf'"""
    from gaussian_process_amd import GPContext
    c = GPContext(0)
    yield c
    c.close()


@pytest.fixture(scope="module")
def book():
    g = golden("kernels_bo_co2")
    return g["co2_theta"], g["co2_X"], g["co2_y"]


_cache = {}


def fixture_mirror(book, N):
    """the long-double mirror on the fixture's first N points: one evaluation per size, shared and left unchanged"""
    th, X, y = book
    if ("ld", N) not in _cache:
        _cache[("ld", N)] = R.lml_and_grad(X[:N], y[:N], th, R.NOISE, np.longdouble)
    return _cache[("ld", N)]


def synthetic(N, d):
    """the float64 mirror on the positive definite multi-dimensional problem, one evaluation per shape"""
    if (N, d) not in _cache:
        X, y = R.problem_md(N, d, seed=100 + d)
        _cache[(N, d)] = (X, y, R.lml_and_grad(X, y, R.THETA_MD))
    return _cache[(N, d)]


def fit(c, X, y, th, noise=R.NOISE):
    c.set_kernel("co2", th)
    return c.fit(X, y, 1.0, 1.0, noise)


def hold(got, ref, tag, bar=GRAD_RTOL):
    err = R.error_over_scale(got[0], got[1], ref)
    print("%s: error / scale per component (theta_1..11, noise): %s" % (tag, " ".join("%.1e" % e for e in err)))
    assert np.all(np.isfinite(err)) and np.all(err <= bar), (tag, int(err.argmax()), float(err.max()))


# ------------------------------------------------------------------------------------ gradient against the mirror
@pytest.mark.parametrize("N", [1, 128, 130, 300, 360])
def test_fixture_gradient_against_long_double(cctx, book, N):
    """one tile, ragged two and three tile rows, the whole fixture (K_y of condition up to 4e7)"""
    th, X, y = book
    ref = fixture_mirror(book, N)
    try:
        lml = fit(cctx, X[:N], y[:N], th)
        got = cctx.lml_grad_co2()
    finally:
        cctx.set_kernel("rbf")
    assert abs(lml - float(ref["lml"])) <= LML_RTOL * abs(float(ref["lml"])), (lml, float(ref["lml"]))
    hold(got, ref, "fixture N=%d" % N)


@pytest.mark.parametrize("N,d", [(130, 2), (257, 11), (200, D_BIG)])
def test_synthetic_gradient_against_the_mirror(cctx, N, d):
    """d > 1 staged in LDS, and d above the LDS width (the instantiation that reads X from global memory)"""
    X, y, ref = synthetic(N, d)
    try:
        lml = fit(cctx, X, y, R.THETA_MD)
        got = cctx.lml_grad_co2()
    finally:
        cctx.set_kernel("rbf")
    assert abs(lml - ref["lml"]) <= LML_RTOL * abs(ref["lml"])
    hold(got, ref, "N=%d d=%d" % (N, d))


@pytest.mark.parametrize("nb", [128, 256, 0])
def test_gradient_mid_size_and_blocking(cctx, nb):
    """the factor-inverse front at several block sizes, nine tile rows"""
    X, y, ref = synthetic(1100, 3)
    cctx.set_option("nb", nb)
    try:
        fit(cctx, X, y, R.THETA_MD)
        got = cctx.lml_grad_co2()
    finally:
        cctx.set_option("nb", 0)
        cctx.set_kernel("rbf")
    hold(got, ref, "N=1100 d=3 nb=%d" % nb)


def test_noise_and_theta11_share_the_diagonal_sum(cctx, book):
    th, X, y = book
    try:
        fit(cctx, X[:300], y[:300], th)
        d_theta, d_noise = cctx.lml_grad_co2()
    finally:
        cctx.set_kernel("rbf")
    want = d_theta[10] / (2 * th[10])
    assert abs(d_noise - want) <= 1e-12 * abs(want), (d_noise, want)


def test_outputs_are_optional(cctx):
    from gaussian_process_amd._lib import check, ptr
    X, y, _ = synthetic(130, 2)
    try:
        fit(cctx, X, y, R.THETA_MD)
        full = cctx.lml_grad_co2()
        dn = C.c_double()
        check(cctx._lib.gpmi_lml_grad_co2(cctx._h, None, C.byref(dn)))
        assert dn.value == full[1]
        dt = np.empty(11)
        check(cctx._lib.gpmi_lml_grad_co2(cctx._h, ptr(dt), None))
        assert np.array_equal(dt, full[0])
        check(cctx._lib.gpmi_lml_grad_co2(cctx._h, None, None))
    finally:
        cctx.set_kernel("rbf")


@pytest.mark.parametrize("case", ["fixture_300_1", "synthetic_257_11"])
def test_gradient_is_bitwise_reproducible(cctx, book, case):
    if case == "fixture_300_1":
        th, X, y = book[0], book[1][:300], book[2][:300]
    else:
        th, (X, y, _) = R.THETA_MD, synthetic(257, 11)
    try:
        fit(cctx, X, y, th)
        g1 = cctx.lml_grad_co2()
        g2 = cctx.lml_grad_co2()
    finally:
        cctx.set_kernel("rbf")
    assert np.array_equal(g1[0], g2[0]) and g1[1] == g2[1]


# ---------------------------------------------------------------------------------------------------- state rules
def test_state_rules(cctx):
    from gaussian_process_amd import GPContext
    X, y, ref = synthetic(130, 2)
    Xs = X[:10] + 0.01
    empty = GPContext(0)
    try:
        with pytest.raises(ValueError, match="no regression factorisation resident"):
            empty.lml_grad_co2()
        empty.set_kernel("co2", R.THETA_MD)
        with pytest.raises(ValueError, match="no regression factorisation resident"):
            empty.lml_grad_co2()
    finally:
        empty.close()
    try:
        cctx.set_kernel("rbf")
        cctx.fit(X, y, 1.0, 1.0, R.NOISE)
        with pytest.raises(ValueError, match="kind 3"):
            cctx.lml_grad_co2()
        cctx.laplace_fit(X, np.where(y > 0, 1.0, -1.0), 1.0, 1.0)
        with pytest.raises(ValueError):
            cctx.lml_grad_co2()
        # the call only reads the fit
        fit(cctx, X, y, R.THETA_MD)
        alpha, pred = cctx.alpha(), cctx.predict(Xs)
        cctx.lml_grad_co2()
        assert np.array_equal(cctx.alpha(), alpha)
        again = cctx.predict_resident()
        assert np.array_equal(again[0], pred[0]) and np.array_equal(again[1], pred[1])
        # the older gradients keep refusing the composite kernel, in their own words
        for call, text in ((cctx.lml_grad, r"gpmi_lml_grad: squared-exponential or Matern kernel only \(kinds 0, 4, 5, 6\)"),
                           (cctx.lml_grad_ard, r"gpmi_lml_grad_ard: squared-exponential or Matern kernel only \(kinds 0, 4, 5, 6\)")):
            with pytest.raises(ValueError, match=text):
                call()
        hold(cctx.lml_grad_co2(), ref, "after the refusals")
    finally:
        cctx.set_kernel("rbf")


def test_gradient_after_a_refused_append(cctx):
    """gpmi_append refuses the composite kernel (its delta term belongs to a square matrix; tests/test_append_gpu.py),
    so there is no extended kind-3 fit to differentiate: the refusal leaves the fit, and the gradient, as they were"""
    X, y, ref = synthetic(130, 2)
    try:
        fit(cctx, X[:127], y[:127], R.THETA_MD)
        before = cctx.lml_grad_co2()
        with pytest.raises(ValueError, match="composite kernel"):
            cctx.append(X[127:], y[127:])
        after = cctx.lml_grad_co2()
        assert cctx.N == 127 and np.array_equal(before[0], after[0]) and before[1] == after[1]
        fit(cctx, X, y, R.THETA_MD)                              # the 130 points take a fit of their own
        hold(cctx.lml_grad_co2(), ref, "refit on 127 + 3")
    finally:
        cctx.set_kernel("rbf")


# ------------------------------------------------------------------------------------------- CO2_example's functions
def test_lml_and_gradient_is_the_two_calls(cctx, book):
    from gaussian_process_amd import CO2_example as C2
    th, X, y = book
    lml, d_theta, d_noise = C2.lml_and_gradient(X, y, th, ctx=cctx)
    assert lml == C2.compute_mar_likelihood(X, y, th, ctx=cctx)
    try:
        fit(cctx, X, y, th, C2.NOISE_VAR)
        want = cctx.lml_grad_co2()
    finally:
        cctx.set_kernel("rbf")
    assert np.array_equal(d_theta, want[0]) and d_noise == want[1]
    # left on 'rbf': the next fit is a squared-exponential one and the composite gradient refuses it
    cctx.fit(X[:64], y[:64], 1.0, 1.0, R.NOISE)
    with pytest.raises(ValueError, match="kind 3"):
        cctx.lml_grad_co2()


def test_tuner_from_the_book_values(cctx, book):
    from gaussian_process_amd import CO2_example as C2
    _, X, y = book
    th, noise, lml, trace = C2.tune_hyperparameters_gradient(X, y, max_iter=15, ctx=cctx)
    print("tuner: lml %.6f -> %.6f in %d accepted steps; theta %s" % (trace[0], lml, len(trace) - 1, th))
    assert np.all(np.diff(trace) >= 0)
    assert lml > trace[0] and trace[-1] == lml
    assert noise == C2.NOISE_VAR
    at = C2.compute_mar_likelihood(X, y, th, ctx=cctx)
    assert abs(lml - at) <= 1e-9 * abs(at), (lml, at)
