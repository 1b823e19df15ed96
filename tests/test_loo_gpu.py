"""Leave-one-out cross-validation on the GPU: gpmi_loo and gpmi_loo_grad against the NumPy mirror of tests/loo_ref.py.
The bars are the project's existing ones: LML_RTOL for values, GRAD_RTOL times each component's cancellation scale for
the derivatives."""
import ctypes as C

import numpy as np
import pytest

import ard_ref as R
import loo_ref as LR

pytestmark = pytest.mark.gpu

LML_RTOL = 1e-10      # tests/test_parity_gpu.py
GRAD_RTOL = 1e-8      # tests/test_parity_gpu.py: relative to the terms that cancel
SIGMA, ELL = 1.2, 1.3
# the three inputs of tests/test_loo_cpu.py, exactly one tile, several tiles and no multiple of 128
CASES = [(130, 2, 1e-2), (300, 5, 5e-4), (257, 8, 5e-4), (128, 3, 1e-2), (641, 5, 5e-4)]
MID = (1500, 8, 5e-4)


@pytest.fixture(scope="module")
def lctx():
    """a context of this module's own: lengthscales, the kernel kind and options are context state"""
    from gaussian_process_amd import GPContext
    c = GPContext(0)
    yield c
    c.close()


@pytest.fixture(scope="module")
def fresh():
    from gaussian_process_amd import GPContext
    c = GPContext(0)
    yield c
    c.close()


_cache = {}


def _mirror(N, d, noise):
    """one mirror evaluation per input, shared by the tests below and left unchanged"""
    key = (N, d, noise)
    if key not in _cache:
        X, y = R.problem(N, d, seed=100 + d)
        _cache[key] = (X, y, LR.closed(X, y, np.ones(d), SIGMA, ELL, noise))
    return _cache[key]


def _hold_values(got, ref, y, tag):
    mu, var, logp, tot = got
    e_mu = np.max(np.abs(mu - ref["mu"]))
    e_var = np.max(np.abs(var - ref["var"]) / ref["var"])
    e_lp = np.max(np.abs(logp - ref["logp"]) / np.maximum(1.0, np.abs(ref["logp"])))
    e_tot = abs(tot - ref["loo"]) / np.sum(np.abs(ref["logp"]))
    print("%s cond %.2e: mu %.2e var %.2e logp %.2e total %.2e" % (tag, ref["cond"], e_mu, e_var, e_lp, e_tot))
    assert e_mu <= 1e-10 * max(1.0, np.max(np.abs(y)))
    assert e_var <= 1e-10
    assert e_lp <= 1e-10
    assert e_tot <= LML_RTOL


def _hold_gradient(got, ref, tag):
    errs = [abs(g - ref["g_" + k]) / ref["s_" + k] for g, k in zip(got, ("l", "sigma", "noise"))]
    print("%s cond %.2e: error / scale l %.2e, sigma %.2e, noise %.2e" % (tag, ref["cond"], errs[0], errs[1], errs[2]))
    for e, k in zip(errs, ("l", "sigma", "noise")):
        assert e <= GRAD_RTOL, (tag, k, e)


# ------------------------------------------------------------------------------------------------------------ values
@pytest.mark.parametrize("N,d,noise", CASES)
def test_values_against_the_mirror(lctx, N, d, noise):
    X, y, ref = _mirror(N, d, noise)
    lctx.fit(X, y, SIGMA, ELL, noise)
    _hold_values(lctx.loo(), ref, y, "N=%d d=%d noise=%g" % (N, d, noise))


def test_values_with_the_linear_kernel(lctx):
    """gpmi_loo reads L, m and y only: kind 1, K = (X - c)(X - c)^T, with a noise that keeps K_y well conditioned"""
    X, y = R.problem(130, 2, seed=21)
    c, noise = 0.5, 1.0
    ref = LR.from_Ky((X - c) @ (X - c).T + noise * np.eye(130), y)
    try:
        lctx.set_kernel("lin", c)
        lctx.fit(X, y, 1.0, 1.0, noise)
        _hold_values(lctx.loo(), ref, y, "linear N=130")
        with pytest.raises(ValueError):
            lctx.loo_grad()                                   # squared-exponential only
    finally:
        lctx.set_kernel("rbf")
    lctx.fit(X, y, SIGMA, ELL, 1e-2)
    assert len(lctx.loo_grad()) == 3


def test_outputs_are_optional(lctx):
    from gaussian_process_amd._lib import check
    X, y, _ = _mirror(130, 2, 1e-2)
    lctx.fit(X, y, SIGMA, ELL, 1e-2)
    full = lctx.loo()
    tot = C.c_double()
    check(lctx._lib.gpmi_loo(lctx._h, None, None, None, C.byref(tot)))
    assert tot.value == full[3]
    check(lctx._lib.gpmi_loo(lctx._h, None, None, None, None))
    grad = lctx.loo_grad()
    dn = C.c_double()
    check(lctx._lib.gpmi_loo_grad(lctx._h, None, None, C.byref(dn)))
    assert dn.value == grad[2]
    check(lctx._lib.gpmi_loo_grad(lctx._h, None, None, None))


# ---------------------------------------------------------------------------------------------------------- gradient
@pytest.mark.parametrize("N,d,noise", CASES)
def test_gradient_against_the_mirror(lctx, N, d, noise):
    X, y, ref = _mirror(N, d, noise)
    lctx.fit(X, y, SIGMA, ELL, noise)
    _hold_gradient(lctx.loo_grad(), ref, "N=%d d=%d noise=%g" % (N, d, noise))


@pytest.mark.parametrize("nb", [128, 256, 0])
def test_gradient_mid_size_and_blocking(lctx, nb):
    """the row-block loop of the K_y^-1 D product runs more than once, with a short last block"""
    X, y, ref = _mirror(*MID)
    lctx.set_option("nb", nb)
    try:
        lctx.fit(X, y, SIGMA, ELL, MID[2])
        got = lctx.loo_grad()
        vals = lctx.loo()
    finally:
        lctx.set_option("nb", 0)
    _hold_gradient(got, ref, "N=1500 d=8 nb=%d" % nb)
    _hold_values(vals, ref, y, "N=1500 d=8 nb=%d" % nb)


# ------------------------------------------------------------------------------------------------------ lengthscales
@pytest.mark.parametrize("N,d", [(130, 2), (641, 5)])
def test_lengthscales_equal_prescaled_inputs_bit_for_bit(lctx, fresh, N, d):
    X, y = R.problem(N, d, seed=N)
    r = np.random.default_rng(3).uniform(0.5, 3.0, d) * np.sqrt(d)
    try:
        lctx.set_train(X, y)
        lctx.set_lengthscales(r)
        lctx.factorize(SIGMA, ELL, 5e-4)
        a_val, a_grad = lctx.loo(), lctx.loo_grad()
    finally:
        lctx.set_lengthscales(None)
    fresh.fit(X / r, y, SIGMA, ELL, 5e-4)
    b_val, b_grad = fresh.loo(), fresh.loo_grad()
    for p, q in zip(a_val, b_val):
        assert np.array_equal(np.asarray(p), np.asarray(q))
    assert a_grad == b_grad and np.all(np.isfinite(a_grad))


# --------------------------------------------------------------------------------------------------- reproducibility
@pytest.mark.parametrize("N,d,noise", [(641, 5, 5e-4), MID])
def test_bitwise_reproducible(lctx, N, d, noise):
    X, y, _ = _mirror(N, d, noise)
    lctx.fit(X, y, SIGMA, ELL, noise)
    v1, v2 = lctx.loo(), lctx.loo()
    for p, q in zip(v1, v2):
        assert np.array_equal(np.asarray(p), np.asarray(q))
    g1, g2 = lctx.loo_grad(), lctx.loo_grad()
    assert g1 == g2
    for p, q in zip(v1, lctx.loo()):                         # and the values after the gradient has used U's buffer
        assert np.array_equal(np.asarray(p), np.asarray(q))


# ---------------------------------------------------------------------------------------- the resident state survives
def test_resident_state_survives(lctx, fresh):
    X, y, _ = _mirror(300, 5, 5e-4)
    Xs = X[:23] + 0.01

    def state(c):
        return (c.alpha(), c.predict_resident(), c.post_chol(1e-6), c.lml_grad())

    lml = lctx.fit(X, y, SIGMA, ELL, 5e-4)
    lctx.set_test(Xs)
    lctx.predict_resident()
    before = state(lctx)
    m_before = lctx.m()
    for call in (lctx.loo, lctx.loo_grad):
        call()
        after = state(lctx)
        assert np.array_equal(before[0], after[0]) and before[3] == after[3]
        assert np.array_equal(before[1][0], after[1][0]) and np.array_equal(before[1][1], after[1][1])
        assert np.array_equal(before[2], after[2])
        assert np.array_equal(m_before, lctx.m())
    assert lctx.factorize(SIGMA, ELL, 5e-4) == lml
    # the ARD gradient shares U and Kn with loo_grad: after it, the bits of a context that never ran it
    lctx.loo_grad()
    got = lctx.lml_grad_ard()
    assert fresh.fit(X, y, SIGMA, ELL, 5e-4) == lml
    want = fresh.lml_grad_ard()
    assert np.array_equal(got[0], want[0]) and got[1:] == want[1:]


# ------------------------------------------------------------------------------------------------------- state rules
def test_state_rules(lctx):
    from gaussian_process_amd import GPContext
    X, y = R.problem(130, 2, seed=6)
    with GPContext(0) as empty:
        for call in (empty.loo, empty.loo_grad):
            with pytest.raises(ValueError):
                call()
        empty.set_train(X, y)
        for call in (empty.loo, empty.loo_grad):
            with pytest.raises(ValueError):
                call()
    lctx.laplace_fit(X, np.where(y > 0, 1.0, -1.0), 1.0, 1.0)
    for call in (lctx.loo, lctx.loo_grad):
        with pytest.raises(ValueError):
            call()
    lctx.softmax_fit(X, np.digitize(y, np.quantile(y, [1 / 3, 2 / 3])).astype(np.float64), 3, 1.0, 1.0)
    for call in (lctx.loo, lctx.loo_grad):
        with pytest.raises(ValueError):
            call()
    lctx.fit(X, y, 1.0, 1.0, 1e-2)                              # a regression fit re-enables both
    ref = LR.closed(X, y, np.ones(2), 1.0, 1.0, 1e-2)
    _hold_values(lctx.loo(), ref, y, "after the classifiers")
    _hold_gradient(lctx.loo_grad(), ref, "after the classifiers")


# ------------------------------------------------------------------------------------------------ drop-in functions
def test_drop_in_functions(lctx, fresh):
    from gaussian_process_amd import tune_hyperparms_regression as T
    X, y, ref = _mirror(130, 2, 1e-2)
    got = T.compute_loo_likelihood(X, None, y, SIGMA, ELL, noise_var=1e-2, ctx=lctx)
    assert got == lctx.loo()[3]
    assert abs(got - ref["loo"]) <= LML_RTOL * np.sum(np.abs(ref["logp"]))
    vec = np.array([0.8, 2.2])
    a = T.compute_loo_likelihood(X, None, y, 1.0, vec, noise_var=1e-2, ctx=lctx)
    b = T.compute_loo_likelihood(X / vec, None, y, 1.0, 1.0, noise_var=1e-2, ctx=fresh)
    assert a == b
    assert lctx.fit(X, y, 1.0, 1.0, 1e-2) == fresh.fit(X, y, 1.0, 1.0, 1e-2)     # no lengthscales left behind
    tot, dl, ds, dn = T.loo_and_gradient(X, y, SIGMA, ELL, noise_var=1e-2, ctx=lctx)
    assert tot == got
    _hold_gradient((dl, ds, dn), ref, "loo_and_gradient")


# ------------------------------------------------------------------------------------------------------------ tuner
def test_tuner_raises_the_criterion(lctx):
    from gaussian_process_amd import tune_hyperparms_regression as T
    X, y = R.problem(400, 3, seed=12)
    l, sigma, noise, loo, trace = T.tune_hyperparms_loo(X, y, sigma=1.0, l=3.0, noise_var=1e-2, max_iter=30, ctx=lctx)
    print("tuner: l %.3f sigma %.3f noise %.2e L_LOO %.3f -> %.3f in %d steps" % (l, sigma, noise, trace[0], loo, len(trace) - 1))
    assert np.all(np.diff(trace) >= 0)
    assert trace[-1] > trace[0] and trace[-1] == loo
    again = T.compute_loo_likelihood(X, None, y, sigma, l, noise_var=noise, ctx=lctx)
    assert abs(again - loo) <= LML_RTOL * abs(loo)
