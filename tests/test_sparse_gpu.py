"""Sparse GP regression with inducing points on the GPU (gpmi_sparse_fit, gpmi_sparse_predict_resident) against the
NumPy mirror of tests/sgpr_ref.py.  The bars are the project's existing ones: LML_RTOL of the sum of the absolute
terms for the value (the scale comes from the mirror), 1e-9 max(1, max|y|) for the mean, 1e-10 sigma^2 for the
variance and 1e-8 max|c| for c.  The shapes are the smallest at which the kernels can go wrong, not the workload's."""
import numpy as np
import pytest

import ard_ref as R
import sgpr_ref as S

pytestmark = pytest.mark.gpu

LML_RTOL = 1e-10      # tests/test_parity_gpu.py
METHODS = ["vfe", "fitc"]
N_TEST = 64


@pytest.fixture(scope="module")
def sctx():
    """a context of this module's own: lengthscales and options are context state"""
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


def _problem(N, d, m):
    X, y = R.problem(N, d, seed=100 + d)
    Xs = np.random.default_rng(7).uniform(0.0, 4.0, size=(N_TEST, d))
    return X, y, S.inducing(X, m), Xs


def _mirror(N, d, m, noise, method):
    """one mirror evaluation per input, shared by the tests below and left unchanged"""
    key = (N, d, m, noise, method)
    if key not in _cache:
        X, y, Z, Xs = _problem(N, d, m)
        _cache[key] = (X, y, Z, Xs, S.fit(X, y, Z, S.SIGMA, S.ELL, noise, method=method, Xs=Xs))
    return _cache[key]


def _hold(value, state, pred, ref, y, tag):
    """value, (c, q), (mean, var) of the device against the mirror"""
    e_val = abs(value - ref["value"]) / ref["scale"]
    print("%s cond %.2e: value %.2e" % (tag, ref["cond"], e_val), end="")
    assert e_val <= LML_RTOL
    if state is not None:
        c, q = state
        e_c = np.max(np.abs(c - ref["c"])) / np.max(np.abs(ref["c"]))
        e_q = np.max(np.abs(q - ref["q"])) / S.SIGMA ** 2
        print(" c %.2e q %.2e" % (e_c, e_q), end="")
        assert e_c <= 1e-8
        assert e_q <= 1e-10
    if pred is not None:
        mu, var = pred
        e_mu = np.max(np.abs(mu - ref["mean"]))
        e_var = np.max(np.abs(var - ref["var"]))
        print(" mean %.2e var %.2e" % (e_mu, e_var), end="")
        assert e_mu <= 1e-9 * max(1.0, np.max(np.abs(y)))
        assert e_var <= 1e-10 * S.SIGMA ** 2
    print()


def _run(ctx, X, y, Z, Xs, noise, method, **kw):
    value = ctx.sparse_fit(X, y, Z, S.SIGMA, S.ELL, noise, method=method, **kw)
    return value, ctx.sparse_state(), ctx.sparse_predict(Xs, want_sd=False)


# ------------------------------------------------------------------------------------------------------------ values
@pytest.mark.parametrize("method", METHODS)
@pytest.mark.parametrize("N,d,m,noise", S.CASES + [S.MID])
def test_against_the_mirror(sctx, N, d, m, noise, method):
    X, y, Z, Xs, ref = _mirror(N, d, m, noise, method)
    value, state, pred = _run(sctx, X, y, Z, Xs, noise, method)
    _hold(value, state, pred, ref, y, "N=%d d=%d m=%d %s" % (N, d, m, method))
    mu, sd = sctx.sparse_predict(Xs)                         # the standard deviation is the root of that variance
    assert np.array_equal(mu, pred[0]) and np.array_equal(sd, np.sqrt(pred[1]))


# ------------------------------------------------------------------------------------------------------------- slabs
@pytest.mark.parametrize("method", METHODS)
@pytest.mark.parametrize("slab", [128, 256, 0])
def test_slabs(sctx, slab, method):
    """N = 641 (padded: 768 rows), m = 130: six slabs of 128, three of 256, or one; the last slab of each is partial"""
    N, d, m, noise = 641, 5, 130, 5e-4
    X, y, Z, Xs, ref = _mirror(N, d, m, noise, method)
    sctx.set_option("sparse_slab", slab)
    try:
        a = _run(sctx, X, y, Z, Xs, noise, method)
        b = _run(sctx, X, y, Z, Xs, noise, method)
    finally:
        sctx.set_option("sparse_slab", 0)
    _hold(a[0], a[1], a[2], ref, y, "slab=%d %s" % (slab, method))
    assert a[0] == b[0] and np.array_equal(a[1][0], b[1][0])          # the value and c, bit for bit
    assert np.array_equal(a[1][1], b[1][1]) and np.array_equal(a[2][0], b[2][0]) and np.array_equal(a[2][1], b[2][1])


def test_slab_option_is_checked(sctx):
    with pytest.raises(ValueError, match="sparse_slab"):
        sctx.set_option("sparse_slab", -1)


# ------------------------------------------------------------------------------------------------------------- split
@pytest.mark.parametrize("method", METHODS)
def test_the_gram_kernel_splits_the_slab(sctx, method):
    """The Gram kernel cuts a slab into chunks of whole 128-row units, as many as bring tiles x splits to 1024 (sparse.hip:
    gram_plan).  m = 40 is one lower tile, so every unit becomes a split of its own: N = 129 (256 padded rows) is the
    smallest N at which the launch has two splits -- the second holds one real row and 127 rows of padding.  The larger
    case (N = 1500, m = 384: 12 units, 21 tiles) has twelve splits of one unit."""
    for N, d, m, noise in [(129, 2, 40, 1e-2), S.MID]:
        if N == 129:
            X, y = R.problem(N, d, seed=100 + d)
            Z, Xs = S.inducing(X, m), X[:N_TEST] + 0.03
            ref = S.fit(X, y, Z, S.SIGMA, S.ELL, noise, method=method, Xs=Xs)
        else:
            X, y, Z, Xs, ref = _mirror(N, d, m, noise, method)
        a = _run(sctx, X, y, Z, Xs, noise, method)
        b = _run(sctx, X, y, Z, Xs, noise, method)
        _hold(a[0], a[1], a[2], ref, y, "split N=%d m=%d %s" % (N, m, method))
        assert a[0] == b[0] and np.array_equal(a[1][0], b[1][0]) and np.array_equal(a[1][1], b[1][1])


# ------------------------------------------------------------------------------------------------------ lengthscales
@pytest.mark.parametrize("method", METHODS)
@pytest.mark.parametrize("N,d,m", [(130, 2, 40), (641, 5, 130)])
def test_lengthscales_equal_prescaled_inputs_bit_for_bit(sctx, fresh, N, d, m, method):
    X, y, Z, Xs = _problem(N, d, m)
    r = np.random.default_rng(3).uniform(0.5, 3.0, d) * np.sqrt(d)
    try:
        va = sctx.sparse_fit(X, y, Z, S.SIGMA, S.ELL, 5e-3, method=method, lengthscales=r)
        sa, pa = sctx.sparse_state(), sctx.sparse_predict(Xs, want_sd=False)
    finally:
        sctx.set_lengthscales(None)
    vb = fresh.sparse_fit(X / r, y, Z / r, S.SIGMA, S.ELL, 5e-3, method=method)
    sb, pb = fresh.sparse_state(), fresh.sparse_predict(Xs / r, want_sd=False)
    assert va == vb and np.isfinite(va)
    for p, q in zip(sa + pa, sb + pb):
        assert np.array_equal(p, q)


def test_drop_in_function_with_a_vector_lengthscale(sctx, fresh):
    from gaussian_process_amd import sparse_prediction
    X, y, Z, Xs = _problem(130, 2, 40)
    vec = np.array([0.8, 2.2])
    mu, sd, val = sparse_prediction(X, Xs, y, Z, 1.0, vec, 1e-2, ctx=sctx)
    mu2, sd2, val2 = sparse_prediction(X / vec, Xs / vec, y, Z / vec, 1.0, 1.0, 1e-2, ctx=fresh)
    assert val == val2 and np.array_equal(mu, mu2) and np.array_equal(sd, sd2)
    ref = S.fit(X / vec, y, Z / vec, 1.0, 1.0, 1e-2, Xs=Xs / vec)
    _hold(val, None, (mu, sd ** 2), ref, y, "sparse_prediction")
    assert sctx.fit(X, y, 1.0, 1.0, 1e-2) == fresh.fit(X, y, 1.0, 1.0, 1e-2)     # no lengthscales left behind


# ------------------------------------------------------------------------------------------------------------- Z = X
def test_every_point_inducing(sctx):
    """Z = X at N = 256: the bound stays below the exact LML, and the sparse mean meets the exact one as closely as the
    mirror says the two differ on this input (Q_ff differs from K by O(jitter)), times 10"""
    N, d, noise = 256, 5, 5e-4
    X, y = R.problem(N, d, seed=100 + d)
    Xs = np.random.default_rng(7).uniform(0.0, 4.0, size=(N_TEST, d))
    ref = S.fit(X, y, X, S.SIGMA, S.ELL, noise, Xs=Xs)
    K = S.kernel(X, X, S.SIGMA, S.ELL) + noise * np.eye(N)
    exact_mean = S.kernel(Xs, X, S.SIGMA, S.ELL) @ np.linalg.solve(K, y)
    bound = 10 * np.max(np.abs(ref["mean"] - exact_mean))
    value = sctx.sparse_fit(X, y, X, S.SIGMA, S.ELL, noise)
    mu_sparse, _ = sctx.sparse_predict(Xs)
    lml = sctx.fit(X, y, S.SIGMA, S.ELL, noise)
    mu_exact, _ = sctx.predict(Xs)
    print("Z = X: bound %.6f exact %.6f; |sparse - exact| mean %.2e (mirror's difference x 10: %.2e)"
          % (value, lml, np.max(np.abs(mu_sparse - mu_exact)), bound))
    assert value <= lml
    assert np.max(np.abs(mu_sparse - mu_exact)) <= bound


# ------------------------------------------------------------------------------------------------------------- state
def test_state_rules(sctx):
    from gaussian_process_amd import GPContext
    X, y, Z, Xs = _problem(130, 2, 40)
    sctx.fit(X, y, S.SIGMA, S.ELL, 1e-2)
    sctx.sparse_fit(X, y, Z, S.SIGMA, S.ELL, 1e-2)
    sctx.set_test(Xs)
    for call, text in ((sctx.predict_resident, "no factorisation resident"), (sctx.alpha, "no factorisation resident"),
                       (sctx.lml_grad, "factorisation resident"), (sctx.lml_grad_ard, "factorisation resident"),
                       (sctx.loo, "factorisation resident"), (sctx.loo_grad, "factorisation resident"),
                       (lambda: sctx.post_chol(1e-6), "run gpmi_predict first")):
        with pytest.raises(ValueError, match=text):
            call()
    assert len(sctx.sparse_predict(Xs)) == 2                       # the refusals left the sparse fit alone
    sctx.fit(X, y, S.SIGMA, S.ELL, 1e-2)                           # a regression fit drops it
    with pytest.raises(ValueError, match="no sparse fit resident"):
        sctx.sparse_predict(Xs)
    with pytest.raises(ValueError, match="no sparse fit resident"):
        sctx.sparse_state()
    assert len(sctx.predict(Xs)) == 2
    sctx.sparse_fit(X, y, Z, S.SIGMA, S.ELL, 1e-2)
    sctx.set_lengthscales(np.array([1.5, 0.7]))                    # ... and so do new lengthscales
    try:
        with pytest.raises(ValueError, match="no sparse fit resident"):
            sctx.sparse_predict(Xs)
    finally:
        sctx.set_lengthscales(None)
    sctx.sparse_fit(X, y, Z, S.SIGMA, S.ELL, 1e-2)
    sctx.laplace_fit(X, np.where(y > 0, 1.0, -1.0), 1.0, 1.0)      # ... and a classifier's fit
    with pytest.raises(ValueError, match="no sparse fit resident"):
        sctx.sparse_predict(Xs)
    # a stale test set of another d: the new training set dropped it, and the shim refuses the wrong width
    sctx.set_test(Xs)
    X5, y5, Z5, Xs5 = _problem(300, 5, 64)
    sctx.sparse_fit(X5, y5, Z5, S.SIGMA, S.ELL, 5e-4)
    from gaussian_process_amd._lib import check
    mu = np.empty(N_TEST)
    with pytest.raises(ValueError, match="no test set"):
        check(sctx._lib.gpmi_sparse_predict_resident(sctx._h, mu.ctypes.data_as(sctx._lib.gpmi_sparse_predict_resident.argtypes[1]), None, 0))
    with pytest.raises(ValueError, match="d=2"):
        sctx.sparse_predict(Xs)
    with GPContext(0) as empty:
        with pytest.raises(ValueError, match="no training set"):
            check(empty._lib.gpmi_sparse_fit(empty._h, Z.ctypes.data_as(empty._lib.gpmi_sparse_fit.argtypes[1]), 40, 1.0, 1.0,
                                             1e-2, 1e-6, 0, None, None))
    try:                                                           # kernel kind 0 only
        sctx.set_kernel("lin", 0.5)
        with pytest.raises(ValueError, match="squared-exponential"):
            sctx.sparse_fit(X, y, Z, S.SIGMA, S.ELL, 1e-2)
    finally:
        sctx.set_kernel("rbf")


# ---------------------------------------------------------------------------------------------------------- failures
def test_failures_are_reported(sctx):
    import ctypes as C
    from gaussian_process_amd import _lib
    X, y, Z, Xs = _problem(130, 2, 40)
    Zd = Z.copy()
    Zd[1] = Zd[0]                     # with sigma = 1 the second copy's pivot is 1 - 1 * 1 = 0 exactly
    with pytest.raises(np.linalg.LinAlgError) as info:
        sctx.sparse_fit(X, y, Zd, 1.0, S.ELL, 1e-2, jitter=0.0)
    assert info.value.bad_pivot == 2
    with pytest.raises(ValueError, match="no sparse fit resident"):
        sctx.sparse_predict(Xs)
    for kw, text in (({"noise_var": 0.0}, "noise_var"), ({"noise_var": -1.0}, "noise_var"), ({"jitter": -1e-6}, "jitter")):
        args = {"noise_var": 1e-2, "jitter": 1e-6}
        args.update(kw)
        with pytest.raises(ValueError, match=text):
            sctx.sparse_fit(X, y, Z, S.SIGMA, S.ELL, args["noise_var"], jitter=args["jitter"])
    sctx.set_train(X, y)
    zp = Z.ctypes.data_as(_lib._dp)
    for m, method in ((0, 0), (131, 0), (40, 2)):
        st = sctx._lib.gpmi_sparse_fit(sctx._h, zp, m, 1.0, 1.0, 1e-2, 1e-6, method, None, None)
        assert st == _lib.GPMI_ERR_BAD_ARG, (m, method)
    val = C.c_double()
    assert sctx._lib.gpmi_sparse_fit(sctx._h, zp, 40, 1.0, 1.0, 1e-2, 1e-6, 1, C.byref(val), None) == _lib.GPMI_OK
    assert np.isfinite(val.value)


# -------------------------------------------------------------------------------------------------------- prediction
@pytest.mark.parametrize("method", METHODS)
def test_chunked_prediction(sctx, method):
    """n = 1000 test points (1024 padded rows) on a fit whose slab workspace has 256 rows: four chunks"""
    N, d, m, noise = 130, 2, 40, 1e-2
    X, y, Z, _ = _problem(N, d, m)
    Xs = np.random.default_rng(11).uniform(0.0, 4.0, size=(1000, d))
    ref = S.fit(X, y, Z, S.SIGMA, S.ELL, noise, method=method, Xs=Xs)
    value = sctx.sparse_fit(X, y, Z, S.SIGMA, S.ELL, noise, method=method)
    _hold(value, None, sctx.sparse_predict(Xs, want_sd=False), ref, y, "n=1000 %s" % method)


def test_timers(sctx):
    X, y, Z, _ = _problem(300, 5, 64)
    sctx.sparse_fit(X, y, Z, S.SIGMA, S.ELL, 5e-4)
    tm = sctx.timers()
    assert tm["sparse"] > 0 and tm["sparse"] >= tm["postchol"] > 0
