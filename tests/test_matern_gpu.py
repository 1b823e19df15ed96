"""The Matern covariance functions nu = 1/2, 3/2, 5/2 (kinds 4, 5, 6) on the GPU against the NumPy mirror of
tests/matern_ref.py: the K build on every path, the fit and both prediction forms, lml_batch, per-dimension
lengthscales, the three gradients, the refusals of what stays squared-exponential only, and the tuner.  The bars are the
project's existing ones: K_RTOL for kernel elements (identical exp argument, exp < 1 ulp on each side), LML_RTOL, MU_ATOL
and SD_ATOL for the fit, GRAD_RTOL times each component's cancellation scale for the gradients."""
import numpy as np
import pytest

import ard_ref as R
import matern_ref as M

pytestmark = pytest.mark.gpu

K_RTOL = 7e-16        # tests/test_parity_gpu.py: 3 ulp
MU_ATOL = 1e-9
SD_ATOL = 1e-9
LML_RTOL = 1e-10
GRAD_RTOL = 1e-8      # relative to the terms that cancel
NOISE = 5e-4
SIGMA, ELL = 1.2, 1.3
NU_IDS = ["nu12", "nu32", "nu52"]


@pytest.fixture(scope="module")
def mctx():
    """a context of this module's own: the kernel kind and the lengthscales are context state"""
    from gaussian_process_amd import GPContext
    c = GPContext(0)
    yield c
    c.close()


@pytest.fixture(scope="module")
def fresh():
    """a second context that never hears of a Matern kind or of lengthscales"""
    from gaussian_process_amd import GPContext
    c = GPContext(0)
    yield c
    c.close()


# ------------------------------------------------------------------------------------------------ K through ctx.cov
def _cov_inputs(d, a):
    """130 x 257 (both edges off the 128 tile).  Plain: every t = a |x - x'| below 50.  Planted: one exactly duplicated
    pair (sq == 0 off the diagonal), one pair with 700 < t < 708 (the library-exp fallback, a normal result), a column with
    t > 760 against every row (exactly 0 on both sides); the two far points lie far from everything else, so that no
    other pair falls into the subnormal range 708 < t < 746 where a relative bar means nothing."""
    rng = np.random.default_rng(40 + d)
    A = rng.uniform(0.0, 4.0, size=(130, d))
    B = rng.uniform(0.0, 4.0, size=(257, d))
    Ap, Bp = A.copy(), B.copy()
    Bp[5] = Ap[3]
    Ap[4, 0] = 2000.0 / a
    Bp[6] = Ap[4]
    Bp[6, 0] = Ap[4, 0] + 704.0 / a
    Bp[7, 0] = -900.0 / a
    return A, B, Ap, Bp


@pytest.mark.parametrize("sigma", [1.0, 1.2], ids=["unit", "sigma1.2"])
@pytest.mark.parametrize("d", [1, 3, 8, 16, 11, 40])       # register path; 11: LDS path; 40: straight from global memory
@pytest.mark.parametrize("nu", M.NUS, ids=NU_IDS)
def test_kernel_matrix_against_the_mirror(mctx, nu, d, sigma):
    a = M.a_of(nu, ELL)
    A, B, Ap, Bp = _cov_inputs(d, a)
    t = a * np.sqrt(M.sq_cross(Ap, Bp))
    assert M.sq_cross(Ap, Bp)[3, 5] == 0.0 and 700.0 < t[4, 6] < 708.0 and t[:, 7].min() > 760.0      # what this test is about
    assert not np.any((t > 708.0) & (t < 760.0)) and a * np.sqrt(M.sq_cross(A, B)).max() < 50.0
    # plain inputs: the host proves every exp argument inside the domain and the interior tiles skip the wave-wide test
    got = mctx.cov(M.KIND[nu], A, B, sigma, ELL)
    np.testing.assert_allclose(got, M.kernel_cross(A, B, nu, sigma, ELL), rtol=K_RTOL, atol=0)
    got = mctx.cov(M.KIND[nu], Ap, Bp, sigma, ELL)
    want = M.kernel_cross(Ap, Bp, nu, sigma, ELL)
    np.testing.assert_allclose(got, want, rtol=K_RTOL, atol=0)
    assert got[3, 5] == sigma * sigma                                     # every factor is exactly 1 at sq == 0
    assert want[4, 6] > 2.3e-308 and np.all(got[:, 7] == 0.0) and np.all(want[:, 7] == 0.0)


def test_negative_lengthscale_and_refused_values(mctx):
    X, _ = R.problem(20, 2, seed=1)
    for kind in M.KIND.values():
        assert np.array_equal(mctx.cov(kind, X, X, 1.2, -1.3), mctx.cov(kind, X, X, 1.2, 1.3))
        with pytest.raises(ValueError):
            mctx.cov(kind, X, X, 1.2, 0.0)
        try:
            mctx.set_kernel(kind)
            mctx.set_train(X, np.zeros(20))
            for bad in (0.0, np.nan):
                with pytest.raises(ValueError):
                    mctx.factorize(1.2, bad, NOISE)
        finally:
            mctx.set_kernel("rbf")


def test_drop_in_kernel_function(mctx):
    from gaussian_process_amd import GP_regression as G
    X, _ = R.problem(70, 3, seed=2)
    Xs = X[:9] + 0.02
    vec = np.array([0.8, 2.2, 1.1])
    for nu in M.NUS:
        assert np.array_equal(G.matern_kernel(X, Xs, 1.2, 1.3, nu=nu), mctx.cov(M.KIND[nu], X, Xs, 1.2, 1.3))
        assert np.array_equal(G.matern_kernel(X, Xs, 1.2, vec, nu=nu), mctx.cov(M.KIND[nu], X / vec, Xs / vec, 1.2, 1.0))


# ------------------------------------------------------------------------------------------ symmetric build and fit
_fit_cache = {}


def _fit_case(nu, N, d):
    """problem, test points and the mirror's K_y, LML and prediction: computed once, left unchanged"""
    key = (nu, N, d)
    if key not in _fit_cache:
        X, y = R.problem(N, d, seed=N)
        Xs = np.random.default_rng(N + 1).uniform(0.0, 4.0, size=(37, d))
        one = np.ones(d)
        Ky = M.kernel(X, one, nu, SIGMA, ELL) + NOISE * np.eye(N)
        mu, sd = M.predict(X, y, Xs, one, nu, SIGMA, ELL, NOISE)
        _fit_cache[key] = (X, y, Xs, Ky, M.lml(X, y, one, nu, SIGMA, ELL, NOISE), mu, sd)
    return _fit_cache[key]


@pytest.mark.parametrize("N,d", [(130, 2), (641, 5)])
@pytest.mark.parametrize("nu", M.NUS, ids=NU_IDS)
def test_fit_and_prediction_against_the_mirror(mctx, nu, N, d):
    X, y, Xs, Ky, ref_lml, ref_mu, ref_sd = _fit_case(nu, N, d)
    try:
        mctx.set_kernel(M.KIND[nu])
        lml = mctx.fit(X, y, SIGMA, ELL, NOISE)
        Lf = mctx.factor()
        mu, sd = mctx.predict(Xs)
        a2, m2 = mctx.alpha(), mctx.m()
        _, var = mctx.predict_resident(want_sd=False)
        P2 = mctx.post_chol(1e-6)
        print("nu=%.1f N=%d: lml %.10f mirror %.10f  max|dmu| %.1e  max|dsd| %.1e"
              % (nu, N, lml, ref_lml, np.max(np.abs(mu - ref_mu)), np.max(np.abs(sd - ref_sd))))
        # a Cholesky factor reproduces its matrix to a few ulp of the diagonal scale (tests/test_ard_gpu.py)
        assert np.max(np.abs(Lf @ Lf.T - Ky)) <= 64 * np.finfo(np.float64).eps * np.max(np.diag(Ky))
        assert abs(lml - ref_lml) <= LML_RTOL * abs(ref_lml)
        assert np.allclose(mu, ref_mu, rtol=0, atol=MU_ATOL) and np.allclose(sd, ref_sd, rtol=0, atol=SD_ATOL)
        # the one-pass forms against the two calls, at the bars of test_fit_predict_sample_one_pass_matches_the_separate_steps
        amax = max(1.0, np.abs(a2).max())
        lml1, mu1, var1 = mctx.fit_predict(X, y, Xs, SIGMA, ELL, NOISE, want_sd=False)
        assert abs(lml1 - lml) <= 1e-11 * max(abs(lml), np.sum(m2 * m2))
        assert np.max(np.abs(mu1 - mu)) <= 1e-10 * max(1.0, amax * 1e-3) and np.max(np.abs(var1 - var)) <= 1e-11
        lml3, mu3, var3, P3 = mctx.fit_predict_sample(X, y, Xs, SIGMA, ELL, NOISE, 1e-6, want_sd=False)
        assert abs(lml3 - lml) <= 1e-11 * max(abs(lml), np.sum(m2 * m2))
        assert np.max(np.abs(mu3 - mu)) <= 1e-10 * max(1.0, amax * 1e-3) and np.max(np.abs(var3 - var)) <= 1e-11
        assert np.max(np.abs(P3 - P2)) <= 1e-6 * max(1.0, np.abs(P2).max())
        assert np.max(np.abs(P3 @ P3.T - P2 @ P2.T)) <= 1e-10
        Z = np.random.default_rng(7).standard_normal((37, 3))
        assert np.max(np.abs(mctx.post_sample(1e-6, Z) - P3 @ Z)) <= 1e-13 * max(1.0, np.abs(P3 @ Z).max()) * 37 ** 0.5
    finally:
        mctx.set_kernel("rbf")


def test_prediction_drop_in_with_a_vector_l(mctx, fresh):
    """prediction / f_prior / compute_mar_likelihood with a Matern and a d-vector l: the call on X / l with l = 1"""
    from gaussian_process_amd import GP_regression as G
    from gaussian_process_amd import tune_hyperparms_regression as T
    X, y = R.problem(130, 2, seed=13)
    Xs = X[:9] + 0.02
    vec = np.array([0.8, 2.2])
    np.random.seed(1)
    a = G.prediction(X, Xs, y, 'matern32', vec, 2, return_lml=True, ctx=mctx)
    np.random.seed(1)
    b = G.prediction(X / vec, Xs / vec, y, 'matern32', 1.0, 2, return_lml=True, ctx=fresh)
    for p, q in zip(a, b):
        assert np.array_equal(p, q)
    ref = M.lml(X, y, vec, 1.5, 1.0, 1.0, G.NOISE_VAR)
    assert abs(a[3] - ref) <= LML_RTOL * abs(ref)
    np.random.seed(2)
    fa = G.f_prior(Xs, 0.0, 'matern52', vec, 2, ctx=mctx)
    np.random.seed(2)
    fb = G.f_prior(Xs / vec, 0.0, 'matern52', 1.0, 2, ctx=fresh)
    assert np.array_equal(fa, fb)
    got = T.compute_mar_likelihood(X, None, y, 1.0, vec, ctx=mctx, kernel="matern32")
    assert got == T.compute_mar_likelihood(X / vec, None, y, 1.0, 1.0, ctx=fresh, kernel="matern32")
    assert abs(got - ref) <= LML_RTOL * abs(ref)
    # no call left lengthscales behind, and the kernel= keyword (default 'rbf') is set on every call
    assert (T.compute_mar_likelihood(X, None, y, 1.0, 1.0, noise_var=NOISE, ctx=mctx)
            == T.compute_mar_likelihood(X, None, y, 1.0, 1.0, noise_var=NOISE, ctx=fresh) == fresh.fit(X, y, 1.0, 1.0, NOISE))
    assert mctx.fit(X, y, 1.0, 1.0, NOISE) == fresh.fit(X, y, 1.0, 1.0, NOISE)


# --------------------------------------------------------------------------------------------- cross-kernel behaviour
TRIPLES = np.array([[1.3, 1.2, 5e-4], [0.9, 1.0, 1e-3], [2.0, 0.7, 5e-4], [1.1, 1.5, 2e-3], [1.6, 1.1, 5e-4]])


@pytest.mark.parametrize("nu", M.NUS, ids=NU_IDS)
def test_lml_batch_equals_single_factorisations_bit_for_bit(mctx, nu):
    X, y = R.problem(300, 3, seed=5)
    try:
        mctx.set_kernel(M.KIND[nu])
        mctx.set_train(X, y)
        lml, status = mctx.lml_batch(TRIPLES)
        assert np.all(status == 0)
        for i, (l, sigma, noise) in enumerate(TRIPLES):
            assert mctx.factorize(sigma, l, noise) == lml[i]
        ref = M.lml(X, y, np.ones(3), nu, TRIPLES[0, 1], TRIPLES[0, 0], TRIPLES[0, 2])
        assert abs(lml[0] - ref) <= LML_RTOL * abs(ref)
        from gaussian_process_amd import tune_hyperparms_regression as T
        assert np.array_equal(T.compute_mar_likelihood_batch(X, y, TRIPLES, ctx=mctx, kernel=M.KIND[nu]), lml)
    finally:
        mctx.set_kernel("rbf")


@pytest.mark.parametrize("N,d", [(130, 2), (641, 5)])
@pytest.mark.parametrize("nu", M.NUS, ids=NU_IDS)
def test_lengthscales_equal_prescaled_inputs_bit_for_bit(mctx, fresh, nu, N, d):
    """with r set, every regression path gives what it gives on X / r (divided in NumPy) with none set"""
    X, y = R.problem(N, d, seed=N)
    Xs = np.random.default_rng(N + 1).uniform(0.0, 4.0, size=(37, d))
    r = np.random.default_rng(3).uniform(0.5, 3.0, d) * np.sqrt(d)

    def run(c, A, As):
        out = {}
        c.set_train(A, y)
        out["lml"] = c.factorize(SIGMA, ELL, NOISE)
        out["alpha"] = c.alpha()
        out["lml_grad"] = c.lml_grad()
        out["loo"] = c.loo()
        out["loo_grad"] = c.loo_grad()
        c.set_test(As)
        out["one_pass"] = c.fit_predict_resident(SIGMA, ELL, NOISE, want_sd=False)
        out["post_chol"] = c.post_chol(1e-6)
        c.set_train(A, y)
        out["batch"] = c.lml_batch(TRIPLES)
        return out

    def same(p, q, name):
        if isinstance(p, tuple):
            assert len(p) == len(q)
            for i, (u, v) in enumerate(zip(p, q)):
                same(u, v, "%s[%d]" % (name, i))
        else:
            assert np.array_equal(np.asarray(p), np.asarray(q)), name

    try:
        mctx.set_kernel(M.KIND[nu])
        fresh.set_kernel(M.KIND[nu])
        mctx.set_train(X, y)
        mctx.set_lengthscales(r)
        got = run(mctx, X, Xs)
        mctx.set_lengthscales(None)
        want = run(fresh, X / r, Xs / r)
    finally:
        mctx.set_lengthscales(None)
        mctx.set_kernel("rbf")
        fresh.set_kernel("rbf")
    assert np.all(np.isfinite(got["alpha"])) and np.all(got["batch"][1] == 0)
    for k in want:
        same(got[k], want[k], k)


def test_lengthscales_stay_refused_for_the_reference_kinds(mctx):
    X, y = R.problem(130, 2, seed=6)
    try:
        mctx.set_train(X, y)
        mctx.set_lengthscales([0.8, 1.7])
        mctx.set_kernel("lin", 0.5)
        with pytest.raises(ValueError, match="lengthscales"):
            mctx.factorize(1.0, 1.0, NOISE)
        mctx.set_kernel("matern32")
        assert np.isfinite(mctx.factorize(1.0, 1.0, NOISE))
    finally:
        mctx.set_lengthscales(None)
        mctx.set_kernel("rbf")


def test_no_stale_kernel_state(mctx, fresh):
    """after set_kernel('matern32') and back, a fit is a fresh context's bit for bit -- and nothing fitted survives the switch"""
    X, y = R.problem(641, 5, seed=2)
    Xs = X[:20] + 0.01
    mctx.set_kernel("matern32")
    mctx.fit(X, y, SIGMA, ELL, NOISE)
    mctx.set_kernel("rbf")
    with pytest.raises(ValueError):
        mctx.alpha()                                     # the factor belonged to the Matern covariance
    a = (mctx.fit(X, y, SIGMA, ELL, NOISE), mctx.lml_grad(), mctx.alpha(), mctx.predict(Xs))
    b = (fresh.fit(X, y, SIGMA, ELL, NOISE), fresh.lml_grad(), fresh.alpha(), fresh.predict(Xs))
    assert a[0] == b[0] and a[1] == b[1] and np.array_equal(a[2], b[2])
    assert np.array_equal(a[3][0], b[3][0]) and np.array_equal(a[3][1], b[3][1])
    assert np.array_equal(mctx.rbf(X[:130], Xs, SIGMA, ELL), fresh.rbf(X[:130], Xs, SIGMA, ELL))


# ---------------------------------------------------------------------------------------------------------- gradients
_grad_cache = {}


def _grad_case(nu, N, d, dup=False):
    """one mirror evaluation per case, shared by the tests below and left unchanged"""
    key = (nu, N, d, dup)
    if key not in _grad_cache:
        X, y = R.problem(N, d, seed=100 + d)
        if dup:
            X, y = M.duplicate_rows(X, y, [(7, 30), (101, 2)])
        r = np.random.default_rng(7 + d).uniform(0.5, 3.0, d) * np.sqrt(d)
        _grad_cache[key] = (X, y, r, M.lml_and_grad(X, y, r, nu, SIGMA, ELL, NOISE),
                            M.loo_closed(X, y, r, nu, SIGMA, ELL, NOISE))
    return _grad_cache[key]


def _hold_gradients(c, ref, loo, r, tag):
    d_r, d_l, d_s, d_n = c.lml_grad_ard()
    dl2, ds2 = c.lml_grad()
    total = c.loo()[3]
    gl, gs, gn = c.loo_grad()
    err = np.abs(d_r - ref["g_r"]) / ref["s_r"]
    print("%s cond %.1e: d_r %.1e l %.1e sigma %.1e noise %.1e | lml_grad l %.1e sigma %.1e | loo l %.1e sigma %.1e noise %.1e"
          % (tag, ref["cond"], err.max(), abs(d_l - ref["g_l"]) / ref["s_l"], abs(d_s - ref["g_sigma"]) / ref["s_sigma"],
             abs(d_n - ref["g_noise"]) / ref["s_noise"], abs(dl2 - ref["g_l"]) / ref["s_l"],
             abs(ds2 - ref["g_sigma"]) / ref["s_sigma"], abs(gl - loo["g_l"]) / loo["s_l"],
             abs(gs - loo["g_sigma"]) / loo["s_sigma"], abs(gn - loo["g_noise"]) / loo["s_noise"]))
    assert np.all(np.isfinite(d_r)) and np.all(np.isfinite([d_l, d_s, d_n, dl2, ds2, gl, gs, gn]))
    assert np.all(err <= GRAD_RTOL), (tag, int(err.argmax()), float(err.max()))
    assert abs(d_l - ref["g_l"]) <= GRAD_RTOL * ref["s_l"] and abs(dl2 - ref["g_l"]) <= GRAD_RTOL * ref["s_l"]
    assert abs(d_s - ref["g_sigma"]) <= GRAD_RTOL * ref["s_sigma"] and abs(ds2 - ref["g_sigma"]) <= GRAD_RTOL * ref["s_sigma"]
    assert abs(d_n - ref["g_noise"]) <= GRAD_RTOL * ref["s_noise"]
    assert abs(float(r @ d_r) - ELL * d_l) <= GRAD_RTOL * ELL * ref["s_l"]             # the Euler identity
    assert abs(total - loo["loo"]) <= LML_RTOL * abs(loo["loo"])
    assert abs(gl - loo["g_l"]) <= GRAD_RTOL * loo["s_l"]
    assert abs(gs - loo["g_sigma"]) <= GRAD_RTOL * loo["s_sigma"]
    assert abs(gn - loo["g_noise"]) <= GRAD_RTOL * loo["s_noise"]
    # two runs give the same bits
    again = c.lml_grad_ard()
    assert np.array_equal(again[0], d_r) and again[1:] == (d_l, d_s, d_n)
    assert c.lml_grad() == (dl2, ds2) and c.loo_grad() == (gl, gs, gn)


@pytest.mark.parametrize("N,d", [(130, 2), (300, 5), (130, 33), (300, 2)])      # d = 33: a second launch of the ARD kernel
@pytest.mark.parametrize("nu", M.NUS, ids=NU_IDS)
def test_gradients_against_the_mirror(mctx, nu, N, d):
    X, y, r, ref, loo = _grad_case(nu, N, d)
    try:
        mctx.set_kernel(M.KIND[nu])
        mctx.set_train(X, y)
        mctx.set_lengthscales(r)
        lml = mctx.factorize(SIGMA, ELL, NOISE)
        assert abs(lml - ref["lml"]) <= LML_RTOL * abs(ref["lml"])
        _hold_gradients(mctx, ref, loo, r, "nu=%.1f N=%d d=%d" % (nu, N, d))
    finally:
        mctx.set_lengthscales(None)
        mctx.set_kernel("rbf")


def test_duplicated_rows_nu12(mctx):
    """H_1/2 = e^-t / t is singular at t = 0: two exactly duplicated training rows give finite gradients that match"""
    X, y, r, ref, loo = _grad_case(0.5, 130, 2, dup=True)
    assert np.sum(M.sq_cross(X / r, X / r) == 0.0) == 130 + 4
    try:
        mctx.set_kernel("matern12")
        mctx.set_train(X, y)
        mctx.set_lengthscales(r)
        lml = mctx.factorize(SIGMA, ELL, NOISE)
        assert abs(lml - ref["lml"]) <= LML_RTOL * abs(ref["lml"])
        _hold_gradients(mctx, ref, loo, r, "nu=0.5 N=130 d=2 duplicated rows")
    finally:
        mctx.set_lengthscales(None)
        mctx.set_kernel("rbf")


def test_gradient_drop_ins(mctx):
    from gaussian_process_amd import tune_hyperparms_regression as T
    X, y, r, ref, loo = _grad_case(1.5, 130, 2)
    try:
        lml, d_ls, d_sigma, d_noise = T.lml_and_gradient_ard(X, y, SIGMA, ELL * r, noise_var=NOISE, ctx=mctx, kernel="matern32")
        assert abs(lml - ref["lml"]) <= LML_RTOL * abs(ref["lml"])
        assert np.all(np.abs(d_ls - ref["g_r"] / ELL) <= GRAD_RTOL * ref["s_r"] / ELL)          # absolute lengthscales l r_k
        assert abs(d_sigma - ref["g_sigma"]) <= GRAD_RTOL * ref["s_sigma"]
        mctx.set_lengthscales(None)
        iso = M.lml_and_grad(X, y, np.ones(2), 2.5, SIGMA, ELL, NOISE)
        lml, dl, ds = T.lml_and_gradient(X, y, SIGMA, ELL, noise_var=NOISE, ctx=mctx, kernel="matern52")
        assert abs(lml - iso["lml"]) <= LML_RTOL * abs(iso["lml"])
        assert abs(dl - iso["g_l"]) <= GRAD_RTOL * iso["s_l"] and abs(ds - iso["g_sigma"]) <= GRAD_RTOL * iso["s_sigma"]
        lc = M.loo_closed(X, y, np.ones(2), 2.5, SIGMA, ELL, NOISE)
        total, gl, gs, gn = T.loo_and_gradient(X, y, SIGMA, ELL, noise_var=NOISE, ctx=mctx, kernel="matern52")
        assert abs(total - lc["loo"]) <= LML_RTOL * abs(lc["loo"]) and abs(gl - lc["g_l"]) <= GRAD_RTOL * lc["s_l"]
        assert T.compute_loo_likelihood(X, None, y, SIGMA, ELL, noise_var=NOISE, ctx=mctx, kernel="matern52") == total
    finally:
        mctx.set_lengthscales(None)
        mctx.set_kernel("rbf")


# ---------------------------------------------------------------------------------------------------------- refusals
def test_what_stays_squared_exponential_refuses_the_matern_kinds(mctx, fresh):
    X, y = R.problem(130, 2, seed=6)
    Z = X[::10].copy()
    labels = np.where(y > np.median(y), 1.0, -1.0)
    classes = np.digitize(y, np.quantile(y, [1 / 3, 2 / 3])).astype(np.float64)
    want = fresh.fit(X, y, SIGMA, ELL, NOISE)
    Kinv = np.eye(130)
    for kind in M.KIND.values():
        try:
            mctx.set_kernel(kind)
            with pytest.raises(ValueError, match="squared-exponential"):
                mctx.sparse_fit(X, y, Z, SIGMA, ELL, NOISE)
            with pytest.raises(ValueError, match="squared-exponential"):
                mctx.laplace_fit(X, labels, SIGMA, ELL)
            with pytest.raises(ValueError, match="squared-exponential"):
                mctx.softmax_fit(X, classes, 3, SIGMA, ELL)
            with pytest.raises(ValueError, match="squared-exponential"):
                mctx.grad_trace(X, X, SIGMA, ELL, y, Kinv)
            assert np.isfinite(mctx.fit(X, y, SIGMA, ELL, NOISE))          # the context works afterwards
            assert np.all(np.isfinite(mctx.loo()[0]))
        finally:
            mctx.set_kernel("rbf")
        assert mctx.fit(X, y, SIGMA, ELL, NOISE) == want


# ------------------------------------------------------------------------------------------------------------- tuner
def test_tuner_finds_the_relevant_dimension(mctx):
    from gaussian_process_amd import tune_hyperparms_regression as T
    X, y = R.problem(200, 3, seed=12, relevant=1)        # y depends on dimension 0 only
    try:
        ls, sigma, noise, lml, trace = T.tune_hyperparms_ard(X, y, sigma=1.0, lengthscales=np.ones(3), noise_var=NOISE,
                                                             max_iter=30, ctx=mctx, kernel="matern52")
        print("tuner: lengthscales %s sigma %.3f noise %.2e lml %.3f -> %.3f in %d steps"
              % (ls, sigma, noise, trace[0], lml, len(trace) - 1))
        assert lml >= trace[0] and trace[-1] == lml
        assert ls[1] > ls[0] and ls[2] > ls[0]
        ref = M.lml(X, y, ls, 2.5, sigma, 1.0, noise)
        assert abs(lml - ref) <= LML_RTOL * abs(ref)      # the factor resident is the Matern one at the point reached
        l, s2, n2, total, tr = T.tune_hyperparms_loo(X, y, sigma=1.0, l=1.0, noise_var=NOISE, max_iter=5, ctx=mctx, kernel="matern32")
        assert total >= tr[0]
    finally:
        mctx.set_lengthscales(None)
        mctx.set_kernel("rbf")
