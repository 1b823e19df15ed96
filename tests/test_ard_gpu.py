"""Per-dimension lengthscales (ARD) on the GPU: gpmi_set_lengthscales through every path that builds a covariance, and
gpmi_lml_grad_ard against the NumPy mirror of tests/ard_ref.py.  The bars are the project's existing ones: LML_RTOL for
the LML, GRAD_RTOL times each component's cancellation scale for the gradient."""
import numpy as np
import pytest

import ard_ref as R

pytestmark = pytest.mark.gpu

LML_RTOL = 1e-10      # tests/test_parity_gpu.py
GRAD_RTOL = 1e-8      # tests/test_parity_gpu.py: relative to the two terms the trace cancels
NOISE = 5e-4


@pytest.fixture(scope="module")
def actx():
    """a context of this module's own: lengthscales are context state, and the session's shared one stays isotropic"""
    from gaussian_process_amd import GPContext
    c = GPContext(0)
    yield c
    c.close()


@pytest.fixture(scope="module")
def fresh():
    """a second context that never hears of lengthscales"""
    from gaussian_process_amd import GPContext
    c = GPContext(0)
    yield c
    c.close()


def _r(d, seed=3):
    return np.random.default_rng(seed).uniform(0.5, 3.0, d) * np.sqrt(d)


# ------------------------------------------------------------------------------------ equivalence by pre-scaling
@pytest.mark.parametrize("N,d", [(130, 2), (641, 5)])
def test_lengthscales_equal_prescaled_inputs_bit_for_bit(actx, fresh, N, d):
    """with r set, every path gives what it gives on X / r (divided in NumPy) with none set"""
    X, y = R.problem(N, d, seed=N)
    Xs = np.random.default_rng(N + 1).uniform(0.0, 4.0, size=(37, d))
    r = _r(d)
    Z, Zs = X / r, Xs / r
    sigma, l = 1.2, 1.3
    triples = np.array([[1.3, 1.2, 5e-4], [0.9, 1.0, 1e-3], [2.0, 0.7, 5e-4], [1.1, 1.5, 2e-3], [1.6, 1.1, 5e-4]])
    labels = np.where(y > np.median(y), 1.0, -1.0)
    classes = np.digitize(y, np.quantile(y, [1 / 3, 2 / 3])).astype(np.float64)
    normals = np.random.default_rng(5).standard_normal((16, 3))

    def run(c, A, As):
        out = {}
        c.set_train(A, y)
        out["lml"] = c.factorize(sigma, l, NOISE)
        out["alpha"] = c.alpha()
        c.set_test(As)
        out["one_pass"] = c.fit_predict_resident(sigma, l, NOISE, want_sd=False)
        out["post_chol"] = c.post_chol(1e-6)
        c.set_train(A, y)
        out["batch"] = c.lml_batch(triples)
        out["laplace"] = c.laplace_fit(A, labels, sigma, l)[:3]
        out["laplace_predict"] = c.laplace_predict(As)
        out["softmax"] = c.softmax_fit(A, classes, 3, sigma, l)[:3]
        out["softmax_predict"] = c.softmax_predict(As, normals)
        return out

    try:
        actx.set_train(X, y)
        actx.set_lengthscales(r)
        got = run(actx, X, Xs)
    finally:
        actx.set_lengthscales(None)
    want = run(fresh, Z, Zs)

    def same(a, b, name):
        if isinstance(a, tuple):
            assert len(a) == len(b)
            for i, (p, q) in enumerate(zip(a, b)):
                same(p, q, "%s[%d]" % (name, i))
        else:
            assert np.array_equal(np.asarray(a), np.asarray(b)), name

    assert np.all(np.isfinite(got["alpha"])) and np.all(got["batch"][1] == 0)
    for k in want:
        same(got[k], want[k], k)


# ------------------------------------------------------------------------------------------- K against the mirror
def test_kernel_matrix_against_the_mirror(actx):
    """the LML at N = 130 and the factor of a 64-point set: L L^T is K + noise I of the mirror"""
    X, y = R.problem(64, 3, seed=64)
    r = np.array([0.7, 2.5, 1.4])
    sigma, l = 1.2, 1.3
    try:
        actx.set_train(X, y)
        actx.set_lengthscales(r)
        lml = actx.factorize(sigma, l, NOISE)
        Lf = actx.factor()
    finally:
        actx.set_lengthscales(None)
    Ky = R.kernel(X, r, sigma, l) + NOISE * np.eye(64)
    ref = R.lml(X, y, r, sigma, l, NOISE)
    assert abs(lml - ref) <= LML_RTOL * abs(ref), (lml, ref)
    # a Cholesky factor reproduces its matrix to a few ulp of the diagonal scale, whatever the conditioning
    assert np.max(np.abs(Lf @ Lf.T - Ky)) <= 64 * np.finfo(np.float64).eps * np.max(np.diag(Ky))


# ----------------------------------------------------------------------------------------------- box under ARD
def test_box_bounds_the_scaled_inputs(actx, fresh):
    """r = (1, 1e-3) stretches dimension 1 a thousandfold: exp arguments down to -4.6e5, most of K exactly 0.  A box
    that still bounded x would let the K build skip its exp-domain test and produce garbage."""
    N, d = 130, 2
    rng = np.random.default_rng(11)
    X = rng.uniform(0.0, 1.0, size=(N, d))
    y = np.sin(3 * X[:, 0]) + 0.05 * rng.standard_normal(N)
    Xs = rng.uniform(0.0, 1.0, size=(20, d))
    r = np.array([1.0, 1e-3])
    sq = ((X[:, None, :] / r - X[None, :, :] / r) ** 2).sum(-1)
    Kref = np.exp(-.5 * sq)
    off = ~np.eye(N, dtype=bool)
    assert (-.5 * sq).min() < -4e5 and np.mean(Kref[off] == 0.0) > 0.9          # what this test is about
    ref = R.lml(X, y, r, 1.0, 1.0, NOISE)
    iso = fresh.fit_predict(X, y, Xs, 1.0, 1.0, NOISE)
    try:
        actx.set_train(X, y)
        actx.set_test(Xs)
        actx.set_lengthscales(r)
        lml, mu, sd = actx.fit_predict_resident(1.0, 1.0, NOISE)
        print("box test: lml %.12f mirror %.12f" % (lml, ref))
        assert abs(lml - ref) <= LML_RTOL * abs(ref), (lml, ref)
        assert np.all(np.isfinite(mu)) and np.all(np.isfinite(sd))
        actx.set_lengthscales(None)
        back = actx.fit_predict_resident(1.0, 1.0, NOISE)
    finally:
        actx.set_lengthscales(None)
    assert back[0] == iso[0] and np.array_equal(back[1], iso[1]) and np.array_equal(back[2], iso[2])


# ------------------------------------------------------------------------------------ gradient against the mirror
_mirror_cache = {}


def _mirror(N, d, sigma=1.2, l=1.3):
    """one mirror evaluation per shape, shared by the tests below and left unchanged"""
    key = (N, d, sigma, l)
    if key not in _mirror_cache:
        X, y = R.problem(N, d, seed=100 + d)
        r = np.random.default_rng(7 + d).uniform(0.5, 3.0, d) * np.sqrt(d)
        _mirror_cache[key] = (X, y, r, R.lml_and_grad(X, y, r, sigma, l, NOISE))
    return _mirror_cache[key]


def _hold_gradient(got, ref, tag):
    d_r, d_l, d_s, d_n = got
    err = np.abs(d_r - ref["g_r"]) / ref["s_r"]
    print("%s: worst d_r error / scale %.2e, l %.2e, sigma %.2e, noise %.2e" % (
        tag, err.max(), abs(d_l - ref["g_l"]) / ref["s_l"], abs(d_s - ref["g_sigma"]) / ref["s_sigma"],
        abs(d_n - ref["g_noise"]) / ref["s_noise"]))
    assert np.all(err <= GRAD_RTOL), (tag, int(err.argmax()), float(err.max()))
    assert abs(d_l - ref["g_l"]) <= GRAD_RTOL * ref["s_l"]
    assert abs(d_s - ref["g_sigma"]) <= GRAD_RTOL * ref["s_sigma"]
    assert abs(d_n - ref["g_noise"]) <= GRAD_RTOL * ref["s_noise"]       # .5 alpha^T alpha + .5 tr K_y^-1


@pytest.mark.parametrize("N,d", [(130, 2), (300, 3), (257, 33), (200, 1), (200, 7), (200, 13), (200, 20)])
def test_gradient_against_the_mirror(actx, N, d):
    """every chunk width (4, 8, 16, 32), the two-launch d > 32 rule, d = 1, and sizes that are no multiple of the tile"""
    X, y, r, ref = _mirror(N, d)
    try:
        actx.set_train(X, y)
        actx.set_lengthscales(r)
        lml = actx.factorize(1.2, 1.3, NOISE)
        got = actx.lml_grad_ard()
    finally:
        actx.set_lengthscales(None)
    assert abs(lml - ref["lml"]) <= LML_RTOL * abs(ref["lml"])
    _hold_gradient(got, ref, "N=%d d=%d" % (N, d))


@pytest.mark.parametrize("nb", [128, 256, 0])
def test_gradient_mid_size_and_blocking(actx, nb):
    X, y, r, ref = _mirror(1500, 8)
    actx.set_option("nb", nb)
    try:
        actx.set_train(X, y)
        actx.set_lengthscales(r)
        actx.factorize(1.2, 1.3, NOISE)
        got = actx.lml_grad_ard()
    finally:
        actx.set_option("nb", 0)
        actx.set_lengthscales(None)
    _hold_gradient(got, ref, "N=1500 d=8 nb=%d" % nb)


def test_gradient_outputs_are_optional(actx):
    import ctypes as C
    from gaussian_process_amd._lib import check
    X, y, r, _ = _mirror(130, 2)
    try:
        actx.set_train(X, y)
        actx.set_lengthscales(r)
        actx.factorize(1.2, 1.3, NOISE)
        full = actx.lml_grad_ard()
        dn = C.c_double()
        check(actx._lib.gpmi_lml_grad_ard(actx._h, None, None, None, C.byref(dn)))
        assert dn.value == full[3]
        check(actx._lib.gpmi_lml_grad_ard(actx._h, None, None, None, None))
    finally:
        actx.set_lengthscales(None)


# ---------------------------------------------------------------------------------- consistency with gpmi_lml_grad
def test_consistent_with_the_two_component_gradient(actx):
    X, y, r, ref = _mirror(300, 3)
    l = 1.3
    try:
        actx.set_train(X, y)
        actx.set_lengthscales(r)
        actx.factorize(1.2, l, NOISE)
        d_r, d_l, d_s, _ = actx.lml_grad_ard()
        dl2, ds2 = actx.lml_grad()           # reads the scaled inputs: the derivative w.r.t. the common multiplier l
    finally:
        actx.set_lengthscales(None)
    assert abs(float(r @ d_r) - l * dl2) <= GRAD_RTOL * l * ref["s_l"]
    assert abs(d_l - dl2) <= GRAD_RTOL * ref["s_l"]
    assert abs(d_s - ds2) <= GRAD_RTOL * ref["s_sigma"]


def test_no_lengthscales_d1_is_the_isotropic_gradient(actx):
    X, y = R.problem(200, 1, seed=9)
    l = 0.8
    ref = R.lml_and_grad(X, y, np.ones(1), 1.1, l, NOISE)
    actx.set_lengthscales(None)
    actx.fit(X, y, 1.1, l, NOISE)
    d_r, d_l, d_s, _ = actx.lml_grad_ard()
    dl2, ds2 = actx.lml_grad()
    assert abs(d_r[0] * 1.0 - l * dl2) <= GRAD_RTOL * l * ref["s_l"]
    assert abs(d_s - ds2) <= GRAD_RTOL * ref["s_sigma"]
    _hold_gradient((d_r, d_l, d_s, actx.lml_grad_ard()[3]), ref, "d=1, none set")


# --------------------------------------------------------------------------------------- isotropic calls unchanged
def test_isotropic_calls_unchanged(actx, fresh):
    X, y = R.problem(641, 5, seed=2)
    try:
        actx.set_train(X, y)
        actx.set_lengthscales(_r(5))
        actx.factorize(1.0, 2.0, NOISE)
    finally:
        actx.set_lengthscales(None)
    a = (actx.fit(X, y, 1.0, 2.0, NOISE), actx.lml_grad(), actx.alpha())
    b = (fresh.fit(X, y, 1.0, 2.0, NOISE), fresh.lml_grad(), fresh.alpha())
    assert a[0] == b[0] and a[1] == b[1] and np.array_equal(a[2], b[2])


# ------------------------------------------------------------------------------------------------ reproducibility
@pytest.mark.parametrize("N,d", [(641, 5), (257, 33)])
def test_gradient_is_bitwise_reproducible(actx, N, d):
    X, y = R.problem(N, d, seed=4)
    try:
        actx.set_train(X, y)
        actx.set_lengthscales(_r(d))
        actx.factorize(1.2, 1.3, NOISE)
        alpha = actx.alpha()
        g1 = actx.lml_grad_ard()
        g2 = actx.lml_grad_ard()
        assert np.array_equal(g1[0], g2[0]) and g1[1:] == g2[1:]
        assert np.array_equal(actx.alpha(), alpha)          # the factor is still usable afterwards
    finally:
        actx.set_lengthscales(None)


# ---------------------------------------------------------------------------------------------------- state rules
def test_state_rules(actx):
    X, y = R.problem(130, 2, seed=6)
    Xs = X[:10] + 0.01
    r = np.array([0.8, 1.7])
    try:
        actx.set_lengthscales(None)
        actx.fit(X, y, 1.0, 1.0, NOISE)
        actx.set_test(Xs)
        actx.set_lengthscales(r)            # the factor belonged to the isotropic covariance
        for call in (actx.predict_resident, actx.alpha, actx.lml_grad, actx.lml_grad_ard):
            with pytest.raises(ValueError):
                call()
        lml = actx.factorize(1.0, 1.0, NOISE)                       # the next fit: usable again, test set kept
        mu, _ = actx.predict_resident()
        assert np.all(np.isfinite(mu))
        actx.laplace_fit(X, np.where(y > 0, 1.0, -1.0), 1.0, 1.0)
        actx.set_lengthscales(r * 2)
        with pytest.raises(ValueError):
            actx.laplace_predict(Xs)
        # refused values leave the context as it was
        for bad in ([1.0, 0.0], [1.0, -2.0], [np.nan, 1.0], [np.inf, 1.0], [1.0, 2.0, 3.0], [1.0]):
            with pytest.raises(ValueError):
                actx.set_lengthscales(bad)
        actx.set_lengthscales(r)
        assert actx.fit(X, y, 1.0, 1.0, NOISE) == lml               # same d: set_train keeps the lengthscales
        X3, y3 = R.problem(130, 3, seed=8)
        lml3 = actx.fit(X3, y3, 1.0, 1.0, NOISE)                    # another d clears them
        ref3 = R.lml(X3, y3, np.ones(3), 1.0, 1.0, NOISE)
        assert abs(lml3 - ref3) <= LML_RTOL * abs(ref3)
        actx.set_lengthscales([1.0, 2.0, 3.0])                      # and the new d is the one that counts now
        with pytest.raises(ValueError):
            actx.set_lengthscales(r)
    finally:
        actx.set_lengthscales(None)


# ---------------------------------------------------------------------------------------------------------- tuner
def test_tuner_finds_the_relevant_dimension(actx):
    from gaussian_process_amd import tune_hyperparms_regression as T
    X, y = R.problem(400, 3, seed=12, relevant=1)        # y depends on dimension 0 only
    try:
        ls, sigma, noise, lml, trace = T.tune_hyperparms_ard(X, y, sigma=1.0, lengthscales=np.ones(3), noise_var=NOISE,
                                                             max_iter=30, ctx=actx)
        print("tuner: lengthscales %s sigma %.3f noise %.2e lml %.3f -> %.3f in %d steps"
              % (ls, sigma, noise, trace[0], lml, len(trace) - 1))
        assert lml > trace[0] and trace[-1] == lml
        assert np.all(np.diff(trace) >= 0)
        assert np.argmin(ls) == 0
        # lml_and_gradient_ard at the point reached: the LML the tuner reports
        lml2, d_ls, d_sigma, d_noise = T.lml_and_gradient_ard(X, y, sigma, ls, noise_var=noise, ctx=actx)
        assert lml2 == lml and d_ls.shape == (3,)
    finally:
        actx.set_lengthscales(None)


def test_vector_l_through_the_drop_in_functions(actx, fresh):
    """prediction / compute_mar_likelihood / RBF_kernel with a d-vector l: the isotropic call on X / l with l = 1"""
    from gaussian_process_amd import GP_regression as G
    from gaussian_process_amd import tune_hyperparms_regression as T
    X, y = R.problem(130, 2, seed=13)
    Xs = X[:9] + 0.02
    vec = np.array([0.8, 2.2])
    np.random.seed(1)
    a = G.prediction(X, Xs, y, 'rbf', vec, 2, return_lml=True, ctx=actx)
    np.random.seed(1)
    b = G.prediction(X / vec, Xs / vec, y, 'rbf', 1.0, 2, return_lml=True, ctx=fresh)
    for p, q in zip(a, b):
        assert np.array_equal(p, q)
    assert T.compute_mar_likelihood(X, None, y, 1.0, vec, ctx=actx) == T.compute_mar_likelihood(X / vec, None, y, 1.0, 1.0, ctx=fresh)
    # neither call left lengthscales behind
    assert actx.fit(X, y, 1.0, 1.0, NOISE) == fresh.fit(X, y, 1.0, 1.0, NOISE)
    assert np.array_equal(G.RBF_kernel(X, Xs, 1.3, vec), G.RBF_kernel(X / vec, Xs / vec, 1.3, 1.0))
