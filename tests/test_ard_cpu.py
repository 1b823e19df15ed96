"""Per-dimension lengthscales (ARD) without a GPU: the preconditions on the NumPy mirror the GPU tests are held against
(tests/ard_ref.py), and the Python plumbing that needs no device."""
import numpy as np
import pytest

import ard_ref as R

CASES = [(130, 2), (300, 3), (257, 33)]
L, SIGMA, NOISE = 1.3, 1.2, 5e-4


def _case(N, d):
    X, y = R.problem(N, d, seed=100 + d)
    r = np.random.default_rng(7 + d).uniform(0.5, 3.0, d) * np.sqrt(d)
    return X, y, r


@pytest.fixture(scope="module", params=CASES, ids=lambda c: "N%d_d%d" % c)
def mirror(request):
    X, y, r = _case(*request.param)
    return X, y, r, R.lml_and_grad(X, y, r, SIGMA, L, NOISE)


def _central(f, h):
    return (f(h) - f(-h)) / (2 * h)


def test_mirror_gradient_matches_finite_differences(mirror):
    """the constants of the existing finite-difference test: h = 1e-4 (1e-7 for the noise), 1e-5 * max(1, |fd|)"""
    X, y, r, ref = mirror
    worst = 0.0

    def hold(name, got, fd):
        nonlocal worst
        err = abs(got - fd) / max(1.0, abs(fd))
        worst = max(worst, err)
        assert err <= 1e-5, (name, got, fd)

    for k in range(min(len(r), 6)):      # the first dimensions and, below, the last: each costs two factorisations
        e = np.zeros_like(r)
        e[k] = 1.0
        hold("r%d" % k, ref["g_r"][k], _central(lambda h: R.lml(X, y, r + h * e, SIGMA, L, NOISE), 1e-4))
    e = np.zeros_like(r)
    e[-1] = 1.0
    hold("r_last", ref["g_r"][-1], _central(lambda h: R.lml(X, y, r + h * e, SIGMA, L, NOISE), 1e-4))
    hold("l", ref["g_l"], _central(lambda h: R.lml(X, y, r, SIGMA, L + h, NOISE), 1e-4))
    hold("sigma", ref["g_sigma"], _central(lambda h: R.lml(X, y, r, SIGMA + h, L, NOISE), 1e-4))
    hold("noise", ref["g_noise"], _central(lambda h: R.lml(X, y, r, SIGMA, L, NOISE + h), 1e-7))
    print("worst analytic-vs-fd error: %.2e" % worst)


def test_mirror_euler_identity(mirror):
    """K depends on the products l * r_k only: sum_k r_k dLML/dr_k == l dLML/dl"""
    _, _, r, ref = mirror
    lhs, rhs = float(r @ ref["g_r"]), L * ref["g_l"]
    assert abs(lhs - rhs) <= 1e-12 * max(abs(lhs), abs(rhs)), (lhs, rhs, abs(lhs - rhs) / max(abs(lhs), abs(rhs)))


def test_mirror_isotropic_limit():
    """r = 1 is the plain squared-exponential kernel"""
    X, _, _ = _case(130, 2)
    sq = ((X[:, None, :] - X[None, :, :]) ** 2).sum(-1)
    assert np.array_equal(R.kernel(X, np.ones(2), SIGMA, L), SIGMA ** 2 * np.exp(-.5 / L ** 2 * sq))


# ---------------------------------------------------------------------------------------------- plumbing, no device
class StubContext:
    """Records what the drop-in functions ask of a context.  Its LML is a concave quadratic of the logarithms of
    (lengthscales, sigma, noise) with the maximum at `peak`, and the gradient is exact."""

    def __init__(self, d, peak=None, curv=None):
        self.d = d
        self.peak = np.zeros(d + 2) if peak is None else np.asarray(peak, dtype=np.float64)
        self.curv = np.ones(d + 2) if curv is None else np.asarray(curv, dtype=np.float64)
        self.r = None
        self.calls = []
        self.theta = None

    def set_train(self, X, y):
        self.calls.append(("set_train", np.shape(X)))

    def set_lengthscales(self, r):
        self.calls.append(("set_lengthscales", None if r is None else np.array(r, dtype=np.float64)))
        self.r = None if r is None else np.array(r, dtype=np.float64)

    def factorize(self, sigma, l, noise_var):
        assert l == 1.0
        self.theta = np.log(np.concatenate([self.r, [sigma, noise_var]]))
        self.calls.append(("factorize", self.theta.copy()))
        return 5.0 - .5 * float(np.sum(self.curv * (self.theta - self.peak) ** 2))

    def lml_grad_ard(self):
        g = -self.curv * (self.theta - self.peak) / np.exp(self.theta)      # d/dp = (d/dlog p) / p
        return g[:self.d], 0.0, g[self.d], g[self.d + 1]

    def fit(self, X, y, sigma, l, noise_var, *, lengthscales="keep"):
        self.calls.append(("fit", l, None if lengthscales is None else np.array(lengthscales)))
        return 1.25

    def fit_predict_sample(self, X, y, Xs, sigma, l, noise_var, jitter, want_sd=True, want_factor=True, *,
                           lengthscales="keep"):
        self.calls.append(("fit_predict_sample", l, None if lengthscales is None else np.array(lengthscales)))
        n = np.shape(Xs)[0]
        return 1.25, np.zeros(n), np.ones(n), None

    def post_sample(self, jitter, Z):
        return np.zeros_like(Z)

    def set_kernel(self, *a):
        pass

    def laplace_fit(self, X, y, sigma, l, *, tol, max_iter, lengthscales="keep"):
        self.calls.append(("laplace_fit", l, None if lengthscales is None else np.array(lengthscales)))

    def softmax_fit(self, X, lab, nc, sigma, l, *, tol, max_iter, lengthscales="keep"):
        self.calls.append(("softmax_fit", l, None if lengthscales is None else np.array(lengthscales)))


def test_split_lengthscale():
    from gaussian_process_amd.gp import split_lengthscale
    assert split_lengthscale(2.5) == (2.5, None)
    one = np.array([0.7])
    l, r = split_lengthscale(one)
    assert l is one and r is None                       # the reference's 1-element array: isotropic, passed through
    l, r = split_lengthscale([1.0, 2.0, 3.0])
    assert l == 1.0 and np.array_equal(r, [1.0, 2.0, 3.0])
    with pytest.raises(ValueError):
        split_lengthscale(np.ones((2, 2)))


def test_vector_l_dispatch():
    from gaussian_process_amd import GP_binary_classification as B
    from gaussian_process_amd import GP_multi_classification as M
    from gaussian_process_amd import GP_regression as G
    from gaussian_process_amd import tune_hyperparms_regression as T
    X, Xs, y = np.zeros((6, 3)), np.zeros((4, 3)), np.zeros(6)
    vec = np.array([1.0, 2.0, 0.5])
    c = StubContext(3)
    G.prediction(X, Xs, y, 'rbf', vec, 2, ctx=c)
    name, l, r = c.calls[0]
    assert name == "fit_predict_sample" and l == 1.0 and np.array_equal(r, vec)
    assert c.calls[-1][0] == "set_lengthscales" and c.calls[-1][1] is None      # does not outlive the call
    c = StubContext(3)
    G.prediction(X, Xs, y, 'rbf', 0.8, 2, ctx=c)
    assert c.calls == [("fit_predict_sample", 0.8, None)]                       # scalar: isotropic, cleared by the fit
    c = StubContext(3)
    assert T.compute_mar_likelihood(X, None, y, 1.0, vec, ctx=c) == 1.25
    assert c.calls[0][1] == 1.0 and np.array_equal(c.calls[0][2], vec) and c.calls[-1] == ("set_lengthscales", None)
    c = StubContext(3)
    T.compute_mar_likelihood(X, None, y, 1.0, np.array([0.9]), ctx=c)
    assert len(c.calls) == 1 and c.calls[0][2] is None
    c = StubContext(3)
    B.laplace_fit(X, np.ones(6), 1.0, vec, ctx=c)
    M.laplace_fit(X, np.array([0, 1, 2, 0, 1, 2]), 1.0, vec, ctx=c)
    B.laplace_fit(X, np.ones(6), 1.0, 2.0, ctx=c)
    assert [(n, l) for n, l, _ in c.calls] == [("laplace_fit", 1.0), ("softmax_fit", 1.0), ("laplace_fit", 2.0)]
    assert np.array_equal(c.calls[0][2], vec) and np.array_equal(c.calls[1][2], vec) and c.calls[2][2] is None


def test_vector_l_refused_on_the_partitioned_path():
    from gaussian_process_amd import GP_regression as G
    from gaussian_process_amd import tune_hyperparms_regression as T
    X, Xs, y = np.zeros((6, 3)), np.zeros((4, 3)), np.zeros(6)
    dist = object()          # never touched: the refusal comes first
    with pytest.raises(ValueError, match="partitioned"):
        G.prediction(X, Xs, y, 'rbf', np.ones(3), 1, dist=dist)
    with pytest.raises(ValueError, match="partitioned"):
        T.compute_mar_likelihood(X, None, y, 1.0, np.ones(3), dist=dist)


def test_tuner_accepts_and_halves_on_a_quadratic():
    from gaussian_process_amd import tune_hyperparms_regression as T
    d = 2
    peak = np.log([0.5, 3.0, 2.0, 1e-2])
    # curvature 4: a full gradient step overshoots to the far side (LML lower), so the first trial must be halved
    c = StubContext(d, peak=peak, curv=np.full(d + 2, 4.0))
    ls, sigma, noise, lml, trace = T.tune_hyperparms_ard(np.zeros((5, d)), np.zeros(5), sigma=1.0, noise_var=1e-3,
                                                         max_iter=200, tol=1e-14, ctx=c)
    assert np.all(np.diff(trace) >= 0) and trace[0] < trace[-1] == lml
    assert np.allclose(np.log(np.concatenate([ls, [sigma, noise]])), peak, atol=1e-5)
    assert abs(lml - 5.0) < 1e-9
    # one gradient per accepted point, one factorisation per trial: more trials than accepted points means halvings
    trials = sum(1 for x in c.calls if x[0] == "factorize")
    assert trials > len(trace)
    assert c.calls[0][0] == "set_train" and sum(1 for x in c.calls if x[0] == "set_train") == 1


def test_tuner_first_trial_is_capped_and_halved_in_order():
    from gaussian_process_amd import tune_hyperparms_regression as T
    c = StubContext(1, peak=np.log([2.0, 1.0, 1e-3]), curv=np.array([6.0, 6.0, 6.0]))
    T.tune_hyperparms_ard(np.zeros((5, 1)), np.zeros(5), lengthscales=[1.0], sigma=1.0, noise_var=1e-3, max_iter=1, ctx=c)
    th = [x[1] for x in c.calls if x[0] == "factorize"]
    g = 6.0 * np.log(2.0)                      # the only non-zero log-gradient component
    steps = [(t[0] - th[0][0]) / g for t in th[1:]]
    assert np.isclose(steps[0], T.ARD_MAX_LOG_STEP / g)                  # no parameter moves by more than a factor e
    assert np.allclose(np.array(steps[1:]) / np.array(steps[:-1]), 0.5)  # then halved, one trial each
    # curvature 6 around log 2: a step s lands at log2 * (1 - 6 s) from the peak; accepted once |1 - 6 s| <= 1
    assert abs(1 - 6 * steps[-1]) <= 1 and all(abs(1 - 6 * s) > 1 for s in steps[:-1])


def test_tuner_refuses_bad_start():
    from gaussian_process_amd import tune_hyperparms_regression as T
    c = StubContext(2)
    with pytest.raises(ValueError):
        T.tune_hyperparms_ard(np.zeros((5, 2)), np.zeros(5), lengthscales=[1.0, -1.0], ctx=c)
    with pytest.raises(ValueError):
        T.tune_hyperparms_ard(np.zeros((5, 2)), np.zeros(5), lengthscales=[1.0], ctx=c)
    with pytest.raises(ValueError):
        T.tune_hyperparms_ard(np.zeros((5, 2)), np.zeros(5), noise_var=0.0, ctx=c)


def test_signatures_list_the_new_entry_points():
    from gaussian_process_amd import _lib
    assert "gpmi_set_lengthscales" in _lib.SIGNATURES and "gpmi_lml_grad_ard" in _lib.SIGNATURES
    assert _lib.ABI_VERSION == 4
