"""The Matern mirror (tests/matern_ref.py) against scikit-learn's kernel and against long-double central differences of
its own LML, and the host-side pieces of the Matern kinds that need no device.  No GPU.

Bars.  K against scikit-learn: the evaluation orders differ (cdist against the pairwise sum, another polynomial form), so
the bar is absolute, 1e-14 sigma^2 (measured: 8.9e-16 at sigma^2 = 1.44).  Gradient against central differences:
GRAD_RTOL = 1e-8 (tests/test_parity_gpu.py) of each component's cancellation scale, the bar the device is held to against
this mirror; the differences' own error lies far below it (h^2 = 1e-14 relative from the truncation, eps / h = 1e-12 of
the LML's scale from its rounding in long double), as does the float64 mirror's (cond(K_y) eps, cond <= 2e5)."""
import os
import re

import numpy as np
import pytest

import ard_ref as R
import matern_ref as M

LD = np.longdouble
GRAD_RTOL = 1e-8
H = LD(1e-7)
NOISE = 5e-4
SIGMA, ELL = 1.2, 1.3
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

_cache = {}


def _case(nu, dup):
    """a small problem (long-double Cholesky in Python loops), random lengthscales and the mirror: computed once"""
    key = (nu, dup)
    if key not in _cache:
        X, y = R.problem(48, 3, seed=21)
        if dup:                      # two exactly duplicated rows: sq == 0 off the diagonal, where H_1/2 is singular
            X, y = M.duplicate_rows(X, y, [(7, 30), (19, 2)])
        r = np.random.default_rng(5).uniform(0.7, 1.6, size=3)
        _cache[key] = (X, y, r, M.lml_and_grad(X, y, r, nu, SIGMA, ELL, NOISE))
    return _cache[key]


def _central(f, x0, h):
    return (f(LD(x0) + h) - f(LD(x0) - h)) / (2 * h)


# ------------------------------------------------------------------------------------------------ K against sklearn
@pytest.mark.parametrize("N,d", [(130, 2), (300, 5)])
@pytest.mark.parametrize("nu", M.NUS)
def test_kernel_against_sklearn(nu, N, d):
    kernels = pytest.importorskip("sklearn.gaussian_process.kernels")
    X, _ = R.problem(N, d, seed=N)
    r = np.random.default_rng(3).uniform(0.5, 3.0, d)
    sigma, l = 1.2, 1.3
    want = sigma ** 2 * kernels.Matern(length_scale=l * r, nu=nu)(X)
    got = M.kernel(X, r, nu, sigma, l)
    err = np.max(np.abs(got - want))
    print("nu=%.1f N=%d d=%d: max |K - sklearn| = %.2e" % (nu, N, d, err))
    assert err <= 1e-14 * sigma ** 2
    assert np.all(np.diag(got) == sigma * sigma)          # every factor is exactly 1 at sq == 0


def test_mirror_evaluation_order():
    """the header's order, operation for operation, on a 2 x 3 example"""
    A = np.array([[0.0, 1.0], [2.0, 0.5]])
    B = np.array([[0.0, 1.0], [1.0, 1.0], [3.0, -2.0]])
    sq = np.array([[sum((A[i, k] - B[j, k]) ** 2 for k in range(2)) for j in range(3)] for i in range(2)])
    for nu, two_nu in ((0.5, 1.0), (1.5, 3.0), (2.5, 5.0)):
        a = np.sqrt(two_nu) / 1.3
        t = a * np.sqrt(sq)
        P = {0.5: np.ones_like(t), 1.5: 1.0 + t, 2.5: (1.0 + t) + (t * t) * (1.0 / 3.0)}[nu]
        assert np.array_equal(M.kernel_cross(A, B, nu, 1.2, -1.3), (1.2 * 1.2) * (P * np.exp(-t)))    # a negative l means |l|


# ------------------------------------------------------------------------- gradient against central differences
@pytest.mark.parametrize("nu,dup", [(0.5, False), (1.5, False), (2.5, False), (0.5, True)],
                         ids=["nu12", "nu32", "nu52", "nu12_duplicated_rows"])
def test_mirror_gradient_against_central_differences(nu, dup):
    X, y, r, g = _case(nu, dup)
    f0 = M.lml_long(X, y, r, nu, SIGMA, ELL, NOISE)
    assert abs(g["lml"] - float(f0)) <= 1e-11 * abs(g["lml"])
    errs = {}
    errs["l"] = abs(_central(lambda v: M.lml_long(X, y, r, nu, SIGMA, v, NOISE), ELL, H) - g["g_l"]) / g["s_l"]
    errs["sigma"] = abs(_central(lambda v: M.lml_long(X, y, r, nu, v, ELL, NOISE), SIGMA, H) - g["g_sigma"]) / g["s_sigma"]
    errs["noise"] = abs(_central(lambda v: M.lml_long(X, y, r, nu, SIGMA, ELL, v), NOISE, H * LD(NOISE)) - g["g_noise"]) / g["s_noise"]
    for k in range(3):
        def f(v, k=k):
            rr = np.asarray(r, dtype=LD).copy()
            rr[k] = v
            return M.lml_long(X, y, rr, nu, SIGMA, ELL, NOISE)
        errs["r%d" % k] = abs(_central(f, r[k], H) - g["g_r"][k]) / g["s_r"][k]
    print("nu=%.1f dup=%s cond %.1e: " % (nu, dup, g["cond"]) + " ".join("%s %.1e" % (k, float(v)) for k, v in errs.items()))
    assert np.all(np.isfinite(g["g_r"])) and np.isfinite(g["g_l"])
    for k, v in errs.items():
        assert v <= GRAD_RTOL, (k, float(v))


@pytest.mark.parametrize("nu,dup", [(0.5, False), (1.5, False), (2.5, False), (0.5, True)])
def test_euler_identity(nu, dup):
    """sum_k r_k dLML/dr_k = l dLML/dl: a common factor of every r_k is a factor of l"""
    _, _, r, g = _case(nu, dup)
    assert abs(float(r @ g["g_r"]) - ELL * g["g_l"]) <= 1e-12 * ELL * g["s_l"]


def test_loo_mirror_matches_brute_force():
    """the closed leave-one-out forms on a Matern K_y against N fits with one point deleted each"""
    import loo_ref as LR
    X, y, r, _ = _case(1.5, False)
    c = M.loo_closed(X, y, r, 1.5, SIGMA, ELL, NOISE)
    b = LR.brute_from_Ky(M.kernel(X, r, 1.5, SIGMA, ELL) + NOISE * np.eye(X.shape[0]), y)
    assert np.max(np.abs(c["mu"] - b["mu"])) <= 1e-9 and np.max(np.abs(c["var"] - b["var"])) <= 1e-10 * np.max(b["var"]) + 1e-12
    assert abs(c["loo"] - b["loo"]) <= 1e-8 * abs(b["loo"])


# ----------------------------------------------------------------------------------------------- the host surface
def test_kinds_carry_the_three_names():
    from gaussian_process_amd import GPContext
    assert GPContext.KINDS["matern12"] == 4 and GPContext.KINDS["matern32"] == 5 and GPContext.KINDS["matern52"] == 6
    assert {k: GPContext.KINDS[k] for k in ("rbf", "lin", "per", "co2")} == {"rbf": 0, "lin": 1, "per": 2, "co2": 3}
    assert M.KIND == GPContext.MATERN


def test_argument_errors_need_no_device():
    from gaussian_process_amd import GP_regression as G
    from gaussian_process_amd import tune_hyperparms_regression as T

    class Dummy:            # no GPU here: prediction() resets the kernel on its way out, nothing else may be called
        def set_kernel(self, *a):
            assert a == ("rbf",)

    class Strict:           # refused on the host before the context hears of it
        pass
    X, y = np.zeros((4, 2)), np.zeros(4)
    for nu in (1.0, 2, "x", None):
        with pytest.raises(ValueError, match="nu must be"):
            G.matern_kernel(X, X, 1.0, 1.0, nu=nu)
    with pytest.raises(ValueError):
        G.matern_kernel(X, X, 1.0, np.ones((2, 2)), nu=1.5)       # l: a scalar or a d-vector
    with pytest.raises(ValueError):
        G.prediction(X, X, y, "matern32", np.ones((2, 2)), 1, ctx=Dummy())
    with pytest.raises(ValueError, match="kernel_choice"):
        G.prediction(X, X, y, "matern42", 1.0, 1, ctx=Dummy())
    with pytest.raises(ValueError, match="partitioned"):
        G.prediction(X, X, y, "matern52", 1.0, 1, dist=object())
    with pytest.raises(ValueError, match="partitioned"):
        T.compute_mar_likelihood(X, None, y, 1.0, 1.0, dist=object(), kernel="matern32")
    for call in (lambda: T.compute_mar_likelihood(X, None, y, 1.0, 1.0, ctx=Strict(), kernel="lin"),
                 lambda: T.compute_mar_likelihood_batch(X, y, np.ones((1, 3)), ctx=Strict(), kernel="matern"),
                 lambda: T.lml_and_gradient(X, y, 1.0, 1.0, ctx=Strict(), kernel="per"),
                 lambda: T.lml_and_gradient_ard(X, y, 1.0, np.ones(2), ctx=Strict(), kernel="co2"),
                 lambda: T.tune_hyperparms_ard(X, y, ctx=Strict(), kernel="x"),
                 lambda: T.compute_loo_likelihood(X, None, y, 1.0, 1.0, ctx=Strict(), kernel="x"),
                 lambda: T.loo_and_gradient(X, y, 1.0, 1.0, ctx=Strict(), kernel="x"),
                 lambda: T.tune_hyperparms_loo(X, y, ctx=Strict(), kernel="x")):
        with pytest.raises(ValueError, match="kernel must be"):
            call()


def test_kernel_keyword_is_set_on_the_context_every_call():
    from gaussian_process_amd import tune_hyperparms_regression as T
    seen = []

    class Stub:
        def set_kernel(self, kind, *a):
            seen.append(kind)

        def fit(self, *a, **k):
            return 1.5

        def set_lengthscales(self, r):
            pass
    X, y = np.zeros((4, 2)), np.zeros(4)
    assert T.compute_mar_likelihood(X, None, y, 1.0, 1.0, ctx=Stub()) == 1.5
    assert T.compute_mar_likelihood(X, None, y, 1.0, [1.0, 2.0], ctx=Stub(), kernel="matern52") == 1.5
    assert seen == ["rbf", "matern52"]


def test_header_names_the_matern_kinds():
    src = open(os.path.join(ROOT, "include", "gpmi.h")).read()
    assert re.search(r"#define\s+GPMI_ABI_VERSION\s+4\b", src)
    assert re.search(r"GPMI_T_COUNT\s*=\s*16\b", src)
    for pat in (r"kind 4: nu = 1/2", r"kind 5: nu = 3/2", r"kind 6: nu = 5/2", r"sqrt\(2 nu\) / \|l\|",
                r"\(1 \+ t\) \+ \(t \* t\) \* c3"):
        assert re.search(pat, src), pat
    from gaussian_process_amd import _lib
    assert _lib.ABI_VERSION == 4
