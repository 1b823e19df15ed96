"""The CO2 composite kernel's LML gradient without a GPU: the preconditions on the NumPy mirror the GPU tests are held
against (tests/co2_grad_ref.py) -- its K against the reference's own vectors, its long-double gradient against
long-double central differences, its float64 gradient against the long-double one at half the GPU bar -- and the
gradient tuner of CO2_example.py over a NumPy stub context."""
import numpy as np
import pytest

import co2_grad_ref as R
from conftest import golden

CO2_K_RTOL = 2e-14     # tests/test_parity_gpu.py
FD_RTOL = 1e-5         # of each component's cancellation scale: the truncation error of the difference step
MIRROR_RTOL = 5e-9     # half of GRAD_RTOL, the way test_panel_ref_cpu.py holds references to half of every bar


@pytest.fixture(scope="module")
def fixture():
    g = golden("kernels_bo_co2")
    return g, g["co2_theta"], g["co2_X"], g["co2_y"]


_ld_cache = {}


def long_double_mirror(N, th, X, y):
    """one long-double evaluation per size, shared and left unchanged"""
    if N not in _ld_cache:
        _ld_cache[N] = R.lml_and_grad(X[:N], y[:N], th, R.NOISE, np.longdouble)
    return _ld_cache[N]


def test_mirror_kernel_matrix_is_the_reference_one(fixture):
    g, th, X, _ = fixture
    K = R.kernel(X, th)
    assert np.allclose(K[:16, :16], g["co2_K_corner"], rtol=CO2_K_RTOL, atol=0)
    assert np.allclose(K[-1], g["co2_K_lastrow"], rtol=CO2_K_RTOL, atol=0)
    Kl = R.kernel(X, th, np.longdouble)
    assert np.allclose(np.asarray(Kl, dtype=np.float64), K, rtol=CO2_K_RTOL, atol=0)


def test_mirror_lml_is_the_reference_one(fixture):
    g, th, X, y = fixture
    want = float(g["co2_lml"])
    assert abs(R.lml(X, y, th) - want) <= 1e-9 * abs(want)          # the CO2 bar of tests/test_parity_gpu.py


def test_long_double_gradient_matches_central_differences(fixture):
    """Step 1e-6 * theta, bar 1e-5 of each component's cancellation scale.  What is left at that step is the rounding of
    the two long-double LML values (K_y has condition 1.6e7 here), not truncation: measured worst component 7.9e-6 at
    step 1e-6 and 2.0e-7 at step 1e-5 (1.1e-5 and 5.5e-7 with the inner products of the mirror's Cholesky kept in one
    running sum, which is why it sums pairwise)."""
    _, th, X, y = fixture
    N = 130
    ref = long_double_mirror(N, th, X, y)
    fd = R.central_differences(X[:N], y[:N], th, R.NOISE, 1e-6)
    err = R.error_over_scale(fd[:11], fd[11], ref)
    print("analytic against central differences, error / scale:", " ".join("%.1e" % e for e in err))
    assert np.all(err <= FD_RTOL), err


@pytest.mark.parametrize("N", [130, 300, 360])
def test_float64_mirror_against_long_double(fixture, N):
    _, th, X, y = fixture
    ref = long_double_mirror(N, th, X, y)
    got = R.lml_and_grad(X[:N], y[:N], th, R.NOISE)
    err = R.error_over_scale(got["g_theta"], got["g_noise"], ref)
    print("N=%d float64 mirror against long double, error / scale: worst %.1e" % (N, err.max()))
    assert np.all(err <= MIRROR_RTOL), err
    assert abs(got["lml"] - float(ref["lml"])) <= 1e-9 * abs(float(ref["lml"]))


@pytest.mark.parametrize("N,d", [(130, 2), (257, 11)])
def test_multi_dimensional_problem_is_positive_definite(N, d):
    X, y = R.problem_md(N, d, seed=100 + d)
    ref = R.lml_and_grad(X, y, R.THETA_MD)
    assert np.isfinite(ref["lml"]) and np.all(np.isfinite(ref["g_theta"])) and np.all(ref["s_theta"] > 0)
    # both come from the sum over the diagonal
    assert abs(ref["g_noise"] - ref["g_theta"][10] / (2 * R.THETA_MD[10])) <= 1e-12 * ref["s_noise"]


# ------------------------------------------------------------------------------------------ the tuner, no device
def test_tuner_over_the_mirror(fixture):
    from gaussian_process_amd import CO2_example as C2
    _, th, X, y = fixture
    X, y = X[:120], y[:120]
    c = R.MirrorContext()
    got, noise, lml, trace = C2.tune_hyperparameters_gradient(X, y, max_iter=6, ctx=c)
    print("tuner over the mirror: lml %.6f -> %.6f in %d accepted steps, %d factorisations"
          % (trace[0], lml, len(trace) - 1, c.factorizations))
    assert np.all(np.diff(trace) >= 0)
    assert trace[-1] > trace[0] and trace[-1] == lml
    assert abs(trace[0] - R.lml(X, y, C2.HYPERMS_BOOK)) <= 1e-10 * abs(trace[0])       # the default start
    at = R.lml(X, y, got, noise)
    assert abs(lml - at) <= 1e-10 * abs(at)
    assert got.shape == (11,) and np.all(got > 0) and not np.array_equal(got, C2.HYPERMS_BOOK)
    assert noise == C2.NOISE_VAR                                  # tune_noise=False: unchanged
    assert c.kind == "rbf"


def test_tuner_tunes_the_noise_when_asked(fixture):
    from gaussian_process_amd import CO2_example as C2
    _, th, X, y = fixture
    c = R.MirrorContext()
    got, noise, lml, trace = C2.tune_hyperparameters_gradient(X[:120], y[:120], th, noise_var=2e-3, tune_noise=True,
                                                              max_iter=3, ctx=c)
    assert np.all(np.diff(trace) >= 0) and trace[-1] > trace[0]
    assert noise > 0 and noise != 2e-3
    at = R.lml(X[:120], y[:120], got, noise)
    assert abs(lml - at) <= 1e-10 * abs(at)
    assert c.kind == "rbf"


def test_tuner_refuses_bad_starts(fixture):
    from gaussian_process_amd import CO2_example as C2
    _, th, X, y = fixture
    for bad in (0.0, -0.78, np.nan, np.inf):
        start = np.array(th)
        start[7] = bad
        c = R.MirrorContext()
        with pytest.raises(ValueError):
            C2.tune_hyperparameters_gradient(X[:20], y[:20], start, ctx=c)
        assert c.factorizations == 0
    with pytest.raises(ValueError):
        C2.tune_hyperparameters_gradient(X[:20], y[:20], th[:10], ctx=R.MirrorContext())
    with pytest.raises(ValueError):
        C2.tune_hyperparameters_gradient(X[:20], y[:20], th, noise_var=0.0, ctx=R.MirrorContext())


def test_lml_and_gradient_leaves_the_context_on_rbf(fixture):
    from gaussian_process_amd import CO2_example as C2
    _, th, X, y = fixture
    c = R.MirrorContext()
    lml, d_theta, d_noise = C2.lml_and_gradient(X[:60], y[:60], th, ctx=c)
    ref = R.lml_and_grad(X[:60], y[:60], th)
    assert lml == ref["lml"] and np.array_equal(d_theta, ref["g_theta"]) and d_noise == ref["g_noise"]
    assert c.kind == "rbf"
    c.fit_at = None
    with pytest.raises(ValueError):                               # a failing call switches back too
        C2.lml_and_gradient(X[:60], y[:60], th[:5], ctx=c)
    assert c.kind == "rbf"


def test_signatures_list_the_entry_point():
    from gaussian_process_amd import _lib
    assert _lib.SIGNATURES["gpmi_lml_grad_co2"] == [_lib._vp, _lib._dp, _lib._dp]
