"""gpmi_sparse_grad, the gradient of the VFE bound on the GPU, against the long-double mirror of tests/sgpr_grad_ref.py,
and tune_hyperparms_sparse on top of it.

The bar of every component is GRAD_RTOL = 1e-8 (tests/test_parity_gpu.py) times that component's cancellation scale from
the mirror.  Whether float64 arithmetic can meet it is settled on the CPU first: where the float64 mirror itself misses
that bar against the long-double one, the component's bar becomes ten times their difference (the margin covers another,
equally valid order of summation) and is printed.  No bar comes from the device's output.  The shapes are the smallest
at which the kernels can go wrong, not the workload's."""
import ctypes as C

import numpy as np
import pytest

import ard_ref as R
import sgpr_grad_ref as G
import sgpr_ref as S

pytestmark = pytest.mark.gpu

GRAD_RTOL = 1e-8      # tests/test_parity_gpu.py: relative to the terms that cancel
LD = np.longdouble
TWO_SPLITS = (129, 2, 40, 1e-2)       # 256 padded rows: the second 128-row chunk holds one real row
SLABS = (641, 5, 130, 5e-4)
CASES = S.CASES + [TWO_SPLITS, S.MID]
COMPONENTS = ["l", "sigma", "noise", "r", "Z"]


@pytest.fixture(scope="module")
def gctx():
    """a context of this module's own: lengthscales and options are context state"""
    from gaussian_process_amd import GPContext
    c = GPContext(0)
    yield c
    c.close()


_cache = {}


def _problem(N, d, m):
    X, y = R.problem(N, d, seed=100 + d)
    return X, y, S.inducing(X, m)


def _lengthscales(d):
    return np.random.default_rng(3).uniform(0.7, 1.6, size=d)


def _reference(N, d, m, noise, ard, l=S.ELL):
    """(X, y, Z, r or None, long-double mirror, bars): computed once per input, left unchanged"""
    key = (N, d, m, noise, ard, l)
    if key not in _cache:
        X, y, Z = _problem(N, d, m)
        r = _lengthscales(d) if ard else None
        ref = G.grad(X, y, Z, S.SIGMA, l, noise, r=r, dtype=LD)
        f64 = G.grad(X, y, Z, S.SIGMA, l, noise, r=r)
        bars = {}
        for k in COMPONENTS:
            plain = GRAD_RTOL * np.asarray(ref["s_" + k], dtype=np.float64)
            miss = np.abs(np.asarray(f64["g_" + k], dtype=LD) - ref["g_" + k]).astype(np.float64)
            bars[k] = np.where(miss <= plain, plain, 10.0 * miss)
            if np.any(miss > plain):
                print("N=%d d=%d m=%d ard=%d %s: float64 misses 1e-8 x scale; measured bar %s" % (N, d, m, ard, k, bars[k]))
        _cache[key] = (X, y, Z, r, ref, bars)
    return _cache[key]


def _device(ctx, X, y, Z, r, noise, sigma=S.SIGMA, l=S.ELL):
    value = ctx.sparse_fit(X, y, Z, sigma, l, noise, method="vfe", lengthscales=r)
    return value, ctx.sparse_grad()


def _hold(g, ref, bars, tag):
    worst = {}
    for k in COMPONENTS:
        err = np.abs(np.asarray(g[k], dtype=LD) - ref["g_" + k]).astype(np.float64)
        worst[k] = float(np.max(err / bars[k]))
    print(tag + ": error / bar  " + "  ".join("%s %.2e" % kv for kv in worst.items()))
    for k, w in worst.items():
        assert w <= 1.0, (tag, k, w)


def _same_bits(a, b):
    return all(np.array_equal(np.asarray(a[k]), np.asarray(b[k])) for k in COMPONENTS)


# -------------------------------------------------------------------------------------------------------- the mirror
@pytest.mark.parametrize("ard", [0, 1])
@pytest.mark.parametrize("N,d,m,noise", CASES)
def test_against_the_mirror(gctx, N, d, m, noise, ard):
    X, y, Z, r, ref, bars = _reference(N, d, m, noise, ard)
    value, g = _device(gctx, X, y, Z, r, noise)
    assert abs(value - float(ref["value"])) <= 1e-9 * abs(float(ref["value"]))
    _hold(g, ref, bars, "N=%d d=%d m=%d ard=%d" % (N, d, m, ard))
    # sum_k r_k dF/dr_k = l dF/dl, from the device's own numbers
    rr = np.ones(d) if r is None else r
    assert abs(np.sum(g["r"] * rr) - S.ELL * g["l"]) <= 1e-12 * S.ELL * float(ref["s_l"])


# -------------------------------------------------------------------------------------------------- wider inputs
@pytest.mark.parametrize("d", [12, 32])
def test_wide_inputs(gctx, d):
    """d = 12 and d = 32 run the contraction kernel's forms for up to 16 and up to 32 dimensions (the shapes above stop at
    8); the lengthscale grows with sqrt(d) so that the covariances stay of order one"""
    N, m, noise, l = 200, 48, 5e-4, S.ELL * np.sqrt(d / 5.0)
    X, y, Z, r, ref, bars = _reference(N, d, m, noise, 1, l)
    value, g = _device(gctx, X, y, Z, r, noise, l=l)
    assert abs(value - float(ref["value"])) <= 1e-9 * abs(float(ref["value"]))
    _hold(g, ref, bars, "N=%d d=%d m=%d" % (N, d, m))


def test_more_than_32_dimensions_are_refused(gctx):
    X, y, Z = _problem(64, 33, 8)
    gctx.sparse_fit(X, y, Z, S.SIGMA, 4.0, 5e-4, lengthscales=None)
    with pytest.raises(ValueError, match="at most 32 input dimensions"):
        gctx.sparse_grad()


# ------------------------------------------------------------------------------------------------------------- slabs
@pytest.mark.parametrize("slab", [128, 256, 0])
def test_slabs(gctx, slab):
    """N = 641 (padded: 768 rows), m = 130: six slabs of 128, three of 256, or one; the last slab holds one real row"""
    N, d, m, noise = SLABS
    X, y, Z, r, ref, bars = _reference(N, d, m, noise, 1)
    gctx.set_option("sparse_slab", slab)
    try:
        _, a = _device(gctx, X, y, Z, r, noise)
        _, b = _device(gctx, X, y, Z, r, noise)
        c = gctx.sparse_grad()                      # and once more on the same resident fit
    finally:
        gctx.set_option("sparse_slab", 0)
    _hold(a, ref, bars, "slab=%d" % slab)
    assert _same_bits(a, b) and _same_bits(a, c)


# ------------------------------------------------------------------------------------------------- the fit survives
def test_the_resident_fit_survives(gctx):
    N, d, m, noise = S.CASES[1]
    X, y, Z, r, _, _ = _reference(N, d, m, noise, 1)
    Xs = np.random.default_rng(7).uniform(0.0, 4.0, size=(64, d))
    gctx.sparse_fit(X, y, Z, S.SIGMA, S.ELL, noise, lengthscales=r)
    c0, q0 = gctx.sparse_state()
    mu0, var0 = gctx.sparse_predict(Xs, want_sd=False)
    g0 = gctx.sparse_grad()
    c1, q1 = gctx.sparse_state()
    mu1, var1 = gctx.sparse_predict(Xs, want_sd=False)
    g1 = gctx.sparse_grad()                         # after a prediction overwrote the slab workspace
    assert np.array_equal(c0, c1) and np.array_equal(q0, q1)
    assert np.array_equal(mu0, mu1) and np.array_equal(var0, var1)
    assert _same_bits(g0, g1)


# --------------------------------------------------------------------------------------------------- lengthscales
def test_vector_lengthscale_equals_prescaled_inputs(gctx):
    N, d, m, noise = S.CASES[0]
    X, y, Z, r, _, _ = _reference(N, d, m, noise, 1)
    _, a = _device(gctx, X, y, Z, r, noise)
    _, b = _device(gctx, X / r, y, Z / r, None, noise)
    assert a["l"] == b["l"] and a["sigma"] == b["sigma"] and a["noise"] == b["noise"]
    # d/dZ = (d/dz) / r: the same sums, one more rounding
    assert np.max(np.abs(a["Z"] - b["Z"] / r) / np.maximum(np.abs(a["Z"]), 1e-300)) <= 4 * np.finfo(np.float64).eps
    assert np.max(np.abs(a["r"] * r - b["r"]) / np.maximum(np.abs(b["r"]), 1e-300)) <= 4 * np.finfo(np.float64).eps


# ------------------------------------------------------------------------------------------------------- refusals
def test_refusals(gctx):
    from gaussian_process_amd import GPContext
    from gaussian_process_amd._lib import check
    N, d, m, noise = S.CASES[0]
    X, y, Z = _problem(N, d, m)
    with GPContext(0) as fresh:
        with pytest.raises(ValueError, match="no sparse fit resident"):
            fresh.sparse_grad()
    gctx.sparse_fit(X, y, Z, S.SIGMA, S.ELL, noise, method="fitc", lengthscales=None)
    with pytest.raises(ValueError, match="FITC"):
        gctx.sparse_grad()
    drops = [lambda: gctx.fit(X, y, S.SIGMA, S.ELL, noise),
             lambda: gctx.laplace_fit(X, np.where(y > np.median(y), 1.0, -1.0), S.SIGMA, S.ELL),
             lambda: gctx.set_lengthscales(np.full(d, 1.5))]
    try:
        for drop in drops:
            gctx.sparse_fit(X, y, Z, S.SIGMA, S.ELL, noise, lengthscales=None)
            gctx.sparse_grad()
            drop()
            with pytest.raises(ValueError, match="no sparse fit resident"):
                gctx.sparse_grad()
    finally:
        gctx.set_lengthscales(None)
    # every output may be NULL
    gctx.sparse_fit(X, y, Z, S.SIGMA, S.ELL, noise, lengthscales=None)
    full = gctx.sparse_grad()
    check(gctx._lib.gpmi_sparse_grad(gctx._h, None, None, None, None, None))
    dn = C.c_double()
    check(gctx._lib.gpmi_sparse_grad(gctx._h, None, None, C.byref(dn), None, None))
    assert dn.value == full["noise"]
    assert gctx.sparse_grad(want_Z=False)["Z"] is None


# ------------------------------------------------------------------------------------------------------- the tuner
def test_tuner(gctx):
    from gaussian_process_amd.tune_hyperparms_regression import tune_hyperparms_sparse
    N, d, m, noise = 300, 5, 64, 5e-4
    X, y, Z0 = _problem(N, d, m)
    ls0 = np.full(d, 2.0 * S.ELL)                    # off by a factor 2
    for optimise_Z in (True, False):
        ls, sigma, nv, Z, bound, trace = tune_hyperparms_sparse(X, y, Z0, sigma=S.SIGMA, lengthscales=ls0, noise_var=noise,
                                                                optimise_Z=optimise_Z, max_iter=12, ctx=gctx)
        print("optimise_Z=%s: %d accepted steps, bound %.6f -> %.6f" % (optimise_Z, len(trace) - 1, trace[0], trace[-1]))
        assert len(trace) >= 2 and np.all(np.diff(trace) >= 0) and trace[-1] > trace[0]
        assert bound == trace[-1]
        # the ascent starts at the exponentials of the logarithms it keeps
        start = np.exp(np.log(np.concatenate([ls0, [S.SIGMA, noise]])))
        assert trace[0] == gctx.sparse_fit(X, y, Z0, start[d], 1.0, start[d + 1], lengthscales=start[:d])
        assert bound == gctx.sparse_fit(X, y, Z, sigma, 1.0, nv, lengthscales=ls)
        assert Z.shape == Z0.shape
        assert np.array_equal(Z, Z0) != optimise_Z
    gctx.set_lengthscales(None)


def test_bound_and_gradient(gctx):
    from gaussian_process_amd import sparse_bound_and_gradient
    N, d, m, noise = S.CASES[0]
    X, y, Z, r, ref, bars = _reference(N, d, m, noise, 1)
    value, g = sparse_bound_and_gradient(X, y, Z, S.SIGMA, S.ELL * r, noise, ctx=gctx)
    # a vector l: the common lengthscale is 1 and "r" is the derivative w.r.t. l = ELL r, i.e. dF/dr / ELL
    assert abs(value - float(ref["value"])) <= 1e-9 * abs(float(ref["value"]))
    assert np.all(np.abs(g["r"] * S.ELL - np.asarray(ref["g_r"], dtype=np.float64)) <= bars["r"])
    assert np.all(np.abs(g["Z"] - np.asarray(ref["g_Z"], dtype=np.float64)) <= bars["Z"])
    with pytest.raises(ValueError, match="no sparse fit resident"):
        gctx.sparse_grad()                           # the lengthscales were cleared, and the fit with them
