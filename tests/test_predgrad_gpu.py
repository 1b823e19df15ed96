"""gpmi_predict_grad_resident on the device: the gradients of the predictive mean and variance at the test inputs, held to
the long-double mirror (tests/predgrad_ref.py) on the cases of tests/predgrad_cases.py -- N = 641 (six blocks, a partial
last one) and 1500, d = 1, 3, 8, 32, n = 1, 5, 16, 17, 37, 200, the four kernels with and without lengthscales, a third of
the test points outside the training box and one ON a training point -- with both routes to W forced by "pgrad_sweep"
and each held to the mirror, not to the other.

Errors are |got - ref| / S elementwise, maximum over the case (predgrad_ref.err).  Bars: 20 x what the float64 mirror
misses of the long-double one on the same case, never below 1e-13 (predgrad_cases.case; tests/test_predgrad_cpu.py
prints the table).  Every comparison prints its figures before it asserts.

Also: a first-generation factor takes the inverse route whatever "pgrad_sweep" says; mu and var are gpmi_predict_resident's
bits; v, the posterior factor and a later prediction are untouched; the call works without a preceding prediction, with v
in the rows of A after the one-pass and augmented fits, after an append and after a remove; without dvar nothing is
swept; the refusals; the same bits every run; and one suggest_next run on a 1-D toy."""
import numpy as np
import pytest

import predgrad_cases as PC
import predgrad_ref as G

pytestmark = pytest.mark.gpu

ROUTE = {"sweep": 1, "inverse": 0, "by_size": -1}


@pytest.fixture(scope="module")
def ctx():
    from gaussian_process_amd import GPContext
    c = GPContext(0)
    yield c
    c.close()


def _setup(ctx, c, route="by_size", fused=1):
    ctx.set_kernel(c["kind"])
    ctx.set_option("panel_fused", fused)
    ctx.set_option("pgrad_sweep", ROUTE[route])


def _fit(ctx, c, route="by_size", fused=1, X=None, y=None):
    _setup(ctx, c, route, fused)
    ctx.fit(c["X"] if X is None else X, c["y"] if y is None else y, c["sigma"], c["l"], c["noise"], lengthscales=c["r"])
    ctx.set_option("panel_fused", 1)       # the resident factor keeps its kind; later factorisations take the default


def _hold(tag, c, got):
    mu, var, dmu, dvar = got
    ref = c["ld"]
    e_mu = G.err(dmu, ref["dmu"], ref["S_mu"])
    print("%s: dmu %.2e of S (bar %.1e, float64 %.1e)" % (tag, e_mu, c["bar_mu"], c["miss_mu"]))
    e_var = None
    if dvar is not None:
        e_var = G.err(dvar, ref["dvar"], ref["S_var"])
        print("%s: dvar %.2e of S (bar %.1e, float64 %.1e)" % (tag, e_var, c["bar_var"], c["miss_var"]))
    assert np.all(np.isfinite(dmu)) and (dvar is None or np.all(np.isfinite(dvar)))
    assert e_mu <= c["bar_mu"], (tag, e_mu)
    assert e_var is None or e_var <= c["bar_var"], (tag, e_var)
    # mean and variance are the prediction's: to the parity suite's absolute bars of 1e-9 / 1e-8 here (bitwise below)
    assert np.max(np.abs(mu - np.asarray(ref["mu"], dtype=np.float64))) <= 1e-8 * max(1.0, float(np.max(np.abs(ref["mu"]))))


@pytest.mark.parametrize("route", ["sweep", "inverse"])
@pytest.mark.parametrize("name", sorted(PC.CASES))
def test_both_routes_against_the_mirror(ctx, name, route):
    """no prediction precedes the call: it forms v itself"""
    c = PC.case(name)
    _fit(ctx, c, route)
    got = ctx.predict_grad(c["Xs"])
    _hold("%s %s" % (name, route), c, got)


@pytest.mark.parametrize("name", ["rbf_d3_n37_ard_1e-4", "m32_d8_n16_ard"])
def test_first_generation_factor_takes_the_inverse_route(ctx, name):
    """a "panel_fused" 0 fit carries no tile inverses: by size and under "pgrad_sweep" 1 it gets the bits of "pgrad_sweep" 0
    (the sweep would read K's leftovers for inverses), and they hold the mirror's bar"""
    c = PC.case(name)
    out = {}
    for route in ("inverse", "by_size", "sweep"):
        _fit(ctx, c, route, fused=0)
        out[route] = ctx.predict_grad(c["Xs"])
    _hold("%s first generation" % name, c, out["by_size"])
    for route in ("by_size", "sweep"):
        for a, b in zip(out[route], out["inverse"]):
            assert np.array_equal(a, b), route


@pytest.mark.parametrize("route", ["sweep", "inverse"])
def test_agrees_with_the_other_calls_bit_for_bit(ctx, route):
    """mu and var are predict_resident's; post_chol and predict_resident return the same bits before and after; two runs
    give the same bits"""
    c = PC.case("rbf_d3_n37_ard_1e-4")
    _fit(ctx, c, route)
    mu0, var0 = ctx.predict(c["Xs"], want_sd=False)
    L0 = ctx.post_chol(1e-6)
    a = ctx.predict_grad()
    b = ctx.predict_grad()
    for x, y in zip(a, b):
        assert np.array_equal(x, y)
    assert np.array_equal(a[0], mu0) and np.array_equal(a[1], var0)
    assert np.array_equal(ctx.post_chol(1e-6), L0)
    assert np.array_equal(ctx.post_chol(1e-2), ctx.post_chol(1e-2))
    mu1, var1 = ctx.predict_resident(want_sd=False)
    assert np.array_equal(mu1, mu0) and np.array_equal(var1, var0)
    _hold("after a prediction, %s" % route, c, a)


@pytest.mark.parametrize("route", ["sweep", "inverse"])
@pytest.mark.parametrize("form", ["one_pass", "augmented"])
def test_v_in_the_rows_of_A(ctx, form, route):
    """after gpmi_fit_predict_resident and gpmi_fit_predict_sample_resident v lies below the y row: it is reused there, mu
    and var are the fit's own bits, and the riding posterior factor is untouched"""
    c = PC.case("m32_d8_n16_ard" if form == "one_pass" else "rbf_d3_n17_iso_0.1")
    _setup(ctx, c, route)
    ctx.set_lengthscales(None)
    ctx.set_train(c["X"], c["y"])
    if c["r"] is not None:
        ctx.set_lengthscales(c["r"])
    ctx.set_test(c["Xs"])
    if form == "one_pass":
        _, mu0, var0 = ctx.fit_predict_resident(c["sigma"], c["l"], c["noise"], want_sd=False)
    else:
        _, mu0, var0, L0 = ctx.fit_predict_sample_resident(c["sigma"], c["l"], c["noise"], 1e-6, want_sd=False)
    got = ctx.predict_grad()
    assert np.array_equal(got[0], mu0) and np.array_equal(got[1], var0)
    if form == "augmented":
        assert np.array_equal(ctx.post_chol(1e-6), L0)
    _hold("%s %s" % (form, route), c, got)


@pytest.mark.parametrize("route", ["sweep", "inverse"])
def test_after_an_append_and_after_a_remove(ctx, route):
    """the fit of the first 600 points with the other 41 appended, and the fit with five more points in its middle and
    those removed again, are the case's fit: the same mirror, the same bars"""
    c = PC.case("rbf_d3_n37_ard_1e-4")
    _fit(ctx, c, route, X=c["X"][:600], y=c["y"][:600])
    ctx.append(c["X"][600:], c["y"][600:])
    _hold("appended %s" % route, c, ctx.predict_grad(c["Xs"]))
    rng = np.random.RandomState(5)
    at = np.array([3, 130, 131, 400, 640])
    X2 = np.insert(c["X"], at, rng.uniform(-2, 2, size=(5, 3)), axis=0)
    y2 = np.insert(c["y"], at, rng.standard_normal(5) * 0.1)
    where = at + np.arange(5)
    assert np.array_equal(np.delete(X2, where, axis=0), c["X"])
    _fit(ctx, c, route, X=X2, y=y2)
    ctx.remove(where)
    _hold("removed %s" % route, c, ctx.predict_grad(c["Xs"]))


def test_without_dvar_nothing_is_swept(ctx):
    c = PC.case("rbf_d8_n200_iso")
    _fit(ctx, c, "sweep")
    ctx.set_option("timing", 1)
    ctx.predict(c["Xs"])
    v_time = ctx.timers()["solve_v"]
    mu, var, dmu, dvar = ctx.predict_grad(want_var_grad=False)
    t = ctx.timers()
    print("solve_v: %.3f ms for v, %.3f ms in the call without dvar; alpha %.3f ms, the pass %.3f ms"
          % (v_time, t["solve_v"], t["alpha"], t["meanvar"]))
    assert dvar is None and t["solve_v"] == 0.0 and t["ks"] == 0.0 and v_time > 0.0
    _hold("without dvar", c, (mu, var, dmu, None))
    full = ctx.predict_grad()
    assert np.array_equal(full[2], dmu)
    assert ctx.timers()["solve_v"] > 0.0


def test_refusals(ctx):
    from gaussian_process_amd import GPContext
    c = PC.case("rbf_d3_n17_iso_0.1")
    with GPContext(0) as fresh:
        fresh.set_train(c["X"], c["y"])
        fresh.set_test(c["Xs"])
        with pytest.raises(ValueError, match="no factorisation resident"):
            fresh.predict_grad()
        fresh.fit(c["X"], c["y"], 1.0, 1.0, 0.1)            # a new training set drops the test set
        with pytest.raises(ValueError, match="no test set"):
            fresh.predict_grad()
        X1 = np.linspace(0, 3, 40)[:, None]
        y1 = np.sin(X1[:, 0])
        fresh.set_kernel("lin", 0.5)
        fresh.fit(X1, y1, 1.0, 1.0, 0.1)
        fresh.set_test(X1[:5])
        with pytest.raises(ValueError, match=r"kernel only \(kinds 0, 4, 5, 6\)"):
            fresh.predict_grad()
        fresh.set_kernel("co2", [1.0, 2.0, 1.0, 3.0, 1.5, 0.5, 1.0, 0.8, 0.2, 1.0, 0.1])
        fresh.fit(X1, y1, 1.0, 1.0, 0.1)
        fresh.set_test(X1[:5])
        with pytest.raises(ValueError, match=r"kernel only \(kinds 0, 4, 5, 6\)"):
            fresh.predict_grad()
        fresh.set_kernel("rbf")
        rng = np.random.RandomState(2)
        X33 = rng.uniform(-1, 1, size=(50, 33))
        fresh.fit(X33, rng.standard_normal(50), 1.0, 5.0, 0.1)
        fresh.set_test(X33[:4])
        with pytest.raises(ValueError, match="at most 32"):
            fresh.predict_grad()
        fresh.laplace_fit(c["X"], np.where(c["y"] > 0, 1.0, -1.0), 1.0, 1.5)
        fresh.set_test(c["Xs"])
        with pytest.raises(ValueError, match="no factorisation resident"):
            fresh.predict_grad()


def test_suggest_next_on_a_toy(ctx):
    """1-D, N = 257: the point suggest_next returns has an expected improvement no lower than the best of 2000 random
    candidates scored by predict"""
    from gaussian_process_amd import GP_regression as R
    rng = np.random.RandomState(11)
    X = rng.uniform(-3, 3, size=(257, 1))
    y = np.sin(2 * X[:, 0]) + 0.4 * X[:, 0] + 0.05 * rng.standard_normal(257)
    keep = np.abs(X[:, 0] - 0.85) > 0.3                     # a gap around the maximum of the target
    X, y = X[keep], y[keep]
    ctx.set_kernel("rbf")
    ctx.set_option("pgrad_sweep", -1)
    ctx.fit(X, y, 1.0, 0.7, 1e-2, lengthscales=None)
    y_best = float(np.max(y))
    bounds = np.array([[-3.0, 3.0]])
    x, v = R.suggest_next(bounds, "EI", n_starts=16, steps=50, ctx=ctx, seed=0, y_best=y_best)
    cand = rng.uniform(-3, 3, size=(2000, 1))
    mu, var = ctx.predict(cand, want_sd=False)
    ei, _ = R.acquisition_and_gradient("EI", mu, var, np.zeros((2000, 1)), np.zeros((2000, 1)), y_best)
    print("suggest_next: x = %.4f EI = %.3e; best of 2000 random candidates %.3e at %.4f" % (x[0], v, ei.max(), cand[ei.argmax(), 0]))
    assert -3.0 <= x[0] <= 3.0
    assert v >= ei.max()
