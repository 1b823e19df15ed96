"""Sparse GP regression (gpmi_sparse_fit, gpmi_sparse_predict_resident, gpmi_sparse_grad; csrc/sparse.hip) on every factor
route, with factors of more than one panel block, and at the edges of the Gram kernel's launch plan.

The other sparse tests keep m <= 384, so K_uu and B are one panel block (gpmi_ctx::block answers 512): cholesky_inplace
never made a trailing update there, solve_sweep_factor never crossed a block boundary, inverse_transposed never clipped
a row, and every gram_tn_kernel launch had chunks of one 128-row unit.  Here the options of gpmi_set_option that
tests/test_classify_routes_gpu.py drives for the classifiers (ROUTES below) run under the sparse drivers, on

    MID     N 1500 d 8 m 384    m_p 384: three blocks under nb = 128, two under nb = 256
    P600    N 700  d 5 m 600    m_p 640: blocks 512 + 128 at the default nb; the contraction grid's third 256-column
                                group has an upper half that leaves after the barrier; cond K_uu 3.7e5
    TILES   N 2400 d 8 m 2250   m_p 2304, 171 lower tiles.  One slab of 19 units: 5 splits of 512 rows, the last 384;
                                sparse_slab 1408: 6 splits of 256 with a 128-row tail, then a last slab of 1024 rows
    RAGGED  N 4700 d 8 m 1100   m_p 1152, 45 tiles, sparse_slab 3072: 12 splits of 256, then a last slab of 1664 rows in
                                13 splits of 128 -- more splits than the full slab; its last unit holds 92 real rows

all with noise 5e-4 and SIGMA, ELL, JITTER of tests/sgpr_ref.py.  tests/test_sparse_routes_cpu.py asks the plan header
(csrc/gpmi_sparse_plan.h) for these shapes and holds that they are the edges claimed, and holds the float64 mirror to
its own long-double run at P600.

Bars: none is new.  Values, c, q, mean and variance are held by tests/test_sparse_gpu.py::_hold (LML_RTOL x the sum of the
absolute terms; 1e-8; 1e-10 sigma^2; 1e-9 max(1, max|y|); 1e-10 sigma^2) against the float64 mirror, the gradient by
tests/test_sparse_grad_gpu.py::_reference / _hold (1e-8 x the component's cancellation scale from the long-double
mirror, or that module's measured bar where float64 itself misses it on the CPU).  Each mirror is computed once per
session and shared with those modules.

GEMM options: the launches of MID, P600 and RAGGED (sweep updates, trailing updates, neg_product of the gradient) all
have fewer than 128 tiles of 128 x 128, where gemm_tall, gemm_persist and gemm_ticket cannot change a kernel
(tests/test_sparse_routes_cpu.py asks gemm_route); gemm_small_tiles and gemm_small_dma can, and are routes.  TILES
reaches the LDS-DMA family (trailing update 1792 x 1792 x 512, sweep update 2432 x 1792 x 512): gemm_tall with
tall_min_tiles = 0 and gemm_ticket = 2 change its kernels and are routes of test_gram_plan_edges (GEMM_ROUTES);
gemm_persist cannot (fewer than two rounds of blocks).

The sparse path has no backward trsv (c falls out of the factorisation of B as the riding row, the predictions are two
forward sweeps), so there are no trsv_vinv routes.

Bit equality BETWEEN routes is asserted for the lookahead routes alone (la_min: "same bits").

Out of scope: sparse_row_kernel's loop that re-reads a row wider than 8192 columns needs m > 8192, and no mirror of
that size runs in seconds.  test_gram_plan_edges takes no gradient: the long-double gradient mirror would take minutes
at those shapes."""
import numpy as np
import pytest

import sgpr_ref as S
import test_classify_routes_gpu as CR
import test_sparse_gpu as TS
import test_sparse_grad_gpu as TG

pytestmark = pytest.mark.gpu

METHODS = TS.METHODS
PROBLEMS = {"MID": S.MID, "P600": (700, 5, 600, 5e-4), "TILES": (2400, 8, 2250, 5e-4), "RAGGED": (4700, 8, 1100, 5e-4)}
RAGGED_SLAB, TILES_SLAB = 3072, 1408
LAST_SLAB = (TG.SLABS, 512)            # N = 641 (768 padded rows), m = 130: slabs of 512 and 256 rows
DEFAULTS = dict(CR.DEFAULTS, gemm_tall=1, tall_min_tiles=12288, gemm_ticket=0, sparse_slab=0)
# the classifiers' routes without the three of the backward trsv, which the sparse path does not have
ROUTES = {name: opts for name, opts in CR.ROUTES.items() if not name.startswith("trsv_vinv")}
assert list(ROUTES) == ["default", "nb128", "nb256", "lookahead0", "la256_deep", "la256_shallow", "panel_fused0", "small_tiles0",
                        "small_dma0"]
SAME_BITS_AS_DEFAULT = CR.SAME_BITS_AS_DEFAULT
# TILES alone reaches the LDS-DMA family (tests/test_sparse_routes_cpu.py records the kernels)
GEMM_ROUTES = {"default": {}, "tall": {"gemm_tall": 1, "tall_min_tiles": 0}, "ticket2": {"gemm_ticket": 2}}
EDGES = [("TILES", 0, r) for r in GEMM_ROUTES] + [("TILES", TILES_SLAB, r) for r in GEMM_ROUTES] + [("RAGGED", RAGGED_SLAB, "default")]


@pytest.fixture(scope="module")
def rctx():
    """a context of this module's own: lengthscales and options are context state"""
    from gaussian_process_amd import GPContext
    c = GPContext(0)
    yield c
    c.close()


class options:
    def __init__(self, ctx, opts):
        self.ctx, self.opts = ctx, opts

    def __enter__(self):
        for k, v in self.opts.items():
            self.ctx.set_option(k, v)

    def __exit__(self, *exc):
        for k in self.opts:
            self.ctx.set_option(k, DEFAULTS[k])


def fit_predict(ctx, name, method, shape=None):
    """-> (value, (c, q), (mean, var)) without lengthscales, and the mirror's inputs and results"""
    N, d, m, noise = shape or PROBLEMS[name]
    X, y, Z, Xs, ref = TS._mirror(N, d, m, noise, method)
    return TS._run(ctx, X, y, Z, Xs, noise, method, lengthscales=None), ref, y


def gradient(ctx, name, shape=None):
    """-> the gradient of a VFE fit under the lengthscales of tests/test_sparse_grad_gpu.py, its reference and bars"""
    N, d, m, noise = shape or PROBLEMS[name]
    X, y, Z, r, ref, bars = TG._reference(N, d, m, noise, 1)
    value, g = TG._device(ctx, X, y, Z, r, noise)
    assert abs(value - float(ref["value"])) <= 1e-9 * abs(float(ref["value"]))      # as test_sparse_grad_gpu.py
    return g, ref, bars


def same_bits(a, b):
    return a[0] == b[0] and all(np.array_equal(u, v) for u, v in zip(a[1] + a[2], b[1] + b[2]))


def hold(run, ref, y, tag):
    """prints error / bar of every quantity (the measured headroom), then asserts with the bars of test_sparse_gpu._hold"""
    value, (c, q), (mu, var) = run
    ratio = dict(value=abs(value - ref["value"]) / ref["scale"] / TS.LML_RTOL,
                 c=np.max(np.abs(c - ref["c"])) / np.max(np.abs(ref["c"])) / 1e-8,
                 q=np.max(np.abs(q - ref["q"])) / S.SIGMA ** 2 / 1e-10,
                 mean=np.max(np.abs(mu - ref["mean"])) / (1e-9 * max(1.0, np.max(np.abs(y)))),
                 var=np.max(np.abs(var - ref["var"])) / (1e-10 * S.SIGMA ** 2))
    print("%s: error / bar  " % tag + "  ".join("%s %.2e" % kv for kv in ratio.items()) + "  worst %.2e" % max(ratio.values()))
    TS._hold(value, (c, q), (mu, var), ref, y, tag)


_default = {}


def default_run(ctx, name, method):
    if (name, method) not in _default:
        _default[name, method] = fit_predict(ctx, name, method)[0]
    return _default[name, method]


# ------------------------------------------------------------------------------------------------ fit and prediction
@pytest.mark.parametrize("method", METHODS)
@pytest.mark.parametrize("route", list(ROUTES))
@pytest.mark.parametrize("name", ["MID", "P600"])
def test_route_matches_the_mirror_and_itself(rctx, name, route, method):
    with options(rctx, ROUTES[route]):
        a, ref, y = fit_predict(rctx, name, method)
        b, _, _ = fit_predict(rctx, name, method)
    hold(a, ref, y, "%s %s %s" % (name, route, method))
    assert same_bits(a, b)
    if route in SAME_BITS_AS_DEFAULT:
        assert same_bits(a, default_run(rctx, name, method))


# ---------------------------------------------------------------------------------------------------------- gradient
@pytest.mark.parametrize("route", list(ROUTES))
@pytest.mark.parametrize("name", ["MID", "P600"])
def test_gradient_on_every_route(rctx, name, route):
    """VFE with per-dimension lengthscales: inverse_transposed of L_B and of L clips rows to min(m, k + nb) once the factor
    has more than one block, and the seven neg_products run on the route's GEMM kernel"""
    try:
        with options(rctx, ROUTES[route]):
            a, ref, bars = gradient(rctx, name)
            b, _, _ = gradient(rctx, name)
    finally:
        rctx.set_lengthscales(None)
    TG._hold(a, ref, bars, "%s %s gradient" % (name, route))
    assert TG._same_bits(a, b)
    if route == "default":
        _default.setdefault((name, "gradient"), a)
    elif route in SAME_BITS_AS_DEFAULT:                      # inverse_transposed is solve_sweep_factor too
        if (name, "gradient") not in _default:
            try:
                _default[name, "gradient"] = gradient(rctx, name)[0]
            finally:
                rctx.set_lengthscales(None)
        assert TG._same_bits(a, _default[name, "gradient"])


# ------------------------------------------------------------------------------------------------- the resident factors
@pytest.mark.parametrize("name", ["MID", "P600"])
def test_consumers_use_the_leaves_of_the_resident_factors(rctx, name):
    """sparse_fit_impl records panel_fused as sp_fused; sparse_predict_impl and sparse_grad_impl install it again, so a
    prediction and a gradient taken after the option was flipped equal, bit for bit, those taken under the option of
    the fit"""
    for fit_with in (0, 1):
        for method in METHODS:
            with options(rctx, {"panel_fused": fit_with}):
                N, d, m, noise = PROBLEMS[name]
                X, y, Z, Xs, ref = TS._mirror(N, d, m, noise, method)
                value = rctx.sparse_fit(X, y, Z, S.SIGMA, S.ELL, noise, method=method, lengthscales=None)
                want = rctx.sparse_predict(Xs, want_sd=False)
                want_g = rctx.sparse_grad() if method == "vfe" else None
                rctx.set_option("panel_fused", 1 - fit_with)
                got = rctx.sparse_predict(Xs, want_sd=False)
                got_g = rctx.sparse_grad() if method == "vfe" else None
                state = rctx.sparse_state()
            assert np.array_equal(want[0], got[0]) and np.array_equal(want[1], got[1])
            assert want_g is None or TG._same_bits(want_g, got_g)
            hold((value, state, got), ref, y, "%s %s fit with panel_fused %d, predicted with %d" % (name, method, fit_with, 1 - fit_with))
        try:
            with options(rctx, {"panel_fused": fit_with}):
                want_g, ref, bars = gradient(rctx, name)
                rctx.set_option("panel_fused", 1 - fit_with)
                got_g = rctx.sparse_grad()
        finally:
            rctx.set_lengthscales(None)
        assert TG._same_bits(want_g, got_g)
        TG._hold(got_g, ref, bars, "%s fit with panel_fused %d, gradient with %d" % (name, fit_with, 1 - fit_with))


def test_options_changed_after_the_fit(rctx):
    """P600 fitted under nb = 128 with the deep lookahead choreography and consumed under the defaults (one 512-wide block
    and a 128-wide one, no lookahead), and the reverse: the resident factors do not depend on how they are swept"""
    changed = dict(ROUTES["nb128"], **ROUTES["la256_deep"])
    N, d, m, noise = PROBLEMS["P600"]
    for fit_opts, use_opts, tag in ((changed, {}, "fit nb128 + la256_deep, consumed by default"),
                                    ({}, changed, "fit by default, consumed under nb128 + la256_deep")):
        for method in METHODS:
            X, y, Z, Xs, ref = TS._mirror(N, d, m, noise, method)
            with options(rctx, fit_opts):
                value = rctx.sparse_fit(X, y, Z, S.SIGMA, S.ELL, noise, method=method, lengthscales=None)
            with options(rctx, use_opts):
                pred = rctx.sparse_predict(Xs, want_sd=False)
                state = rctx.sparse_state()
            hold((value, state, pred), ref, y, "P600 %s %s" % (method, tag))
        X, y, Z, r, ref, bars = TG._reference(N, d, m, noise, 1)
        try:
            with options(rctx, fit_opts):
                rctx.sparse_fit(X, y, Z, S.SIGMA, S.ELL, noise, method="vfe", lengthscales=r)
            with options(rctx, use_opts):
                g = rctx.sparse_grad()
        finally:
            rctx.set_lengthscales(None)
        TG._hold(g, ref, bars, "P600 gradient %s" % tag)


# ------------------------------------------------------------------------------------------------------ the Gram plan
@pytest.mark.parametrize("method", METHODS)
@pytest.mark.parametrize("name,slab,route", EDGES)
def test_gram_plan_edges(rctx, name, slab, route, method):
    """chunks of several units, a shorter last chunk, 171 and 45 tiles, a last slab with more splits than the full one
    (the table of the module docstring; tests/test_sparse_routes_cpu.py holds it against the plan header).  No gradient:
    its long-double mirror would take minutes at these shapes."""
    with options(rctx, dict(GEMM_ROUTES[route], sparse_slab=slab)):
        a, ref, y = fit_predict(rctx, name, method)
        b, _, _ = fit_predict(rctx, name, method)
    hold(a, ref, y, "%s slab=%d %s %s" % (name, slab, route, method))
    assert same_bits(a, b)


def test_ragged_last_slab(rctx):
    """N = 641, m = 130 under sparse_slab = 512: a slab of 512 rows and one of 256 (129 real) -- the slabs of
    tests/test_sparse_gpu.py::test_slabs all divide the 768 padded rows"""
    shape, slab = LAST_SLAB
    with options(rctx, {"sparse_slab": slab}):
        for method in METHODS:
            a, ref, y = fit_predict(rctx, None, method, shape)
            hold(a, ref, y, "N=641 m=130 slab=%d %s" % (slab, method))
        try:
            g, ref, bars = gradient(rctx, None, shape)
        finally:
            rctx.set_lengthscales(None)
    TG._hold(g, ref, bars, "N=641 m=130 slab=%d gradient" % slab)
