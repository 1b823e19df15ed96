"""Regression prediction and the posterior-sample factor on every factor route and GEMM route, each form held to an
independent reference (tests/predict_ref.py) and not to another form:

    two_call    gpmi_factorize, gpmi_predict_resident (solve_sweep_factor with tri = false and m = np_ rows), then
                gpmi_post_chol and gpmi_post_sample at both jitters: rbf_sym on the test set, one gemm_minus_lower of
                depth K = Np that reads v from V, a cholesky_inplace with no riding row in P (ldP = np_ + 32)
    one_pass    gpmi_fit_predict_resident: the test rows ride through the Cholesky below the y rows (nrows = Np + 128 + np_),
                row_dots_kernel off the finished rows; the posterior GEMM reads v from the rows of A
    augmented   gpmi_fit_predict_sample_resident at jitter 1e-6: one Cholesky of Np + np_ columns, the y rows behind the
                test rows; post_chol(1e-6) fetches the factor from behind L, post_chol(1e-2) forms it in P

Problems SMALL, MID and BIG, their lengthscales and the routes are those of tests/test_postfit_routes_gpu.py.  Test points
from default_rng(15), uniform in [0, 4)^d with every third point in [3, 5)^d: a third leave the training box, so the
variances span 3e-5 .. 0.14 and |mu| reaches 20 (MID).  Z = default_rng(7).standard_normal((n, 17)): two full passes of
tri_mul_kernel<8> and a pass of one.

    SMALL  n 37    np_ 128   one test tile with 37 real rows; the posterior factor is one leaf
    SMALL  n 300   np_ 384   augmented ncols = 1152: the block 512..1024 straddles the K / K_ss boundary at 768
    SMALL  n 700   np_ 768   more test than training points
    MID    n 700   np_ 768   the boundary on a block edge (1536); augmented ncols = 2304 ends in a half block
    BIG    n 1000  np_ 1024  the rectangular sweep's first update 1024 x 2560 (160 tiles), carried rows 4224, augmented 4096
    BIG    n 2100  np_ 2176  m >= 2048: beside_update in the lookahead sweep; the posterior GEMM 2176 x 2176 lower at K = 3072
    FULL   n 256   np_ 256   N = 768: no padding anywhere.  At the three problems above the last 16 columns of L and v are
                             padding, so a sum that lost its last K step would lose zeros; here it loses 4e-3 of Sigma
                             (tests/test_predict_routes_cpu.py does that to a float64 evaluation)

Reference: predict_ref.predict in long double at SMALL, MID and FULL, float64 by LAPACK at BIG (long double takes minutes
there).  Bars: lml, alpha, m, diag and mu keep LML_RTOL, ALPHA_RTOL, M_RTOL, DIAG_RTOL and MU_ATOL x max(1, max|mu|) of
tests/test_parity_gpu.py.  The variance and, per jitter, Sigma (as L_ L_^T), L_ and L_ @ Z are new quantities: 10 x what
the worse of two float64 evaluations misses of the long-double one (FLOAT64_MISS; at BIG 10 x the distance of the two,
FLOAT64_APART), the rule of tests/test_sparse_grad_gpu.py::_reference, and never above VAR_ATOL, 1e-10 and FPOST_ATOL.
That puts L_ at 1e-10 (jitter 1e-6, cond Sigma up to 4e6) and 1e-12 (jitter 1e-2) where the suite had 1e-6 and 1e-7.
tests/test_predict_routes_cpu.py measures both tables again.  hold() prints error / bar of every quantity before it
asserts.

Routes.  SMALL, MID and FULL: the twelve of tests/test_classify_routes_gpu.py.  Their launches have fewer than 128 tiles
of 128 x 128 -- with one exception per block size, all trailing updates of a Cholesky on chol_trailing_update_dma_kernel:
MID's augmented factorisation (2304 columns, 2432 rows: 1920 x 1792 at blocks of 512), and under nb = 128 and nb = 256 the
first updates of MID's carried and augmented forms and of SMALL n = 700's augmented form
(tests/test_predict_routes_cpu.py::LARGE_BELOW_BIG lists them).  BIG (BIG_ROUTES) is there for the 128-tile LDS-DMA
family; tests/test_predict_routes_cpu.py asks gemm_route for the kernel of every launch and records the answers:

    default          the sweep's updates (1024 x 2560 x K512 down to m x 1024) on gemm_nt_dma_kernel<2, false>; the carried
                     and augmented trailing updates on chol_trailing_update_dma_kernel, the first ones (3712 x 2560 and
                     up: two rounds of blocks) on chol_trailing_update_persist_kernel; at n = 2100 the posterior GEMM on
                     gemm_nt_dma_kernel<2, false> and the posterior Cholesky's first update (1664 x 1664) on the trailing kernel
    la256_deep/_shallow   every update split in two, chip shared: no persistent form, so the same launches on
                     chol_trailing_update_dma_kernel -- the pair that isolates gemm_persist here, compared bit for bit;
                     at n = 2100 the sweep runs beside_update (gemm_nt_small_kernel<3>), at n = 1000 and_chip_shared
    tall, tall_nb1024     each of those on the 256 x 128 forms gemm_nt_dma_tall_kernel<false> and
                     chol_trailing_update_dma256_kernel, the posterior GEMM included
    ticket2_nb2048   at n = 2100 the panel update 4352 x 1024 x K1024 on gemm_nt_dma_ticket_kernel and the augmented
                     trailing update 3328 x 3200 x K2048 on chol_trailing_update_ticket_kernel
    nb3072, persist0_nb3072   one block of 3072: the sweep is one trsm_block whose inner update (m x 1536 x K1536) reaches
                     the family; no launch of this side has two rounds, so the two routes launch the same kernels here

Exact statements, every route: each form gives the same bits twice; post_chol is lower triangular; the standard
deviation is the square root of the variance bit for bit; post_sample is the downloaded factor times Z to 1e-13 x
max(1, max|L_ Z|) x sqrt(n); the lookahead routes give the bits of the default route, form by form; lml, m, diag and
alpha of one_pass equal two_call's bit for bit -- the carried rows never enter L, although they move launches of the fit
over the 128-tile line onto other kernels (tests/test_predict_routes_cpu.py names them): every kernel of the update GEMM
adds the K steps of a tile in the same order.

No (problem, test set, route) is skipped, and none is expected to fail."""
import functools

import numpy as np
import pytest

import ard_ref
import predict_ref as P
import test_parity_gpu as TP
from test_postfit_routes_gpu import (BIG_ROUTES, DEFAULTS, ELL, PROBLEMS, ROUTES, SAME_BITS_AS_DEFAULT, SIGMA, inputs,   # noqa: F401
                                     options)

pytestmark = pytest.mark.gpu

LD = np.longdouble
# FULL: one more problem, N and n multiples of 128.  At SMALL, MID and BIG the last 16 columns of the factor, and of v, are
# padding (1, 92 and 6 real rows in the last tile): a kernel that lost the last K step of a sum would lose zeros there
SIZES = dict(PROBLEMS, FULL=(768, 5, 5e-4))                     # N, d, noise
TEST_SETS = {"SMALL": (37, 300, 700), "MID": (700,), "BIG": (1000, 2100), "FULL": (256,)}
JITTERS = (1e-6, 1e-2)
NFUN = 17                     # two full passes of tri_mul_kernel<8> and a pass of one
FORMS = ("two_call", "one_pass", "augmented")
LONG_DOUBLE = ("SMALL", "MID", "FULL")  # the problems whose reference is the long-double evaluation
CASES = [(name, n, route) for name in SIZES for n in TEST_SETS[name] for route in (BIG_ROUTES if name == "BIG" else ROUTES)]
PER_JITTER = tuple("%s@%g" % (k, j) for j in JITTERS for k in P.PER_JITTER)
NEW = ("var",) + PER_JITTER             # the quantities no other module has a measured bar for
# the plain bars: those of tests/test_parity_gpu.py -- for the new quantities the ceilings no measured bar may exceed
PLAIN = dict(lml=TP.LML_RTOL, alpha=TP.ALPHA_RTOL, m=TP.M_RTOL, diag=TP.DIAG_RTOL, mu=TP.MU_ATOL, var=TP.VAR_ATOL)
PLAIN.update({k: 1e-10 if k.startswith("Sigma") else TP.FPOST_ATOL for k in PER_JITTER})

# What float64 itself misses of the long-double evaluation, in the normalisation of predict_ref.errors: the worse of the
# LAPACK and the blocked evaluation, measured on the CPU; tests/test_predict_routes_cpu.py measures both again and holds
# this table within a factor 2
FLOAT64_MISS = {
    ("SMALL", 37): {"lml": 1.6e-12, "alpha": 3.1e-11, "m": 2.5e-11, "diag": 8.6e-14, "mu": 6.5e-12, "var": 3.7e-14,
                    "Sigma@1e-06": 3.8e-14, "L_@1e-06": 6.0e-13, "LZ@1e-06": 2.1e-12,
                    "Sigma@0.01": 3.8e-14, "L_@0.01": 1.0e-13, "LZ@0.01": 3.2e-13},
    ("SMALL", 300): {"lml": 1.6e-12, "alpha": 3.1e-11, "m": 2.5e-11, "diag": 8.6e-14, "mu": 6.2e-12, "var": 3.7e-14,
                     "Sigma@1e-06": 3.8e-14, "L_@1e-06": 1.3e-11, "LZ@1e-06": 9.0e-11,
                     "Sigma@0.01": 3.8e-14, "L_@0.01": 1.3e-13, "LZ@0.01": 9.0e-13},
    ("SMALL", 700): {"lml": 1.6e-12, "alpha": 3.1e-11, "m": 2.5e-11, "diag": 8.6e-14, "mu": 5.7e-12, "var": 5.9e-14,
                     "Sigma@1e-06": 6.2e-14, "L_@1e-06": 2.3e-11, "LZ@1e-06": 1.9e-10,
                     "Sigma@0.01": 6.1e-14, "L_@0.01": 1.7e-13, "LZ@0.01": 9.8e-13},
    ("MID", 700): {"lml": 2.8e-12, "alpha": 7.3e-11, "m": 5.8e-11, "diag": 9.6e-14, "mu": 1.5e-11, "var": 7.2e-14,
                   "Sigma@1e-06": 7.6e-14, "L_@1e-06": 1.1e-11, "LZ@1e-06": 7.6e-11,
                   "Sigma@0.01": 7.6e-14, "L_@0.01": 1.8e-13, "LZ@0.01": 1.3e-12},
    ("FULL", 256): {"lml": 2.3e-12, "alpha": 3.1e-11, "m": 2.3e-11, "diag": 9.1e-14, "mu": 1.0e-11, "var": 4.5e-14,
                    "Sigma@1e-06": 4.5e-14, "L_@1e-06": 8.6e-12, "LZ@1e-06": 4.5e-11,
                    "Sigma@0.01": 4.5e-14, "L_@0.01": 1.6e-13, "LZ@0.01": 8.9e-13},
}
# BIG: how far the blocked float64 evaluation is from the LAPACK one (the reference there), measured the same way.  No
# evaluation here is more exact than float64, so the distance of the two says what float64 misses only of the operations
# they round differently -- and the largest part of that miss is the rounding of K itself, which two evaluations from the
# same bits of K share.  So the blocked one takes its covariance from predict_ref.kernel_other_rounding.  Measured once
# in long double at n = 1000 (2.5 minutes on the CPU, not part of any test): float64 misses L_ by 5.1e-11 (jitter 1e-6)
# and 5.8e-14 (1e-2), L_ @ Z by 5.0e-10 and 7.6e-13, Sigma by 6.3e-15, the variance by 3.7e-15, LAPACK and blocked alike;
# from the same bits of K the two are 5.6e-12, 8.3e-15, 6.6e-11, 1.3e-13, 2.2e-15 and 2.4e-15 apart, up to eight times
# closer to each other than to the truth; with the covariance rounded otherwise, the figures below: within 1.6 x of the miss
FLOAT64_APART = {
    ("BIG", 1000): {"lml": 1.0e-14, "alpha": 2.1e-13, "m": 1.4e-13, "diag": 5.6e-15, "mu": 4.5e-14, "var": 2.9e-15,
                    "Sigma@1e-06": 4.6e-15, "L_@1e-06": 3.8e-11, "LZ@1e-06": 3.1e-10,
                    "Sigma@0.01": 4.6e-15, "L_@0.01": 4.1e-14, "LZ@0.01": 5.8e-13},
    ("BIG", 2100): {"lml": 1.0e-14, "alpha": 2.1e-13, "m": 1.4e-13, "diag": 5.6e-15, "mu": 4.4e-14, "var": 3.3e-15,
                    "Sigma@1e-06": 4.8e-15, "L_@1e-06": 3.6e-11, "LZ@1e-06": 4.1e-10,
                    "Sigma@0.01": 4.8e-15, "L_@0.01": 5.0e-14, "LZ@0.01": 9.0e-13},
}


def bars(name, n):
    """-> {quantity: bar}.  lml, alpha, m, diag and mu keep the bars of tests/test_parity_gpu.py.  The variance and, per
    jitter, Sigma, L_ and L_ @ Z are new quantities: 10 x what float64 itself misses on the CPU (at BIG: 10 x the distance
    of the two float64 evaluations), the rule of tests/test_sparse_grad_gpu.py::_reference, and never above the plain bar"""
    table = (FLOAT64_MISS if name in LONG_DOUBLE else FLOAT64_APART)[name, n]
    return {k: min(10.0 * table[k], PLAIN[k]) if k in NEW else PLAIN[k] for k in PLAIN}


def problem_inputs(name):
    """-> X, y, r: inputs(name) of tests/test_postfit_routes_gpu.py, and FULL drawn the same way"""
    if name != "FULL":
        return inputs(name)
    N, d, _ = SIZES[name]
    X, y = ard_ref.problem(N, d, seed=100 + d)
    return X, y, np.random.default_rng(7 + d).uniform(0.5, 3.0, d) * np.sqrt(d)


def points_at(name, n):
    """a third of the points leave the training box [0, 4)^d"""
    g = np.random.default_rng(15)
    Xs = g.uniform(0.0, 4.0, (n, SIZES[name][1]))
    Xs[2::3] = g.uniform(3.0, 5.0, Xs[2::3].shape)
    return Xs


def normals(n):
    return np.random.default_rng(7).standard_normal((n, NFUN))


@functools.lru_cache(maxsize=None)
def reference_fit(name, dtype):
    X, y, r = problem_inputs(name)
    return P.fit(X, y, r, SIGMA, ELL, SIZES[name][2], dtype)


@functools.lru_cache(maxsize=None)
def reference(name, n):
    """predict_ref.predict in long double (SMALL, MID) or float64 by LAPACK (BIG): one evaluation per (problem, test set),
    one factorisation per problem, shared and left unchanged"""
    return P.predict(reference_fit(name, LD if name in LONG_DOUBLE else np.float64), points_at(name, n), JITTERS, normals(n))


@pytest.fixture(scope="module")
def qctx():
    """a context of this module's own: lengthscales, the test set and options are context state"""
    from gaussian_process_amd import GPContext
    c = GPContext(0)
    yield c
    c.close()


# --------------------------------------------------------------------------------------------------------- the forms
def resident(ctx, name, n):
    X, y, r = problem_inputs(name)
    ctx.set_train(X, y)
    ctx.set_lengthscales(r)
    ctx.set_test(points_at(name, n))


def posterior(ctx, Z, jitters=JITTERS):
    return {j: dict(L_=ctx.post_chol(j), LZ=ctx.post_sample(j, Z)) for j in jitters}


def state(ctx):
    return dict(alpha=ctx.alpha(), m=ctx.m(), diag=ctx.diag())


def two_call(ctx, name, Z):
    """the factor is formed in P at both jitters; the posterior GEMM reads v from V"""
    lml = ctx.factorize(SIGMA, ELL, SIZES[name][2])
    mu, var = ctx.predict_resident(want_sd=False)
    out = dict(lml=lml, mu=mu, var=var, post=posterior(ctx, Z), **state(ctx))
    out["sd"] = ctx.predict_resident(want_sd=True)
    return out


def one_pass(ctx, name, Z):
    """the test rows ride through the Cholesky below the y rows; the posterior GEMM reads v from the rows of A"""
    lml, mu, var = ctx.fit_predict_resident(SIGMA, ELL, SIZES[name][2], want_sd=False)
    return dict(lml=lml, mu=mu, var=var, post=posterior(ctx, Z), **state(ctx))


def augmented(ctx, name, Z):
    """one Cholesky of the augmented matrix at the first jitter: that factor is fetched from behind L, the other is
    formed in P from the rows of A"""
    lml, mu, var, L_ = ctx.fit_predict_sample_resident(SIGMA, ELL, SIZES[name][2], JITTERS[0], want_sd=False)
    out = dict(lml=lml, mu=mu, var=var, post=posterior(ctx, Z), **state(ctx))
    out["returned"] = L_
    return out


RUN = dict(two_call=two_call, one_pass=one_pass, augmented=augmented)


def run(ctx, name, n):
    """-> {form: its results}"""
    try:
        resident(ctx, name, n)
        Z = normals(n)
        return {f: RUN[f](ctx, name, Z) for f in FORMS}
    finally:
        ctx.set_lengthscales(None)


def flat(out):
    """every number of one form's results, for bit comparisons"""
    parts = [[out["lml"]], out["mu"], out["var"], out["alpha"], out["m"], out["diag"]]
    parts += [out["post"][j][k].ravel() for j in sorted(out["post"]) for k in ("L_", "LZ")]
    parts += [a.ravel() for a in out.get("sd", ())] + ([out["returned"].ravel()] if "returned" in out else [])
    return np.concatenate([np.asarray(p, dtype=np.float64) for p in parts])


def same_bits(a, b):
    fa, fb = flat(a), flat(b)
    return fa.shape == fb.shape and np.array_equal(fa, fb, equal_nan=True)


def hold(out, name, n, tag):
    """prints error / bar of every quantity (the measured headroom), then asserts each against the reference"""
    err, bar = P.errors(out, reference(name, n)), bars(name, n)
    assert sorted(err) == sorted(bar), tag
    ratio = {k: err[k] / bar[k] for k in bar}
    print("%s: error / bar  " % tag + "  ".join("%s %.2e" % kv for kv in ratio.items()) + "  worst %.2e" % max(ratio.values()))
    assert np.all(np.isfinite(flat(out))), tag
    for k in bar:
        assert err[k] <= bar[k], (tag, k, err[k], bar[k])


def exact(out, n, tag):
    """what holds exactly, or to the rounding of one product, whatever the route"""
    Z = normals(n)
    for j, p in out["post"].items():
        assert p["L_"].shape == (n, n) and np.array_equal(p["L_"], np.tril(p["L_"])), (tag, j)
        want = p["L_"] @ Z
        gap = np.max(np.abs(p["LZ"] - want))
        assert gap <= 1e-13 * max(1.0, np.abs(want).max()) * n ** 0.5, (tag, j, gap)     # test_post_sample_is_the_factor_times_the_normals
    if "sd" in out:
        with np.errstate(invalid="ignore"):
            assert np.array_equal(out["sd"][1], np.sqrt(out["var"]), equal_nan=True), tag
        assert np.array_equal(out["sd"][0], out["mu"]), tag
    if "returned" in out:
        assert np.array_equal(out["returned"], out["post"][JITTERS[0]]["L_"]), tag       # the resident factor, downloaded again


def fit_bits(out):
    return np.concatenate([[out["lml"]], out["m"], out["diag"], out["alpha"]])


_default = {}


def default_run(ctx, name, n):
    if (name, n) not in _default:
        _default[name, n] = run(ctx, name, n)
    return _default[name, n]


# ------------------------------------------------------------------------------------------------------ every route
@pytest.mark.parametrize("name,n,route", CASES)
def test_every_form_matches_the_reference_and_itself(qctx, name, n, route):
    with options(qctx, (BIG_ROUTES if name == "BIG" else ROUTES)[route]):
        a = run(qctx, name, n)
        b = run(qctx, name, n)
    for f in FORMS:
        tag = "%s n=%d %s %s" % (name, n, route, f)
        hold(a[f], name, n, tag)
        exact(a[f], n, tag)
        assert same_bits(a[f], b[f]), tag
    # the carried rows never enter L
    assert np.array_equal(fit_bits(a["one_pass"]), fit_bits(a["two_call"])), (name, n, route)
    if route == "default":
        _default.setdefault((name, n), a)
    elif route in SAME_BITS_AS_DEFAULT:
        base = default_run(qctx, name, n)
        for f in FORMS:
            assert same_bits(a[f], base[f]), (name, n, route, f)


# --------------------------------------------------------------------------------------------- the resident factor
def test_predictions_use_the_leaves_of_the_resident_factor(qctx):
    """factorize_impl records panel_fused with the factor (Resident::factor_fused) and gpmi_predict_resident installs it
    again (resident_tuning): the rectangular sweep keeps the leaves of the fit whatever the option says by then, so mean,
    variance and standard deviation equal, bit for bit, those taken under the option of the fit.  The regression
    counterpart of tests/test_classify_routes_gpu.py::test_predict_uses_the_leaves_of_the_resident_factor.

    The posterior factor is not part of that statement: gpmi_post_chol and gpmi_post_sample run a factorisation of their
    own, which takes the context's options by design (csrc/gpmi_api.hip, above gpmi_lml_grad) -- under the other option
    it has the other leaves and other bits (measured: L_ 8e-14 apart at jitter 1e-6, 7e-16 at 1e-2).  Here it is held to the reference
    under both options, from the same bits of v, and back under the first option it has its first bits again"""
    name, n = "MID", 700
    Z = normals(n)

    def calls(lml, st):
        mu, var = qctx.predict_resident(want_sd=False)
        return dict(mu=mu, var=var, sd=qctx.predict_resident(want_sd=True), post=posterior(qctx, Z), lml=lml, **st)

    for fit_with in (0, 1):
        tag = "%s n=%d fit with panel_fused %d, prediction under %d" % (name, n, fit_with, 1 - fit_with)
        try:
            with options(qctx, {"panel_fused": fit_with}):
                resident(qctx, name, n)
                lml = qctx.factorize(SIGMA, ELL, SIZES[name][2])
                st = state(qctx)
                want = calls(lml, st)
                qctx.set_option("panel_fused", 1 - fit_with)
                got = calls(lml, st)
                qctx.set_option("panel_fused", fit_with)
                back = calls(lml, st)
        finally:
            qctx.set_lengthscales(None)
        for k in ("mu", "var"):
            assert np.array_equal(want[k], got[k]), (tag, k)
        assert np.array_equal(want["sd"][1], got["sd"][1], equal_nan=True), tag
        assert same_bits(want, back), tag
        for out, which in ((want, "the fit's option"), (got, "the other option")):
            hold(out, name, n, "%s: %s" % (tag, which))
            exact(out, n, tag)
        print("%s: L_ under the two options max %s apart" % (
            tag, ", ".join("%.2e at jitter %g" % (np.max(np.abs(want["post"][j]["L_"] - got["post"][j]["L_"])), j) for j in JITTERS)))


# ------------------------------------------------------------------------------------------------ a bad posterior pivot
@pytest.mark.parametrize("route", ["nb128", "la256_deep"])
def test_a_bad_posterior_pivot_is_reported_and_leaves_the_context_usable(qctx, route):
    """K_ss - 0.5 I - v^T v is not positive definite: the same LinAlgError from the factorisation in P and from the
    augmented one, where the bad-pivot word covers two matrices (the block column 512..1024 of the 1152 augmented columns
    straddles K and K_ss under la256_deep); every form afterwards holds its bars"""
    name, n = "SMALL", 300
    try:
        with options(qctx, ROUTES[route]):
            resident(qctx, name, n)
            qctx.factorize(SIGMA, ELL, SIZES[name][2])
            qctx.predict_resident()
            with pytest.raises(np.linalg.LinAlgError) as in_p:
                qctx.post_chol(-0.5)
            with pytest.raises(np.linalg.LinAlgError) as riding:
                qctx.fit_predict_sample_resident(SIGMA, ELL, SIZES[name][2], -0.5)
            # the first pivot already: sigma^2 - 0.5 - |v_0|^2 = var_0 - 0.5, and no variance here reaches 0.05
            assert str(riding.value) == str(in_p.value) and riding.value.bad_pivot == in_p.value.bad_pivot == 1
            Z = normals(n)
            after = {f: RUN[f](qctx, name, Z) for f in ("augmented", "two_call", "one_pass")}
    finally:
        qctx.set_lengthscales(None)
    for f, out in after.items():
        tag = "%s n=%d %s %s after a bad pivot" % (name, n, route, f)
        hold(out, name, n, tag)
        exact(out, n, tag)

