"""What works from a resident fit, on every factor route: gpmi_get_alpha, gpmi_lml_grad, gpmi_lml_grad_ard, gpmi_loo and
gpmi_loo_grad (csrc/regress.hip), once each gpmi_lml_grad_co2 and a Matern gradient, and the classifiers' gpmi_laplace_grad
and gpmi_softmax_grad.  All of them run the backward solve (backward_solve_rhs: three trsv_vinv forms on a fused factor,
launch_trsv_lt on a first-generation one), inverse_transposed (solve_sweep_factor with tri = true on the identity),
neg_gram_lower or neg_gram_lower_dense (the routed GEMM with lower, diag_off = r0, K = n - r0), and gpmi_loo_grad a
row-block product K_y^-1 D on top.  The other modules drive these calls under nb in {128, 256, 0} alone.

Problems, from ard_ref.problem(N, d, seed = 100 + d) with the relative lengthscales of tests/test_ard_gpu.py::_mirror,
sigma 1.2, l 1.3:

    SMALL   N 641  d 5  noise 5e-4   Np 768: six tiles, the last holds one real row
    MID     N 1500 d 8  noise 5e-4   Np 1536: three blocks of 512, twelve under nb = 128; 92 real rows in the last tile
    BIG     N 2950 d 4  noise 1e-1   Np 3072: 24 tiles, the last holds 6 real rows.  It exists to reach kernels, not to
                                     stress conditioning: cond K_y is 2e4, and tests/test_postfit_routes_cpu.py holds two
                                     independent float64 evaluations of its mirror to a tenth of every bar below (worst:
                                     0.03 of the LOO log-probability bar; at noise 1e-2, cond 2e5, they were 0.74 of that
                                     bar apart, so the noise was raised, not the bar)

One mirror per problem and session: ard_ref.lml_and_grad plus loo_ref.closed with the same r (SMALL and MID share
test_ard_gpu's evaluation).  Bars: none is new.  LML: LML_RTOL.  alpha: ALPHA_RTOL of tests/test_parity_gpu.py.
gpmi_lml_grad_ard: test_ard_gpu._hold_gradient (GRAD_RTOL x each component's cancellation scale); gpmi_lml_grad's two
components at the same g_l, g_sigma and scales.  LOO: _hold_values and _hold_gradient of tests/test_loo_gpu.py -- with one
fallback: at SMALL and MID float64 itself misses _hold_values' bar of the log probabilities (and, at MID, of the means)
against long double, on the CPU, so there the LOO values are held to a long-double evaluation with 10 x float64's own miss
where it exceeds the plain bar, the rule of tests/test_sparse_grad_gpu.py::_reference (loo_reference below has the
figures).  hold() prints error / bar of every quantity before it asserts.

Routes.  SMALL and MID: the twelve of tests/test_classify_routes_gpu.py (the three trsv_vinv forms included); every
launch of theirs has fewer than 128 tiles of 128 x 128, where gemm_tall, gemm_ticket and gemm_persist cannot change a
kernel.  BIG (BIG_ROUTES) is there for the 128-tile LDS-DMA family; tests/test_postfit_routes_cpu.py asks gemm_route
(csrc/gpmi_route.h) for the kernel of every launch under every route and records the answers.  In short:

    default          blocks of 512, no lookahead below 6144 columns: the tri sweep's updates 1024 x 2048, 1536 x 1536 and
                     2048 x 1024 (K 512) run on gemm_nt_dma_kernel<2, false>; the neg_gram_lower row blocks (4 x 24 tiles
                     at most) and the LOO product (4 x 24) stay on the 64 x 64 ring
    nb1024           production's block from 12288 columns on: neg_gram_lower's row blocks 1024 x 2048 (K 2048, diag_off
                     1024) and 1024 x 3072 (K 1024, diag_off 2048), the LOO product 1024 x 3072 x 3072 three times and
                     two sweep updates, all on gemm_nt_dma_kernel<2, false>
    la256_deep/_shallow   lookahead in the tri sweep with m = 3072 >= 2048 rows: Sharing::beside_update, every split
                     update on gemm_nt_small_kernel<3> (SMALL and MID take and_chip_shared under the same routes)
    tall, tall_nb1024     gemm_tall = 1 with tall_min_tiles = 0: each launch named above on gemm_nt_dma_tall_kernel<false>
    ticket2_nb2048   gemm_ticket = 2 needs one round of 256 blocks, which blocks of 512 and 1024 do not give (at most 192
                     tiles): under nb = 2048 the LOO product's first row block (2048 x 3072 x 3072, 384 tiles) runs on
                     gemm_nt_dma_ticket_kernel
    nb3072, persist0_nb3072   gemm_persist (1 by default) needs two rounds: one block of 3072 makes the LOO product
                     3072 x 3072 x 3072 = 576 tiles, on gemm_nt_dma_persist_kernel -- and, under gemm_persist = 0, on
                     gemm_nt_dma_kernel<2, false>.  The tri sweep is then one trsm_block whose inner updates
                     (3072 x 1536 x 1536) are the launches that reach the family

Bit equality BETWEEN routes is asserted for the lookahead routes alone (la_min: "same bits").

Classifier gradients: binary641 and softmax641_C3 of tests/test_classify_routes_gpu.py (isotropic, sigma 1.5, l 3.0) on
the twelve routes, fitted with tol = 1e-13, against the mirrors of tests/laplace_grad_ref.py and tests/softmax_grad_ref.py
computed once here.  No case of tests/test_laplace_grad_gpu.py or tests/test_softmax_grad_gpu.py has this shape, so the
bars are those modules' rule -- gpu_bar: 50 x the mirror's own response to rounding in K, floored at 1e-11 -- applied to
the figures measured for these two problems with their rounding_figure (CLASSIFIER_ROUNDING: 2.6e-15 and 7.5e-14, so
both bars are the floor, 1e-11).

No (problem, route) pair is skipped, and none is expected to fail."""
import functools

import numpy as np
import pytest
from scipy.linalg import solve_triangular

import ard_ref as R
import laplace_grad_ref as LG
import loo_ref as LR
import sgpr_ref as S
import softmax_grad_ref as SG
import test_ard_gpu as TA
import test_classify_routes_gpu as CR
import test_co2_grad_gpu as TC
import test_laplace_grad_gpu as TLG
import test_loo_gpu as TL
import test_matern_gpu as TM
import test_parity_gpu as TP
from conftest import golden
from test_laplace_grad_cpu import FIT_TOL, gpu_bar

pytestmark = pytest.mark.gpu

SIGMA, ELL = 1.2, 1.3
PROBLEMS = {"SMALL": (641, 5, 5e-4), "MID": (1500, 8, 5e-4), "BIG": (2950, 4, 1e-1)}       # N, d, noise
DEFAULTS = dict(CR.DEFAULTS, gemm_tall=1, tall_min_tiles=12288, gemm_ticket=0, gemm_persist=1)
ROUTES = CR.ROUTES
assert list(ROUTES) == ["default", "nb128", "nb256", "lookahead0", "la256_deep", "la256_shallow", "panel_fused0", "trsv_vinv0",
                        "trsv_vinv1", "trsv_vinv2", "small_tiles0", "small_dma0"]
SAME_BITS_AS_DEFAULT = CR.SAME_BITS_AS_DEFAULT
TALL = {"gemm_tall": 1, "tall_min_tiles": 0}
BIG_ROUTES = {
    "default": {},
    "nb1024": {"nb": 1024},
    "la256_deep": ROUTES["la256_deep"],
    "la256_shallow": ROUTES["la256_shallow"],
    "tall": TALL,
    "tall_nb1024": dict(TALL, nb=1024),
    "ticket2_nb2048": {"gemm_ticket": 2, "nb": 2048},
    "nb3072": {"nb": 3072},                                   # gemm_persist = 1 is the default
    "persist0_nb3072": {"gemm_persist": 0, "nb": 3072},
}
CASES = [(name, route) for name in ("SMALL", "MID") for route in ROUTES] + [("BIG", route) for route in BIG_ROUTES]
# the classifiers' mirrors under rounding in K (rounding_figure of tests/test_laplace_grad_cpu.py and
# tests/test_softmax_grad_cpu.py, five seeds), measured on the CPU for the two problems of this module
CLASSIFIER_ROUNDING = {"binary641": 2.6e-15, "softmax641_C3": 7.5e-14}
CALLS = ("lml", "alpha", "lml_grad", "lml_grad_ard", "loo", "loo_grad")
LD = np.longdouble
LOO_LONG_DOUBLE = ("SMALL", "MID")          # the LOO values are held to a long-double evaluation there: loo_reference


@pytest.fixture(scope="module")
def pctx():
    """a context of this module's own: lengthscales, the kernel kind and options are context state"""
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


def inputs(name):
    """-> X, y, r: the problem and the relative lengthscales, drawn as tests/test_ard_gpu.py::_mirror draws them"""
    N, d, _ = PROBLEMS[name]
    X, y = R.problem(N, d, seed=100 + d)
    return X, y, np.random.default_rng(7 + d).uniform(0.5, 3.0, d) * np.sqrt(d)


@functools.lru_cache(maxsize=None)
def mirror(name):
    """-> X, y, r, ard_ref.lml_and_grad, loo_ref.closed: one evaluation per problem, shared and left unchanged"""
    N, d, noise = PROBLEMS[name]
    if noise == TA.NOISE:
        X, y, r, ard = TA._mirror(N, d, SIGMA, ELL)            # the evaluation tests/test_ard_gpu.py uses, and its cache
        assert np.array_equal(r, inputs(name)[2])
    else:
        X, y, r = inputs(name)
        ard = R.lml_and_grad(X, y, r, SIGMA, ELL, noise)
    return X, y, r, ard, LR.closed(X, y, r, SIGMA, ELL, noise)


def fit(ctx, name):
    X, y, r, _, _ = mirror(name)
    ctx.set_train(X, y)
    ctx.set_lengthscales(r)
    return ctx.factorize(SIGMA, ELL, PROBLEMS[name][2])


def post_fit(ctx):
    return dict(alpha=ctx.alpha(), lml_grad=ctx.lml_grad(), lml_grad_ard=ctx.lml_grad_ard(), loo=ctx.loo(),
                loo_grad=ctx.loo_grad())


def run(ctx, name):
    """lengthscales, the fit and the five calls behind it"""
    try:
        lml = fit(ctx, name)
        return dict(post_fit(ctx), lml=lml)
    finally:
        ctx.set_lengthscales(None)


def flat(out):
    """every number of a run, for bit comparisons"""
    parts = []
    for k in CALLS:
        if k in out:
            v = out[k]
            parts += [np.atleast_1d(np.asarray(p, dtype=np.float64)).ravel() for p in (v if isinstance(v, tuple) else (v,))]
    return np.concatenate(parts)


def same_bits(a, b):
    return sorted(a) == sorted(b) and np.array_equal(flat(a), flat(b))


LOO_PLAIN = dict(mu=1e-10, var=1e-10, logp=1e-10, total=TL.LML_RTOL)          # the bars of test_loo_gpu._hold_values


def loo_errors(got, ref, y):
    """the four errors of test_loo_gpu._hold_values, each in the normalisation it asserts; ref: mu, var, logp, loo"""
    mu, var, logp, tot = got
    f = lambda v: np.asarray(v, dtype=np.float64)               # noqa: E731
    return dict(mu=float(np.max(np.abs(f(mu - ref["mu"]))) / max(1.0, np.max(np.abs(y)))),
                var=float(np.max(np.abs(f((var - ref["var"]) / ref["var"])))),
                logp=float(np.max(np.abs(f(logp - ref["logp"])) / np.maximum(1.0, np.abs(f(ref["logp"]))))),
                total=float(abs(f(tot - ref["loo"])) / np.sum(np.abs(f(ref["logp"])))))


def loo_values(name, dtype):
    """the LOO values of loo_ref.from_Ky from the Cholesky factor, in float64 (LAPACK) or long double (the column loops of
    tests/sgpr_ref.py): K from the scaled inputs the device forms (one float64 division), L^-1 by a triangular solve on
    the identity, kappa_i the squared norm of column i of L^-1, alpha by two products with it"""
    X, y, r = inputs(name)
    N, d, noise = PROBLEMS[name]
    chol, solve_lower = S._ops(dtype)
    z = R.scaled(X, r).astype(dtype)
    sq = np.zeros((N, N), dtype=dtype)
    for k in range(d):
        sq += (z[:, None, k] - z[None, :, k]) ** 2
    Ky = dtype(SIGMA) ** 2 * np.exp(dtype(-.5) / dtype(ELL) ** 2 * sq) + dtype(noise) * np.eye(N, dtype=dtype)
    Li = solve_lower(chol(Ky), np.eye(N, dtype=dtype))
    kappa = np.sum(Li * Li, axis=0)
    alpha = Li.T @ (Li @ y.astype(dtype))
    mu, var = y - alpha / kappa, 1 / kappa
    logp = dtype(-.5) * np.log(var) - (y - mu) ** 2 / (2 * var) - dtype(.5) * np.log(2 * dtype(np.pi))
    return {"mu": mu, "var": var, "logp": logp, "loo": np.sum(logp)}


def as_tuple(v):
    return v["mu"], v["var"], v["logp"], v["loo"]


# What float64 itself misses of the long-double LOO values, in the normalisation of test_loo_gpu._hold_values: the worse of
# the mirror (loo_ref.closed: the explicit symmetrised inverse) and loo_values(name, float64) (the Cholesky factor, the
# device's own algorithm), measured on the CPU; tests/test_postfit_routes_cpu.py measures both again and holds this table
# within a factor 2.  The mirror alone: SMALL mu 2.5e-11 logp 1.6e-9, MID mu 9.3e-11 logp 7.0e-9.
LOO_FLOAT64_MISS = {
    "SMALL": dict(mu=3.6e-11, var=8.4e-12, logp=2.2e-9, total=1.5e-12),
    "MID": dict(mu=1.2e-10, var=7.8e-12, logp=7.0e-9, total=2.6e-12),
}


@functools.lru_cache(maxsize=None)
def loo_reference(name):
    """-> the reference of the LOO values and the bar of each of the four errors.

    SMALL and MID have cond K_y 1.1e6 and 2.6e6 and LOO log probabilities down to -6e3 (a smooth kernel, little noise),
    and float64 itself does not hold them to test_loo_gpu._hold_values: two float64 evaluations are 23 and 98 plain bars
    apart in the log probabilities, and at MID the Cholesky evaluation is 1.16 plain bars off the long-double means (the
    explicit inverse 0.93; the device 1.05 to 1.27 on the twelve routes).  So the rule of
    tests/test_sparse_grad_gpu.py::_reference: the reference is the long-double evaluation, and where float64 misses a
    plain bar against it (LOO_FLOAT64_MISS), the bar is 10 x that miss -- per quantity, in the normalisation of
    _hold_values, since the device's worst point need not be float64's on the CPU.  That makes the bars of the log
    probabilities 2.2e-8 (SMALL) and 7.0e-8 (MID) and of MID's means 1.2e-9; every other bar is the plain one.  BIG
    (cond 2e4) keeps the float64 mirror and the plain bars: N = 2950 in long double takes minutes, and its two float64
    evaluations agree to 0.03 of a bar."""
    f64 = mirror(name)[4]
    if name not in LOO_LONG_DOUBLE:
        return f64, dict(LOO_PLAIN)
    miss = LOO_FLOAT64_MISS[name]
    return loo_values(name, LD), {k: LOO_PLAIN[k] if miss[k] <= LOO_PLAIN[k] else 10.0 * miss[k] for k in LOO_PLAIN}


def ratios(out, ard, loo, y, loo_ref=None, loo_bars=LOO_PLAIN):
    """error / bar of every quantity a run holds, against ard_ref.lml_and_grad and loo_ref.closed (the LOO values:
    against loo_ref with loo_bars where given)"""
    ratio = {}
    if "lml" in out:
        ratio["lml"] = abs(out["lml"] - ard["lml"]) / abs(ard["lml"]) / TA.LML_RTOL
    if "alpha" in out:
        ratio["alpha"] = TP.relmax(out["alpha"], ard["alpha"]) / TP.ALPHA_RTOL
    if "lml_grad" in out:
        dl, ds = out["lml_grad"]
        ratio["lml_grad"] = max(abs(dl - ard["g_l"]) / ard["s_l"], abs(ds - ard["g_sigma"]) / ard["s_sigma"]) / TA.GRAD_RTOL
    if "lml_grad_ard" in out:
        d_r, d_l, d_s, d_n = out["lml_grad_ard"]
        ratio["lml_grad_ard"] = max(np.max(np.abs(d_r - ard["g_r"]) / ard["s_r"]), abs(d_l - ard["g_l"]) / ard["s_l"],
                                    abs(d_s - ard["g_sigma"]) / ard["s_sigma"], abs(d_n - ard["g_noise"]) / ard["s_noise"]) / TA.GRAD_RTOL
    if "loo" in out:
        err = loo_errors(out["loo"], loo if loo_ref is None else loo_ref, y)
        ratio["loo"] = max(err[k] / loo_bars[k] for k in err)
    if "loo_grad" in out:
        ratio["loo_grad"] = max(abs(g - loo["g_" + k]) / loo["s_" + k] for g, k in zip(out["loo_grad"], ("l", "sigma", "noise"))) / TL.GRAD_RTOL
    return ratio


def hold(out, name, tag):
    """prints error / bar of every quantity (the measured headroom), then asserts with the modules' own holders"""
    X, y, r, ard, loo = mirror(name)
    loo_ref, loo_bars = loo_reference(name)
    ratio = ratios(out, ard, loo, y, loo_ref, loo_bars)
    print("%s: error / bar  " % tag + "  ".join("%s %.2e" % kv for kv in ratio.items()) + "  worst %.2e" % max(ratio.values()))
    assert np.all(np.isfinite(flat(out))), tag
    if "lml" in out:
        assert abs(out["lml"] - ard["lml"]) <= TA.LML_RTOL * abs(ard["lml"]), tag
    if "alpha" in out:
        assert out["alpha"].shape == ard["alpha"].shape and TP.relmax(out["alpha"], ard["alpha"]) <= TP.ALPHA_RTOL, tag
    if "lml_grad" in out:
        dl, ds = out["lml_grad"]
        assert abs(dl - ard["g_l"]) <= TA.GRAD_RTOL * ard["s_l"] and abs(ds - ard["g_sigma"]) <= TA.GRAD_RTOL * ard["s_sigma"], tag
    if "lml_grad_ard" in out:
        TA._hold_gradient(out["lml_grad_ard"], ard, tag)
    if "loo" in out and name in LOO_LONG_DOUBLE:
        err = loo_errors(out["loo"], loo_ref, y)
        print("%s cond %.2e: mu %.2e var %.2e logp %.2e total %.2e" % (tag, loo["cond"], err["mu"], err["var"], err["logp"], err["total"]))
        for k in err:
            assert err[k] <= loo_bars[k], (tag, k, err[k], loo_bars[k])
    elif "loo" in out:
        TL._hold_values(out["loo"], loo, y, tag)
    if "loo_grad" in out:
        TL._hold_gradient(out["loo_grad"], loo, tag)


_default = {}


def default_run(ctx, name):
    if name not in _default:
        _default[name] = run(ctx, name)
    return _default[name]


# ------------------------------------------------------------------------------------------------------ every route
@pytest.mark.parametrize("name,route", CASES)
def test_route_matches_the_mirror_and_itself(pctx, name, route):
    with options(pctx, (BIG_ROUTES if name == "BIG" else ROUTES)[route]):
        a = run(pctx, name)
        b = run(pctx, name)
    hold(a, name, "%s %s" % (name, route))
    assert same_bits(a, b)
    if route == "default":
        _default.setdefault(name, a)
    elif route in SAME_BITS_AS_DEFAULT:
        assert same_bits(a, default_run(pctx, name))


# --------------------------------------------------------------------------------------------- the resident factor
def test_post_fit_calls_use_the_leaves_of_the_resident_factor(pctx):
    """factorize_impl records panel_fused with the factor (Resident::factor_fused) and the shims install it again
    (resident_tuning): a first-generation factor has no inverses in its diagonal tiles, so the tri sweep must keep the
    64-column leaves and the backward solve launch_trsv_lt, whatever the option says by then -- and the reverse.  Every
    result equals, bit for bit, the one taken under the option of the fit.  The regression counterpart of
    tests/test_classify_routes_gpu.py::test_predict_uses_the_leaves_of_the_resident_factor"""
    for fit_with in (0, 1):
        try:
            with options(pctx, {"panel_fused": fit_with}):
                lml = fit(pctx, "MID")
                want = post_fit(pctx)
                pctx.set_option("panel_fused", 1 - fit_with)
                got = post_fit(pctx)
        finally:
            pctx.set_lengthscales(None)
        assert same_bits(want, got), "fit with panel_fused %d, calls under %d" % (fit_with, 1 - fit_with)
        hold(dict(got, lml=lml), "MID", "MID fit with panel_fused %d, post-fit calls under %d" % (fit_with, 1 - fit_with))


def _prediction_mirror(name, Xs):
    """mean and variance at Xs as oracle/gp_oracle.py::fit_predict_feasible states them, v = L^-1 K_s from the Cholesky
    factor (what tests/test_parity_gpu.py holds predictions to at MU_ATOL and VAR_ATOL up to N = 4096; the explicit
    inverse of the gradient mirror is itself 1e-9 and 1e-10 off that at cond K_y 2.6e6, the whole of both bars)"""
    X, y, r, _, _ = mirror(name)
    K = R.kernel(np.vstack([Xs, X]), r, SIGMA, ELL)
    L = np.linalg.cholesky(K[len(Xs):, len(Xs):] + PROBLEMS[name][2] * np.eye(len(X)))
    v = solve_triangular(L, K[len(Xs):, :len(Xs)], lower=True)
    return v.T @ solve_triangular(L, y, lower=True), SIGMA ** 2 - np.sum(v * v, axis=0)


def test_options_moved_after_the_fit(pctx):
    """one fused factor of MID, every call under another backward solve and sweep: the block inverses of trsv_vinv = 1
    (have_vinv) are there when trsv_vinv = 2 asks for its side copy (have_vside) and when trsv_vinv = 0 wants none, and
    the last gradient sweeps with six blocks of 256 where the fit made three of 512.  The inverses sit above the
    diagonal of the factor's diagonal tiles: no reader of the factor may see them"""
    X = mirror("MID")[0]
    N = len(X)
    Xs = np.random.default_rng(15).uniform(0.0, 4.0, size=(37, X.shape[1]))
    mu_ref, var_ref = _prediction_mirror("MID", Xs)

    def state():
        return pctx.factor(N - 300, N, N - 300, N), pctx.predict(Xs, want_sd=False), pctx.m()

    out = {}
    try:
        out["lml"] = fit(pctx, "MID")
        before = state()
        with options(pctx, {"trsv_vinv": 1}):
            out["alpha"] = pctx.alpha()
        with options(pctx, {"trsv_vinv": 2}):
            out["lml_grad_ard"] = pctx.lml_grad_ard()
        with options(pctx, {"trsv_vinv": 0}):
            out["loo"] = pctx.loo()
        with options(pctx, {"trsv_vinv": 2, "nb": 256, "lookahead": 0}):
            out["loo_grad"] = pctx.loo_grad()
        mu, var = pctx.predict(Xs, want_sd=False)
        after = state()
    finally:
        pctx.set_lengthscales(None)
    hold(out, "MID", "MID, options moved after the fit")
    print("prediction: max|dmu| %.2e (bar %.0e)  max|dvar| %.2e (bar %.0e)" % (np.max(np.abs(mu - mu_ref)), TP.MU_ATOL,
                                                                              np.max(np.abs(var - var_ref)), TP.VAR_ATOL))
    assert np.max(np.abs(mu - mu_ref)) <= TP.MU_ATOL and np.max(np.abs(var - var_ref)) <= TP.VAR_ATOL
    assert np.array_equal(before[0], after[0]) and np.array_equal(np.triu(after[0], 1), np.zeros_like(after[0]))
    assert np.array_equal(before[1][0], after[1][0]) and np.array_equal(before[1][1], after[1][1])
    assert np.array_equal(before[1][0], mu) and np.array_equal(before[1][1], var)
    assert np.array_equal(before[2], after[2])


# ------------------------------------------------------------------------------------- other kernel families, once each
CO2_ROUTES = {"panel_fused0": ROUTES["panel_fused0"], "la256_deep": ROUTES["la256_deep"],
              "la256_deep_nb128": dict(ROUTES["la256_deep"], nb=128), "small_tiles0": ROUTES["small_tiles0"]}


@pytest.mark.parametrize("route", list(CO2_ROUTES))
def test_co2_gradient(pctx, route):
    """gpmi_lml_grad_co2 on the first 300 months of the fixture (Np = 384), against the long-double mirror of
    tests/test_co2_grad_gpu.py with that module's hold.  The front is the one of the calls above and the fused pass does
    not depend on the route, so there is no product with the routes.  384 columns are one block of 512, where
    lookahead_for answers no: la256_deep_nb128 is the route under which the sweep does run beside its panel chain"""
    g = golden("kernels_bo_co2")
    book = (g["co2_theta"], g["co2_X"], g["co2_y"])
    th, X, y = book
    ref = TC.fixture_mirror(book, 300)
    try:
        with options(pctx, CO2_ROUTES[route]):
            lml = TC.fit(pctx, X[:300], y[:300], th)
            got = pctx.lml_grad_co2()
            again = pctx.lml_grad_co2()
    finally:
        pctx.set_kernel("rbf")
    assert abs(lml - float(ref["lml"])) <= TC.LML_RTOL * abs(float(ref["lml"])), (lml, float(ref["lml"]))
    TC.hold(got, ref, "CO2 fixture N=300 %s" % route)
    assert np.array_equal(got[0], again[0]) and got[1] == again[1]


def test_matern52_gradient_on_a_first_generation_factor(pctx):
    """one Matern-5/2 gpmi_lml_grad_ard at SMALL's shape under panel_fused = 0, at the bar of tests/test_matern_gpu.py"""
    N, d, _ = PROBLEMS["SMALL"]
    X, y, r, ref, _ = TM._grad_case(2.5, N, d)
    try:
        with options(pctx, ROUTES["panel_fused0"]):
            pctx.set_kernel("matern52")
            pctx.set_train(X, y)
            pctx.set_lengthscales(r)
            lml = pctx.factorize(TM.SIGMA, TM.ELL, TM.NOISE)
            got = pctx.lml_grad_ard()
            again = pctx.lml_grad_ard()
    finally:
        pctx.set_lengthscales(None)
        pctx.set_kernel("rbf")
    assert abs(lml - ref["lml"]) <= TM.LML_RTOL * abs(ref["lml"])
    assert TM.GRAD_RTOL == TA.GRAD_RTOL
    TA._hold_gradient(got, ref, "Matern 5/2 N=%d d=%d panel_fused0" % (N, d))
    assert np.array_equal(got[0], again[0]) and got[1:] == again[1:]


# --------------------------------------------------------------------------------------------- classifier gradients
@functools.lru_cache(maxsize=None)
def classifier_mirror(name):
    """-> the mirror's flat gradient and log q, at tol = 1e-13: one evaluation per problem"""
    X, lab, Xs, C, z = CR.data(name)
    if C is None:
        ref = LG.log_q_and_gradient(X, lab, CR.SIGMA, CR.ELL, None, tol=FIT_TOL)
        flat_ref = LG.flat(ref)
    else:
        ref = SG.log_q_and_gradient(X, lab, C, CR.SIGMA, CR.ELL, None, tol=FIT_TOL)
        flat_ref = SG.flat(ref)
    assert ref["fit"]["converged"]
    return flat_ref, ref["log_q"]


def classifier_gradient(ctx, name):
    d_r, d_l, d_sigma = ctx.laplace_grad() if CR.data(name)[3] is None else ctx.softmax_grad()
    return np.concatenate([d_r, [d_l, d_sigma]])


def classifier_fit_and_compare(ctx, name, tag, ref, ref_log_q, bar):
    """compare of tests/test_laplace_grad_gpu.py; for the softmax model the statements of
    tests/test_softmax_grad_gpu.py::compare, which computes its mirror on every call, with the shared one"""
    X, lab, Xs, C, z = CR.data(name)
    if C is None:
        return TLG.compare(ctx, tag, X, lab, CR.SIGMA, CR.ELL, None, ref, ref_log_q, bar)
    log_q, _, iters, conv = ctx.softmax_fit(X, lab, C, CR.SIGMA, CR.ELL, tol=FIT_TOL, lengthscales=None)
    g = classifier_gradient(ctx, name)
    err = float(np.max(np.abs(g - ref)) / np.max(np.abs(ref)))
    print("%s: gpu - mirror %.3g (bar %.3g), %d Newton steps, log q %.3g apart"
          % (tag, err, bar, iters, abs(log_q - ref_log_q) / abs(ref_log_q)))
    assert conv
    assert np.all(np.isfinite(g))
    assert err <= bar


@pytest.mark.parametrize("route", list(ROUTES))
@pytest.mark.parametrize("name", ["binary641", "softmax641_C3"])
def test_classifier_gradient_on_every_route(pctx, name, route):
    """laplace_grad_impl runs factor_inverse_front on the factor of B without the backward solve, softmax_grad_impl
    backward_solve_rhs and neg_gram_lower_dense; a fit at tol = 1e-13, the gradient twice and after a fresh fit with the
    same bits, and the fit's prediction the same bits before and after the gradient"""
    ref, ref_log_q = classifier_mirror(name)
    bar = gpu_bar(CLASSIFIER_ROUNDING[name])
    pctx.set_lengthscales(None)
    with options(pctx, ROUTES[route]):
        classifier_fit_and_compare(pctx, name, "%s %s" % (name, route), ref, ref_log_q, bar)
        before = CR.gpu_predict(pctx, name)
        g1 = classifier_gradient(pctx, name)
        after = CR.gpu_predict(pctx, name)
        g2 = classifier_gradient(pctx, name)
        classifier_fit_and_compare(pctx, name, "%s %s, second fit" % (name, route), ref, ref_log_q, bar)
        g3 = classifier_gradient(pctx, name)
    assert np.array_equal(g1, g2) and np.array_equal(g1, g3)
    for u, v in zip(before, after):
        assert np.array_equal(u, v)
