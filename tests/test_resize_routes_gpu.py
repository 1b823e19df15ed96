"""gpmi_append and gpmi_remove on every factor and GEMM route, at borders of several blocks.  An append is built from the
pieces of a fit, called with arguments no other caller uses (csrc/append.hip): solve_sweep_factor with its block size and
lookahead decided from N0 while V is a set of rows of A itself and m = border decides the sharing state at 2048 rows; one
gemm_minus_lower of (border + 128) x border x N0 with the y block as its last row tile; cholesky_inplace on the sub-block
at (N0, N0), its block size and lookahead decided from border, its pivots reported as N0 + info + 1.  A removal has
kernels of its own that no option reaches, but on a fused factor remove_tile_inverse_kernel writes the 16 x 16 inverses
every later trsm128 (one- and two-launch form), launch_vinv128 (trsv_vinv 1 and 2) and skinny border sweep reads.
tests/test_append_gpu.py and tests/test_remove_gpu.py drive all of this with a border of at most two blocks under the
default options alone.

Problems: ard_ref.problem(., 8, seed) through tests/test_append_gpu.py::_problem and tests/test_remove_gpu.py::_problem,
sigma 1.2, l 1.5, noise 1e-2, so the bars of those two modules carry over.  tests/test_resize_routes_cpu.py writes out the
GEMM launches of every (problem, route), asks gemm_route for the kernel of each and holds what is said here:

    WIDE      N 700 + 900    N0 640, Np1 1664, border 1024: the sweep over a factor of 512 + 128 columns, the border two
                             blocks of 512 plus the y block; every launch below 128 tiles.  The twelve ROUTES of
                             tests/test_classify_routes_gpu.py
    WIDER     N 700 + 2000   Np1 2816, border 2176 >= 2048: under la256_* the sweep runs beside_update (the two-launch
                             trsm128, gemm_nt_small_kernel<3>) and both the sweep and the border's Cholesky run with
                             lookahead; the rank-N0 update, 18 x 17 tiles lower with K = 640, on
                             gemm_nt_dma_kernel<2, false> and under `tall` on gemm_nt_dma_tall_kernel<false>.  Without
                             lookahead the border's first trailing update (14 x 13 tiles, role 1) reaches the family too,
                             under the Cholesky's own symbols; under nb128 six of them do
    TICKET    N 700 + 2373   border 2560 (N1 = 3073: one real row in the last tile): the smallest border whose rank-N0
                             update (21 x 20 tiles) is one round of 256 blocks, gemm_nt_dma_ticket_kernel under
                             gemm_ticket = 2.  Counted by hand as live tiles the border would be 2816; the plan counts
                             supertiles, and gemm_route answers 2560
    PERSIST   N 700 + 3397   border 3584 (N1 = 4097): the smallest whose update (29 x 28 tiles) is two rounds,
                             gemm_nt_dma_persist_kernel under the default gemm_persist = 1, gemm_nt_dma_kernel<2, false>
                             under gemm_persist = 0 (by hand: 3968)
    SKINNY    N 1500 + 16    append_skinny = 1: the <= 16-row border sweep does not depend on the route, the border's
                             Cholesky (one block) and the backward solve behind it do
    IN PLACE  WIDE with reserve = 1000, and with reserve = 0 behind a one-pass fit_predict_sample_resident with 900 test
                             points, whose columns and rows take the border: ld and rows stay, the y row moves up
    REMOVED   N 1100 - 16    EDGES of tests/test_remove_gpu.py, one sweep from J0 = 0
              N 1100 - 200   every third index below 600, 13 sweeps
              N 1100 - 3     300, 301 and 700: J0 = 256, and the 16 x 16 tiles at 256 and 272 lie between J0 and the first
                             removed index -- rewritten by the sweep like everything from J0 on, so their inverses are
                             among those remove_tile_inverse_kernel has to write (the other two lists start in tile 0)
                             on the twelve ROUTES, the route set before the fit and kept: alpha, predict at 40 and at 2100
                             points (a sweep with m >= 2048: the two-launch trsm128 under la256_*), lml_grad_ard, loo, a
                             padded append of 300 points and a skinny append of 5; once with panel_fused flipped between
                             fit and removal, in both directions

What a case asserts (hold() prints error / bar of every quantity, one line, before it asserts; no bar is new):
  * against the kernel matrix (the context's own K build): |K_y - L L^T| <= 2 n u |L| |L^T| componentwise, in long double,
    panel_ref.potrf_ratio up to 700 points and beyond on sampled rows of the border (from J0 on for a removal) -- 64 rows,
    fewer where 64 rows of n^2 long-double flops each would take a case beyond a few seconds (52 at 3073 points, 29 at
    4097); the same for a fresh fit of the same points on the same route;
  * against that fresh fit, in a second context: the LML, m, diag(L), alpha, predictions, lml_grad_ard and loo at the bars
    of tests/test_append_gpu.py (LML_RTOL, M_RTOL, DIAG_RTOL, ALPHA_RTOL, MU_ATOL, SD_ATOL, GRAD_RTOL x the cancellation
    scales of the dense mirror, the four LOO bars);
  * against a float64 CPU Cholesky of the final K_y (scipy.linalg.cholesky and two triangular solves): the LML and alpha,
    at LML_RTOL and ALPHA_RTOL, so that two GPU results agreeing is never the only evidence;
  * bit for bit: the leading N0 x N0 (J0 x J0) block is the resident one, the same call twice gives the same bits, and
    each route of SAME_BITS_AS_DEFAULT gives the factor, m and LML of `default` (la_min: "same
    bits").  No other equality between routes is asserted;
  * layout(): N, Np, whether ld and rows moved (never for IN PLACE and the removals), route 1 / 0.

Then a failing pivot in the second block of a border of WIDE's shape (test_failed_pivot_in_the_second_block).

The bookkeeping of this module runs on the CPU first, through a NumPy stand-in for the context
(tests/test_resize_routes_cpu.py).  No (problem, route) pair is skipped, and none is expected to fail."""
import functools

import numpy as np
import pytest
from scipy.linalg import cholesky, solve_triangular

import panel_ref as R
import test_append_gpu as TA
import test_classify_routes_gpu as CR
import test_postfit_routes_gpu as PR
import test_remove_gpu as TR

pytestmark = pytest.mark.gpu

SIGMA, ELL, NOISE, D = TA.SIGMA, TA.ELL, TA.NOISE, 8
assert (SIGMA, ELL, NOISE) == (1.2, 1.5, 1e-2) == (TR.SIGMA, TR.ELL, TR.NOISE)
LML_RTOL, M_RTOL, ALPHA_RTOL, DIAG_RTOL = TA.LML_RTOL, TA.M_RTOL, TA.ALPHA_RTOL, TA.DIAG_RTOL
MU_ATOL, SD_ATOL, GRAD_RTOL = TA.MU_ATOL, TA.SD_ATOL, TA.GRAD_RTOL
assert (LML_RTOL, M_RTOL, ALPHA_RTOL, DIAG_RTOL, MU_ATOL, SD_ATOL, GRAD_RTOL) == (
    TR.LML_RTOL, TR.M_RTOL, TR.ALPHA_RTOL, TR.DIAG_RTOL, TR.MU_ATOL, TR.SD_ATOL, TR.GRAD_RTOL)
LOO_BARS = dict(mu=1e-10, var=1e-10, logp=1e-10, total=LML_RTOL)      # _hold_against_fresh of both modules
FACTOR_BAR = 2.0

ROUTES = CR.ROUTES
SAME_BITS_AS_DEFAULT = CR.SAME_BITS_AS_DEFAULT
DEFAULTS = dict(PR.DEFAULTS, append_skinny=-1, reserve=0)
assert set(CR.DEFAULTS) <= set(DEFAULTS) and all(set(o) <= set(DEFAULTS) for o in list(ROUTES.values()) + list(PR.BIG_ROUTES.values()))

# name: (N, k, option append_skinny)
APPENDS = {"WIDE": (700, 900, -1), "WIDER": (700, 2000, -1), "TICKET": (700, 2373, -1), "PERSIST": (700, 3397, -1),
           "SKINNY": (1500, 16, 1)}
APPEND_ROUTES = {
    "WIDE": dict(ROUTES),
    "WIDER": dict({r: ROUTES[r] for r in ("default", "nb128", "la256_deep", "la256_shallow", "panel_fused0")},
                  tall=PR.BIG_ROUTES["tall"], persist0={"gemm_persist": PR.BIG_ROUTES["persist0_nb3072"]["gemm_persist"]}),
    "TICKET": {"ticket2": {"gemm_ticket": PR.BIG_ROUTES["ticket2_nb2048"]["gemm_ticket"]}},
    "PERSIST": {"default": {}, "persist0": {"gemm_persist": 0}},
    "SKINNY": {r: ROUTES[r] for r in ("nb128", "nb256", "la256_deep", "trsv_vinv0", "trsv_vinv1", "trsv_vinv2")},
}
APPEND_CASES = [(name, route) for name in APPENDS for route in APPEND_ROUTES[name]]
# IN PLACE: WIDE once more; reserve, test points of a one-pass fit in front
IN_PLACE = {"reserve1000": (1000, 0), "one_pass900": (0, 900)}
IN_PLACE_ROUTES = ("default", "la256_deep")

REMOVE_N, REMOVE_APPEND, REMOVE_SKINNY = 1100, 300, 5
REMOVALS = {"EDGES": list(TR.EDGES), "THIRDS": list(range(0, 600, 3)), "MIDDLE": [300, 301, 700]}
assert len(REMOVALS["EDGES"]) == 16 and len(REMOVALS["THIRDS"]) == 200
REMOVE_CASES = [(which, route) for which in REMOVALS for route in ROUTES]
N_WIDE_PREDICT = 2100

PIVOT_ROUTES = ("default", "la256_deep", "panel_fused0")
PIVOT_COLUMN = 600           # of the border: in its second block of 512


@pytest.fixture(scope="module")
def actx():
    """the context that appends and removes; options are context state, so it is this module's own"""
    from gaussian_process_amd import GPContext
    c = GPContext(0)
    yield c
    c.close()


@pytest.fixture(scope="module")
def fctx():
    """the context of the fresh fits, on the same route"""
    from gaussian_process_amd import GPContext
    c = GPContext(0)
    yield c
    c.close()


class options:
    """a route's options on both contexts, and every option back to its default afterwards"""

    def __init__(self, ctxs, opts):
        self.ctxs, self.opts = ctxs, opts

    def __enter__(self):
        for c in self.ctxs:
            for k, v in self.opts.items():
                c.set_option(k, v)

    def __exit__(self, *exc):
        for c in self.ctxs:
            for k in self.opts:
                c.set_option(k, DEFAULTS[k])
            for k in ("append_skinny", "reserve"):
                c.set_option(k, DEFAULTS[k])


def relmax(a, b):
    return float(np.max(np.abs(a - b)) / np.max(np.abs(b)))


# ------------------------------------------------------------------------------------------------------------- the data
def append_data(name):
    """-> X, y (N + k points), 40 test points: the data of tests/test_append_gpu.py for that many points"""
    N, k, _ = APPENDS[name]
    return TA._problem(N + k, D)


def remove_data():
    """-> X, y (1100 + 300 + 5 points), 40 test points: the data of tests/test_remove_gpu.py"""
    return TR._problem(REMOVE_N + REMOVE_APPEND + REMOVE_SKINNY, D)


@functools.lru_cache(maxsize=None)
def wide_test_points(n):
    Xs = np.random.default_rng(n).uniform(0.0, 4.0, size=(n, D))
    Xs.setflags(write=False)
    return Xs


def remove_order(which, stage):
    """the points resident after stage 0 (the removal), 1 (+ 300) and 2 (+ 5), in the context's order"""
    keep = TR._survivors(REMOVE_N, REMOVALS[which])
    return np.concatenate([keep, np.arange(REMOVE_N, REMOVE_N + (0, REMOVE_APPEND, REMOVE_APPEND + REMOVE_SKINNY)[stage])])


# ---------------------------------------------------------------------------------------- references, once per data set
def sample_rows(n, first, cap=64, budget=5e8):
    """the rows whose long-double residual is taken beyond 700 points: the first and the last row from `first` on and a
    seeded sample, `cap` rows at the most and fewer where rows x n^2 flops would pass `budget` (the product runs without
    BLAS; 2.5e8 took PERSIST 2.4 s on the machine of the MI355X, all of it included)"""
    rows = np.arange(min(first, n - 1), n)
    cap = max(8, min(cap, int(budget / float(n) ** 2)))
    if rows.size > cap:
        rng = np.random.default_rng(n)
        keep = {int(rows[0]), int(rows[-1])}
        keep |= set(int(v) for v in rng.choice(rows, cap - len(keep), replace=False))
        rows = np.array(sorted(keep))
    return rows


def ratio_rows(S, G, rows):
    """test_remove_gpu._ratio_rows (panel_ref.potrf_ratio on the given rows), converting to long double only the slices
    a row block needs: the whole factor of 4097 points in long double is 270 MB"""
    n = S.shape[0]
    rows = np.asarray(rows)
    worst = 0.0
    for c0 in range(0, int(rows.max()) + 1, 128):
        c1 = min(n, c0 + 128)
        sel = rows[rows >= c0]
        Lr = np.where(np.arange(c1)[None, :] <= sel[:, None], G[sel, :c1], 0.0)        # the lower triangle's part of each
        Lc = np.tril(G[c0:c1, :c1], c0)
        Rr = np.abs(S[sel, c0:c1].astype(R.LD) - Lr.astype(R.LD) @ Lc.astype(R.LD).T)
        Dn = (np.abs(Lr) @ np.abs(Lc).T).astype(R.LD) * (n * R.U)
        low = sel[:, None] >= np.arange(c0, c1)[None, :]
        worst = max(worst, R._ratio(Rr[low], Dn[low]))
    return worst


def factor_ratio(S, G, first):
    """worst |K_y - L L^T| / (n u |L| |L^T|): the whole factor up to 700 points, sampled rows from `first` on beyond"""
    n = S.shape[0]
    if n <= 700:
        return R.potrf_ratio(S, G)
    return ratio_rows(S, G, sample_rows(n, first))


_reference = {}


def reference(key, ctx, X, y):
    """-> K_y from the context's own K build (its routes are held by tests/test_kbuild_routes_gpu.py), the float64 CPU
    Cholesky of it (LML, alpha) and the cancellation scales of the gradients from the dense mirror (those once per data
    set and session: test_remove_gpu._scales)"""
    if key not in _reference:
        S = ctx.rbf(X, X, SIGMA, ELL)
        S[np.diag_indices_from(S)] += NOISE
        L = cholesky(S, lower=True, check_finite=False)
        m = solve_triangular(L, y, lower=True, check_finite=False)
        alpha = solve_triangular(L, m, lower=True, trans="T", check_finite=False)
        lml = -.5 * (m @ m) - np.sum(np.log(np.diag(L))) - .5 * len(y) * np.log(2 * np.pi)
        del L
        S.setflags(write=False)
        while len(_reference) >= 3:                 # the three stages of a removal case; 134 MB each at 4097 points
            del _reference[next(iter(_reference))]
        _reference[key] = dict(S=S, lml=float(lml), alpha=alpha)
    return _reference[key]


def scales(key, X, y):
    return TR._scales(("resize",) + key, X, y, D, "rbf", False)


def results(ctx, lml, S, first, Xs, full):
    """everything a case compares, read from a context that holds the fit; full: the calls behind the gradient front"""
    out = dict(lml=lml, ratio=factor_ratio(S, ctx.factor(), first), m=ctx.m(), diag=ctx.diag(), alpha=ctx.alpha())
    out["mu"], out["sd"] = ctx.predict(Xs)
    if full:
        out["grad"] = ctx.lml_grad_ard()
        out["loo"] = ctx.loo()
    return out


_fresh = {}


def fresh(fctx, key, route, X, y, first, Xs, full):
    """the fresh fit of the same points on the same route (fctx carries the route's options): once per (data set, route).
    fctx holds that fit afterwards only when it was computed by this call, so everything compared is in the result."""
    if (key, route, full) not in _fresh:
        ref = reference(key, fctx, X, y)
        lml = fctx.fit(X, y, SIGMA, ELL, NOISE, lengthscales=None)
        _fresh[key, route, full] = results(fctx, lml, ref["S"], first, Xs, full)
    return _fresh[key, route, full]


def errors(got, want, ref, y):
    """error / bar of every quantity: got against the fresh fit `want`, both factors against K_y, got against float64"""
    e = dict(factor=got["ratio"] / FACTOR_BAR, fresh_factor=want["ratio"] / FACTOR_BAR,
             lml=abs(got["lml"] - want["lml"]) / abs(want["lml"]) / LML_RTOL,
             m=relmax(got["m"], want["m"]) / M_RTOL, diag=relmax(got["diag"], want["diag"]) / DIAG_RTOL,
             alpha=relmax(got["alpha"], want["alpha"]) / ALPHA_RTOL,
             mu=float(np.max(np.abs(got["mu"] - want["mu"]))) / MU_ATOL, sd=float(np.max(np.abs(got["sd"] - want["sd"]))) / SD_ATOL)
    if "grad" in got:
        ga, gf, s = got["grad"], want["grad"], ref["scales"]()
        e["grad"] = float(max(np.max(np.abs(ga[0] - gf[0]) / s["s_r"]),
                              *(abs(ga[i] - gf[i]) / s[n] for i, n in ((1, "s_l"), (2, "s_sigma"), (3, "s_noise"))))) / GRAD_RTOL
    if "loo" in got:
        la, lf = got["loo"], want["loo"]
        e["loo"] = float(max(np.max(np.abs(la[0] - lf[0])) / max(1.0, np.max(np.abs(y))) / LOO_BARS["mu"],
                             np.max(np.abs(la[1] - lf[1]) / lf[1]) / LOO_BARS["var"],
                             np.max(np.abs(la[2] - lf[2]) / np.maximum(1.0, np.abs(lf[2]))) / LOO_BARS["logp"],
                             abs(la[3] - lf[3]) / np.sum(np.abs(lf[2])) / LOO_BARS["total"]))
    for side, out in (("f64_lml", got), ("fresh_f64_lml", want)):
        e[side] = abs(out["lml"] - ref["lml"]) / abs(ref["lml"]) / LML_RTOL
    for side, out in (("f64_alpha", got), ("fresh_f64_alpha", want)):
        e[side] = relmax(out["alpha"], ref["alpha"]) / ALPHA_RTOL
    return e


WORST = {}            # quantity -> (worst error / bar, tag), for the report


def hold(got, want, ref, y, tag):
    """prints error / bar of every quantity on one line, then asserts each at 1"""
    e = errors(got, want, ref, y)
    print("%s: error / bar  " % tag + "  ".join("%s %.2e" % kv for kv in e.items()) + "  worst %.2e" % max(e.values()))
    for k, v in e.items():
        if v > WORST.get(k, (-1.0, ""))[0]:
            WORST[k] = (v, tag)
    for k in ("m", "diag", "alpha", "mu", "sd"):
        assert got[k].shape == want[k].shape and np.all(np.isfinite(got[k])), (tag, k)
    assert np.isfinite(got["lml"]), tag
    for k, v in e.items():
        assert v <= 1.0, (tag, k, v)


def bits(run):
    return run["lml"], run["G"], run["m"]


def same_bits(a, b):
    return a["lml"] == b["lml"] and np.array_equal(a["G"], b["G"]) and np.array_equal(a["m"], b["m"])


# -------------------------------------------------------------------------------------------------------------- appends
def run_append(ctx, name, reserve=0, n_test=0):
    """the fit of N points and the append of k under the options the context carries -> the LML, the factor, m, both
    layouts and whether the leading N0 x N0 block kept its bits.  n_test > 0: the one-pass fit with its posterior-sample
    factor in front, whose test columns and rows the border then takes"""
    N, k, skinny = APPENDS[name]
    X, y, _ = append_data(name)
    ctx.set_option("append_skinny", skinny)
    ctx.set_option("reserve", reserve)
    if n_test:
        ctx.set_lengthscales(None)
        ctx.set_train(X[:N], y[:N])
        ctx.set_test(wide_test_points(n_test))
        ctx.fit_predict_sample_resident(SIGMA, ELL, NOISE, 1e-6, want_factor=False)
    else:
        ctx.fit(X[:N], y[:N], SIGMA, ELL, NOISE, lengthscales=None)
    N0 = N // 128 * 128
    before = ctx.layout()
    lead = ctx.factor(0, N0, 0, N0)
    lml = ctx.append(X[N:], y[N:])
    return dict(lml=lml, G=ctx.factor(), m=ctx.m(), before=before, after=ctx.layout(),
                lead_kept=np.array_equal(ctx.factor(0, N0, 0, N0), lead))


def check_append_layout(run, name, fused, in_place):
    N, k, skinny = APPENDS[name]
    before, after = run["before"], run["after"]
    assert before["N"] == N and after["N"] == N + k and after["Np"] == (N + k + 127) // 128 * 128, (before, after)
    assert after["route"] == (1 if k <= 16 and fused and N >= 128 and skinny != 0 else 0), after
    assert ((after["ld"], after["rows"]) == (before["ld"], before["rows"])) == in_place, (before, after)
    assert run["lead_kept"], "the leading N0 x N0 block is the resident one"


_default_append = {}


def append_case(actx, fctx, name, route, opts, tag, reserve=0, n_test=0, in_place=False):
    N, k, _ = APPENDS[name]
    X, y, Xs = append_data(name)
    with options((actx, fctx), opts):
        a = run_append(actx, name, reserve, n_test)
        b = run_append(actx, name, reserve, n_test)
        check_append_layout(a, name, opts.get("panel_fused", 1), in_place)
        assert same_bits(a, b), "the same append twice"
        want = fresh(fctx, (name,), route, X, y, N // 128 * 128, Xs, True)
        ref = dict(reference((name,), fctx, X, y), scales=lambda: scales((name,), X, y))
        got = results(actx, a["lml"], ref["S"], N // 128 * 128, Xs, True)
    hold(got, want, ref, y, tag)
    return a


@pytest.mark.parametrize("name,route", APPEND_CASES)
def test_append_on_every_route(actx, fctx, name, route):
    # SKINNY stays inside the padding of the last tile (Np = Np1 = 1536); every other append reallocates
    a = append_case(actx, fctx, name, route, APPEND_ROUTES[name][route], "%s %s" % (name, route), in_place=name == "SKINNY")
    if route == "default" and set(APPEND_ROUTES[name]) & set(SAME_BITS_AS_DEFAULT):
        _default_append[name] = bits(a)
    elif route in SAME_BITS_AS_DEFAULT:
        if name not in _default_append:
            with options((actx,), {}):
                _default_append[name] = bits(run_append(actx, name))
        lml, G, m = _default_append[name]
        assert a["lml"] == lml and np.array_equal(a["G"], G) and np.array_equal(a["m"], m), "the bits of the default route"


@pytest.mark.parametrize("route", IN_PLACE_ROUTES)
@pytest.mark.parametrize("how", list(IN_PLACE))
def test_append_in_place(actx, fctx, how, route):
    """the resident allocation takes the border of WIDE: sized by `reserve`, or left by a one-pass fit with 900 test points
    (columns [768, 1792) and rows [768, 1920) of A then hold K_ss, v^T and the y row behind them).  ld and rows stay, the
    y row moves to row 1664, and the result is the one of the reallocating append, bit for bit"""
    reserve, n_test = IN_PLACE[how]
    a = append_case(actx, fctx, "WIDE", route, ROUTES[route], "WIDE in place (%s) %s" % (how, route), reserve, n_test, in_place=True)
    with options((actx,), ROUTES[route]):
        moved = run_append(actx, "WIDE")
    assert (moved["after"]["ld"], moved["after"]["rows"]) != (a["after"]["ld"], a["after"]["rows"])
    assert same_bits(a, moved), "in place and reallocated: the same arithmetic"


# ------------------------------------------------------------------------------------------------------------- removals
def run_remove(ctx, which, flip=None):
    """the fit of 1100 points and the removal -> as run_append.  flip: the value of panel_fused for the removal and
    everything behind it; the fit runs under the other one"""
    X, y, _ = remove_data()
    idx = REMOVALS[which]
    J0 = min(idx) // 128 * 128
    if flip is not None:
        ctx.set_option("panel_fused", 1 - flip)
    ctx.fit(X[:REMOVE_N], y[:REMOVE_N], SIGMA, ELL, NOISE, lengthscales=None)
    if flip is not None:
        ctx.set_option("panel_fused", flip)
    before = ctx.layout()
    lead = ctx.factor(0, J0, 0, J0)
    lml = ctx.remove(idx)
    return dict(lml=lml, G=ctx.factor(), m=ctx.m(), before=before, after=ctx.layout(),
                lead_kept=np.array_equal(ctx.factor(0, J0, 0, J0), lead))


def check_remove_layout(run, which):
    n = REMOVE_N - len(REMOVALS[which])
    before, after = run["before"], run["after"]
    assert before["N"] == REMOVE_N and after["N"] == n and after["Np"] == (n + 127) // 128 * 128, (before, after)
    assert (after["ld"], after["rows"]) == (before["ld"], before["rows"]), "a removal keeps the allocation's shape"
    assert run["lead_kept"], "the leading J0 x J0 block is the resident one"


def after_the_removal(actx, fctx, which, route, fused, lml, tag):
    """the calls that read what the removal left -- alpha, predict at 40 and at 2100 points, lml_grad_ard, loo -- then a
    padded append of 300 points and a skinny one of 5, each against a fresh fit of the same points on fctx's route"""
    X, y, Xs = remove_data()
    J0 = min(REMOVALS[which]) // 128 * 128
    wide = wide_test_points(N_WIDE_PREDICT)
    for stage, k, skinny in ((0, 0, -1), (1, REMOVE_APPEND, 0), (2, REMOVE_SKINNY, 1)):
        order = remove_order(which, stage)
        key = (which, stage)
        if stage:
            n = len(order) - k
            first = n // 128 * 128
            actx.set_option("append_skinny", skinny)
            before = actx.layout()
            lml = actx.append(X[order[n:]], y[order[n:]])
            after = actx.layout()
            assert after["N"] == len(order) and after["route"] == (1 if skinny == 1 and fused else 0), after
            assert (stage == 1) or (after["ld"], after["rows"]) == (before["ld"], before["rows"]), "5 points fit the padding"
        else:
            first = J0
        want = fresh(fctx, key, route, X[order], y[order], first, Xs, stage == 0)
        ref = dict(reference(key, fctx, X[order], y[order]), scales=lambda: scales(key, X[order], y[order]))
        got = results(actx, lml, ref["S"], first, Xs, stage == 0)
        hold(got, want, ref, y[order], "%s, %s" % (tag, ("removed", "+ 300 padded", "+ 5 skinny")[stage]))
        if stage == 0:
            # a sweep with m >= 2048 rows: Sharing::beside_update under la256_*, the two-launch trsm128 on the new inverses
            mu_a, sd_a = actx.predict(wide)
            if (key, route, "wide") not in _fresh:
                fctx.fit(X[order], y[order], SIGMA, ELL, NOISE, lengthscales=None)
                _fresh[key, route, "wide"] = fctx.predict(wide)
            mu_f, sd_f = _fresh[key, route, "wide"]
            e_mu, e_sd = float(np.max(np.abs(mu_a - mu_f))), float(np.max(np.abs(sd_a - sd_f)))
            print("%s, predict at %d points: error / bar  mu %.2e  sd %.2e" % (tag, N_WIDE_PREDICT, e_mu / MU_ATOL, e_sd / SD_ATOL))
            assert np.all(np.isfinite(mu_a)) and np.all(np.isfinite(sd_a)) and e_mu <= MU_ATOL and e_sd <= SD_ATOL, tag


_default_remove = {}


def remove_case(actx, fctx, which, route, opts, tag, flip=None):
    with options((actx, fctx), opts):
        a = run_remove(actx, which, flip)
        b = run_remove(actx, which, flip)
        check_remove_layout(a, which)
        assert same_bits(a, b), "the same removal twice"
        # fctx keeps the options of the fit: the fresh fits are on the route of the resident factor
        after_the_removal(actx, fctx, which, route, opts.get("panel_fused", 1), b["lml"], tag)
    return a


@pytest.mark.parametrize("which,route", REMOVE_CASES)
def test_remove_on_every_route(actx, fctx, which, route):
    a = remove_case(actx, fctx, which, route, ROUTES[route], "%s %s" % (which, route))
    if route == "default":
        _default_remove[which] = bits(a)
    elif route in SAME_BITS_AS_DEFAULT:
        if which not in _default_remove:
            with options((actx,), {}):
                _default_remove[which] = bits(run_remove(actx, which))
        lml, G, m = _default_remove[which]
        assert a["lml"] == lml and np.array_equal(a["G"], G) and np.array_equal(a["m"], m), "the bits of the default route"


@pytest.mark.parametrize("fit_with", [0, 1])
def test_removal_follows_the_resident_factor(actx, fctx, fit_with):
    """panel_fused flipped between the fit and the removal: remove_impl reads Resident::factor_fused, as the
    *_predict_impl functions do -- a first-generation factor gets no stored inverses and keeps its 64-column leaves
    whatever the option says by then, a fused one gets them and keeps the 128-column ones.  The removal and everything
    behind it equal, bit for bit, what the option of the fit gives"""
    route = "default" if fit_with else "panel_fused0"
    tag = "THIRDS fit with panel_fused %d, removal under %d" % (fit_with, 1 - fit_with)
    flipped = remove_case(actx, fctx, "THIRDS", route, {"panel_fused": fit_with}, tag, flip=1 - fit_with)
    with options((actx,), {"panel_fused": fit_with}):
        kept = run_remove(actx, "THIRDS")
        alpha, mu = actx.alpha(), actx.predict(wide_test_points(N_WIDE_PREDICT))[0]
        run_remove(actx, "THIRDS", flip=1 - fit_with)
        assert np.array_equal(actx.alpha(), alpha), "the backward solve follows the resident factor"
        assert np.array_equal(actx.predict(wide_test_points(N_WIDE_PREDICT))[0], mu), "and so does the sweep"
    assert same_bits(flipped, kept)


# ------------------------------------------------------------------------------------- a failing pivot, second block
def pivot_problem():
    """well-separated grid points, sigma = 1, l = 1 and noise_var = -0.5, as in
    tests/test_append_gpu.py::test_failed_pivot_of_the_border: K is the identity to rounding and K - I / 2 positive
    definite, so the fit of 700 succeeds.  Of the 900 appended points the one at column 600 of the border sits on top
    of an old point: its pivot is 1 - .5 - (1 / sqrt(.5))^2 = -1.5, every pivot in front of it is .5"""
    N, k = APPENDS["WIDE"][:2]
    g = np.arange(N + k)
    X = np.stack([(g % 40) * 10.0, (g // 40) * 10.0], axis=1)
    y = np.sin(g * 0.37)
    N0 = N // 128 * 128
    X[N0 + PIVOT_COLUMN] = X[57]
    return N, N0, X, y


@pytest.mark.parametrize("route", PIVOT_ROUTES)
def test_failed_pivot_in_the_second_block(actx, fctx, route):
    """the border's Cholesky meets its first negative pivot in its second block of 512 (under la256_deep the panel that
    finds it runs on the second stream; under panel_fused0 it is potf2_64 that reports): LinAlgError names pivot
    N0 + column + 1, the one a fresh fit of the same data reports; the fit is dropped, the extended training set is
    resident, and a fit of it with positive noise matches a fresh one.  A numerical refusal: nothing faults"""
    N, N0, X, y = pivot_problem()
    assert 512 < PIVOT_COLUMN < 1024 and N0 + PIVOT_COLUMN >= N
    with options((actx, fctx), ROUTES[route]):
        actx.fit(X[:N], y[:N], 1.0, 1.0, -0.5, lengthscales=None)
        with pytest.raises(np.linalg.LinAlgError) as err:
            actx.append(X[N:], y[N:])
        with pytest.raises(np.linalg.LinAlgError) as err_fresh:
            fctx.fit(X, y, 1.0, 1.0, -0.5, lengthscales=None)
        print("failed pivot %s: append reports %d, a fresh fit %d, N0 + column + 1 = %d"
              % (route, err.value.bad_pivot, err_fresh.value.bad_pivot, N0 + PIVOT_COLUMN + 1))
        assert err.value.bad_pivot == N0 + PIVOT_COLUMN + 1 == err_fresh.value.bad_pivot
        assert actx.N == len(X) and actx.layout()["N"] == len(X)
        with pytest.raises(ValueError, match="no factorisation resident"):
            actx.m()
        with pytest.raises(ValueError, match="no factorisation resident"):
            actx.append(X[:1] + 5.0, y[:1])
        lml_a = actx.factorize(1.0, 1.0, 1e-2)
        lml_f = fctx.fit(X, y, 1.0, 1.0, 1e-2, lengthscales=None)
        e = (abs(lml_a - lml_f) / abs(lml_f) / LML_RTOL, relmax(actx.m(), fctx.m()) / M_RTOL,
             relmax(actx.alpha(), fctx.alpha()) / ALPHA_RTOL)
        print("failed pivot %s, the fit with noise 1e-2 behind it: error / bar  lml %.2e  m %.2e  alpha %.2e" % ((route,) + e))
        assert max(e) <= 1.0


def test_worst_figures():
    """the worst error / bar of each quantity over the cases that ran before this one (LAB_NOTES.md has a table of them)"""
    for k, (v, tag) in WORST.items():
        print("worst %-16s %.2e  (%s)" % (k, v, tag))
        assert v <= 1.0
