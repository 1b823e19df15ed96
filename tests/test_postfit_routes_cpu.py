"""What tests/test_postfit_routes_gpu.py rests on, without a GPU:

* the GEMM launches of its three problems behind the fit, written out from csrc/driver.hip and csrc/regress.hip
  (postfit_launches): inverse_transposed's tri sweep (solve_sweep_factor: the updates inside trsm_block and the sweep's
  own, M = min(m, k + nb) rows, split in two under lookahead), neg_gram_lower's row blocks (M = nb, N = r0 + nb,
  K = n - r0, lower, diag_off = r0) and the row-block product of gpmi_loo_grad (M = nb, N = K = Np);
* the kernel gemm_route (csrc/gpmi_route.h, through tests/sanitize/gemm_route_check.cpp) answers for every one of them
  under every route, held against the names recorded below (RECORD, BIG_LARGE);
* SMALL and MID: every launch has fewer than 128 tiles, and no value of gemm_tall, gemm_persist and gemm_ticket changes a
  kernel under any route -- those options have no route there;
* BIG: each of the three launch sites reaches the 128-tile LDS-DMA family under at least one route, and each of tall,
  ticket2 and persist changes at least one kernel against the route without it.  Blocks of 512 and 1024 leave every launch
  below the 256 blocks gemm_ticket = 2 asks for and the 512 gemm_persist asks for, so those two routes come with
  nb = 2048 and nb = 3072;
* BIG's float64 mirror (the explicit symmetrised inverse of ard_ref.lml_and_grad and loo_ref.closed) against a second
  float64 evaluation from the Cholesky factor (L^-1 by a triangular solve, K_y^-1 = L^-T L^-1, alpha by two triangular
  solves): every quantity agrees to a tenth of the bar the device is held to;
* SMALL and MID (cond K_y 1.1e6 and 2.6e6): both float64 evaluations of the LOO values against a long-double one -- float64
  misses the plain bars of the log probabilities, and of MID's means, which is why the GPU module holds those to the long
  double evaluation with 10 x float64's own miss (the rule of tests/test_sparse_grad_gpu.py::_reference), from the table
  held here."""
import numpy as np
import pytest
from scipy.linalg import solve_triangular

import ard_ref as R
import gemm_route_table as T
import loo_ref as LR
import test_postfit_routes_gpu as G
from test_gemm_route_cpu import MI355X_GROUPS, query, route_check       # noqa: F401 (route_check is a fixture)

C = T.Case
SITES = ("trsm", "sweep", "gram", "loo")
GEMM_OPTIONS = ("gemm_small_tiles", "gemm_small_dma", "gemm_tall", "tall_min_tiles", "gemm_ticket", "gemm_persist")
LDS_DMA_OPTIONS = [dict(gemm_tall=1, tall_min_tiles=0), dict(gemm_tall=0), dict(gemm_persist=0), dict(gemm_persist=1),
                   dict(gemm_ticket=1), dict(gemm_ticket=2)]
SMALL8, SMALL3 = "gemm_nt_small_kernel<8>", "gemm_nt_small_kernel<3>"
REG128, REG64 = "gemm_nt_kernel<4, 4, false>", "gemm_nt_kernel<2, 2, false>"
DMA8, TALL = "gemm_nt_dma_kernel<2, false>", "gemm_nt_dma_tall_kernel<false>"
TICKET, PERSIST = "gemm_nt_dma_ticket_kernel", "gemm_nt_dma_persist_kernel"
LDS_DMA_FAMILY = (DMA8, TALL, TICKET, PERSIST)


def routes_of(name):
    return G.BIG_ROUTES if name == "BIG" else G.ROUTES


def np_of(N):
    return (N + 127) // 128 * 128


# ---------------------------------------------------------------------------------------------------- the GEMM launches
def trsm_updates(m, w, leaf):
    """trsm_rec (driver.hip): the updates inside the triangular solve of one block of w columns, m rows"""
    if w <= leaf:
        return []
    h = (w // 2) // leaf * leaf
    return trsm_updates(m, h, leaf) + [C(m, w - h, h)] + trsm_updates(m, w - h, leaf)


def form(opts, Np):
    """-> block size, lookahead and leaf width of a resident factor of Np columns under a route's options (gpmi_ctx::block
    and lookahead_for below 12288 columns; trsm_rec's leaf), and the options gemm_route reads"""
    o = dict(G.DEFAULTS, **opts)
    nb = o["nb"] or 512
    la = bool(o["lookahead"]) and Np > nb and Np >= o["la_min"]
    return nb, la, 128 if o["panel_fused"] else 64, {k: v for k, v in opts.items() if k in GEMM_OPTIONS}


def postfit_launches(N, nb, la, leaf):
    """-> [(site, Case, (small_lds, chip_shared))] of one gpmi_loo_grad behind a fit of N points, in launch order: the
    front shared by every gradient (inverse_transposed, neg_gram_lower) and the LOO gradient's own product.  All have
    role 0.  The sweep's SharingScope: alone without lookahead, and_chip_shared below 2048 rows, beside_update from there"""
    Np = np_of(N)
    sharing = (0, 0) if not la else (1, 1) if Np >= 2048 else (0, 1)
    out = []
    for k in range(0, Np, nb):                                   # solve_sweep_factor(tri = true), m = Np
        w = min(nb, Np - k)
        rows = min(Np, k + w)
        out += [("trsm", case, sharing) for case in trsm_updates(rows, w, leaf)]
        r0 = k + w
        if r0 >= Np:
            continue
        if not la:
            out.append(("sweep", C(rows, Np - r0, w), sharing))
            continue
        nbn = min(nb, Np - r0)
        out.append(("sweep", C(rows, nbn, w), sharing))
        if r0 + nbn < Np:
            out.append(("sweep", C(rows, Np - r0 - nbn, w), sharing))
    for r0 in range(0, Np, nb):                                  # neg_gram_lower
        w = min(nb, Np - r0)
        out.append(("gram", C(w, r0 + w, Np - r0, lower=1, diag_off=r0), (0, 0)))
    NB = min(nb, Np)
    for r0 in range(0, N, NB):                                   # loo_grad_impl: a row block of padding only is not launched
        out.append(("loo", C(min(NB, Np - r0), Np, Np), (0, 0)))
    return out


def tiles(case):
    return (case.M // 128) * ((case.N + 127) // 128)


def ask(case, sharing, **more):
    return query(MI355X_GROUPS, "small_dma8", case, sharing=sharing, **more)


def route_launches(name, route):
    nb, la, leaf, gemm_opts = form(routes_of(name)[route], np_of(G.PROBLEMS[name][0]))
    return postfit_launches(G.PROBLEMS[name][0], nb, la, leaf), gemm_opts


def kernels(route_check, name, route, **more):
    """-> [(site, Case, kernel)] of every launch of (problem, route); more: options on top of the route's"""
    todo, gemm_opts = route_launches(name, route)
    got = route_check([ask(case, sharing, **dict(gemm_opts, **more)) for _, case, sharing in todo])
    return [(site, case, g) for (site, case, _), g in zip(todo, got)]


def summary(answers):
    """-> {site: {kernel: launches}}"""
    out = {}
    for site, _, kernel in answers:
        out.setdefault(site, {}).setdefault(kernel, 0)
        out[site][kernel] += 1
    return out


def large(answers):
    return [(site, str(case), kernel) for site, case, kernel in answers if tiles(case) >= 128]


def test_the_launch_shapes_are_the_ones_claimed():
    assert {n: np_of(p[0]) for n, p in G.PROBLEMS.items()} == {"SMALL": 768, "MID": 1536, "BIG": 3072}
    assert {n: p[0] - (np_of(p[0]) - 128) for n, p in G.PROBLEMS.items()} == {"SMALL": 1, "MID": 92, "BIG": 6}   # real rows of the last tile
    # MID at the default block: three blocks; the sweep clips its rows, the Gram's K shrinks, the LOO product does neither
    todo = postfit_launches(1500, 512, False, 128)
    assert [str(c) for s, c, _ in todo if s == "sweep"] == ["512x1024xK512", "1024x512xK512"]
    assert [(c.M, c.N, c.K, c.lower, c.diag_off) for s, c, _ in todo if s == "gram"] == [(512, 512, 1536, 1, 0), (512, 1024, 1024, 1, 512),
                                                                                          (512, 1536, 512, 1, 1024)]
    assert [str(c) for s, c, _ in todo if s == "loo"] == ["512x1536xK1536"] * 3
    # lookahead splits every update but the last in two, and the sharing state follows the rows of the sweep
    assert [str(c) for s, c, _ in postfit_launches(1500, 512, True, 128) if s == "sweep"] == ["512x512xK512"] * 2 + ["1024x512xK512"]
    assert {sh for s, _, sh in postfit_launches(1500, 512, True, 128) if s in ("trsm", "sweep")} == {(0, 1)}
    assert {sh for s, _, sh in postfit_launches(2950, 512, True, 128) if s in ("trsm", "sweep")} == {(1, 1)}
    assert {sh for s, _, sh in postfit_launches(2950, 512, True, 128) if s in ("gram", "loo")} == {(0, 0)}
    # first-generation leaves: 64-column updates inside trsm_block
    assert min(c.N for s, c, _ in postfit_launches(641, 512, False, 64) if s == "trsm") == 64
    assert min(c.N for s, c, _ in postfit_launches(641, 512, False, 128) if s == "trsm") == 128
    # BIG: a last LOO row block, 2950 = 2 x 1024 + 902; under nb = 128 the last block of MID (92 real rows) is launched
    assert len([1 for s, _, _ in postfit_launches(2950, 1024, False, 128) if s == "loo"]) == 3
    assert len([1 for s, _, _ in postfit_launches(1500, 128, False, 128) if s == "loo"]) == 12
    # which routes run under lookahead, and with which blocks
    for name, Np in (("SMALL", 768), ("MID", 1536), ("BIG", 3072)):
        forms = {route: form(opts, Np)[:3] for route, opts in routes_of(name).items()}
        assert {r for r, f in forms.items() if f[1]} == {"la256_deep", "la256_shallow"}, name
        assert {r for r, f in forms.items() if f[2] == 64} == ({"panel_fused0"} if name != "BIG" else set())
    assert {r: form(o, 3072)[0] for r, o in G.BIG_ROUTES.items()} == dict(
        default=512, nb1024=1024, la256_deep=512, la256_shallow=512, tall=512, tall_nb1024=1024, ticket2_nb2048=2048, nb3072=3072,
        persist0_nb3072=3072)


# ---------------------------------------------------------------------------------------------------- recorded kernels
# {problem: {route: {site: {kernel: launches}}}}: what gemm_route answered when these tests were written
def one(kernel, trsm, sweep, gram, loo):
    """every launch on the same kernel: the launches per site"""
    return {site: {kernel: n} for site, n in zip(SITES, (trsm, sweep, gram, loo)) if n}


RECORD = {
    "SMALL": {
        "default": one(SMALL8, 4, 1, 2, 2), "nb128": one(SMALL8, 0, 5, 6, 6), "nb256": one(SMALL8, 3, 2, 3, 3),
        "lookahead0": one(SMALL8, 4, 1, 2, 2), "la256_deep": one(SMALL8, 4, 1, 2, 2), "la256_shallow": one(SMALL8, 4, 1, 2, 2),
        "panel_fused0": one(SMALL8, 10, 1, 2, 2), "trsv_vinv0": one(SMALL8, 4, 1, 2, 2), "trsv_vinv1": one(SMALL8, 4, 1, 2, 2),
        "trsv_vinv2": one(SMALL8, 4, 1, 2, 2), "small_tiles0": one(REG128, 4, 1, 2, 2), "small_dma0": one(REG64, 4, 1, 2, 2),
    },
    "MID": {
        "default": one(SMALL8, 9, 2, 3, 3), "nb128": one(SMALL8, 0, 11, 12, 12), "nb256": one(SMALL8, 6, 5, 6, 6),
        "lookahead0": one(SMALL8, 9, 2, 3, 3), "la256_deep": one(SMALL8, 9, 3, 3, 3), "la256_shallow": one(SMALL8, 9, 3, 3, 3),
        "panel_fused0": one(SMALL8, 21, 2, 3, 3), "trsv_vinv0": one(SMALL8, 9, 2, 3, 3), "trsv_vinv1": one(SMALL8, 9, 2, 3, 3),
        "trsv_vinv2": one(SMALL8, 9, 2, 3, 3), "small_tiles0": one(REG128, 9, 2, 3, 3), "small_dma0": one(REG64, 9, 2, 3, 3),
    },
    "BIG": {
        "default": {"trsm": {SMALL8: 18}, "sweep": {SMALL8: 2, DMA8: 3}, "gram": {SMALL8: 6}, "loo": {SMALL8: 6}},
        "nb1024": {"trsm": {SMALL8: 21}, "sweep": {DMA8: 2}, "gram": {SMALL8: 1, DMA8: 2}, "loo": {DMA8: 3}},
        "la256_deep": {"trsm": {SMALL3: 18}, "sweep": {SMALL3: 9}, "gram": {SMALL8: 6}, "loo": {SMALL8: 6}},
        "la256_shallow": {"trsm": {SMALL3: 18}, "sweep": {SMALL3: 9}, "gram": {SMALL8: 6}, "loo": {SMALL8: 6}},
        "tall": {"trsm": {SMALL8: 18}, "sweep": {SMALL8: 2, TALL: 3}, "gram": {SMALL8: 6}, "loo": {SMALL8: 6}},
        "tall_nb1024": {"trsm": {SMALL8: 21}, "sweep": {TALL: 2}, "gram": {SMALL8: 1, TALL: 2}, "loo": {TALL: 3}},
        "ticket2_nb2048": {"trsm": {SMALL8: 21, DMA8: 1}, "sweep": {DMA8: 1}, "gram": {DMA8: 2}, "loo": {TICKET: 1, DMA8: 1}},
        "nb3072": {"trsm": {SMALL8: 20, DMA8: 3}, "gram": {DMA8: 1}, "loo": {PERSIST: 1}},
        "persist0_nb3072": {"trsm": {SMALL8: 20, DMA8: 3}, "gram": {DMA8: 1}, "loo": {DMA8: 1}},
    },
}
# BIG: the launches of at least 128 tiles, (site, shape, kernel) in launch order
SWEEP512 = ["1024x2048xK512", "1536x1536xK512", "2048x1024xK512"]
NB1024 = [("sweep", "1024x2048xK1024"), ("sweep", "2048x1024xK1024"), ("gram", "1024x2048xK2048-lower+1024"),
          ("gram", "1024x3072xK1024-lower+2048")] + [("loo", "1024x3072xK3072")] * 3
NB2048 = [("trsm", "2048x1024xK1024"), ("sweep", "2048x1024xK2048"), ("gram", "2048x2048xK3072-lower+0"),
          ("gram", "1024x3072xK1024-lower+2048")]
NB3072 = [("trsm", "3072x768xK768"), ("trsm", "3072x1536xK1536"), ("trsm", "3072x768xK768"), ("gram", "3072x3072xK3072-lower+0")]
BIG_LARGE = {
    "default": [("sweep", shape, DMA8) for shape in SWEEP512],
    "nb1024": [(site, shape, DMA8) for site, shape in NB1024],
    "la256_deep": [],                     # the split updates have 96 tiles at the most (1024 x 1536, 1536 x 1024)
    "la256_shallow": [],
    "tall": [("sweep", shape, TALL) for shape in SWEEP512],
    "tall_nb1024": [(site, shape, TALL) for site, shape in NB1024],
    "ticket2_nb2048": [(site, shape, DMA8) for site, shape in NB2048] + [("loo", "2048x3072xK3072", TICKET), ("loo", "1024x3072xK3072", DMA8)],
    "nb3072": [(site, shape, DMA8) for site, shape in NB3072] + [("loo", "3072x3072xK3072", PERSIST)],
    "persist0_nb3072": [(site, shape, DMA8) for site, shape in NB3072] + [("loo", "3072x3072xK3072", DMA8)],
}


@pytest.mark.parametrize("name", list(G.PROBLEMS))
def test_every_launch_reaches_the_recorded_kernel(route_check, name):
    assert sorted(RECORD[name]) == sorted(routes_of(name))
    for route in routes_of(name):
        answers = kernels(route_check, name, route)
        assert summary(answers) == RECORD[name][route], (name, route, summary(answers))
        if name == "BIG":
            assert large(answers) == BIG_LARGE[route], (route, large(answers))
        else:
            assert not large(answers)
        # the family is entered by the tile count alone at these shapes
        for site, case, kernel in answers:
            assert (kernel in LDS_DMA_FAMILY) == (tiles(case) >= 128), (name, route, site, str(case), kernel)


@pytest.mark.parametrize("name", ["SMALL", "MID"])
def test_the_lds_dma_options_cannot_reach_small_and_mid(route_check, name):
    """fewer than 128 tiles of 128 x 128 in every launch of every route: the same kernel under every value of gemm_tall,
    gemm_persist and gemm_ticket -- those options get no route at these shapes"""
    for route in G.ROUTES:
        base = kernels(route_check, name, route)
        assert base and max(tiles(case) for _, case, _ in base) < 128
        for more in LDS_DMA_OPTIONS:
            assert kernels(route_check, name, route, **more) == base, (name, route, more)
    print("%s: the largest launch has %d tiles" % (name, max(tiles(case) for r in G.ROUTES for _, case, _ in kernels(route_check, name, r))))


def test_the_small_tile_options_can(route_check):
    for name in ("SMALL", "MID"):
        assert {k for _, _, k in kernels(route_check, name, "default")} == {SMALL8}
        assert {k for _, _, k in kernels(route_check, name, "la256_deep")} == {SMALL8}       # and_chip_shared keeps the deep ring
        assert {k for _, _, k in kernels(route_check, name, "small_tiles0")} == {REG128}
        assert {k for _, _, k in kernels(route_check, name, "small_dma0")} == {REG64}
        assert {k for _, c, k in kernels(route_check, name, "panel_fused0") if c.N % 128} == {SMALL8}


def test_big_reaches_the_lds_dma_family_at_every_site(route_check):
    """the condition tests/test_postfit_routes_gpu.py rests on: the tri sweep's update, neg_gram_lower and the LOO
    gradient's row-block product each run on a kernel of the 128-tile family under at least one BIG route, and each of
    tall, ticket2 and persist changes at least one kernel against the route that differs in that option alone"""
    got = {route: kernels(route_check, "BIG", route) for route in G.BIG_ROUTES}
    reached = {site: sorted({(route, k) for route, ans in got.items() for s, _, k in ans if s == site and k in LDS_DMA_FAMILY})
               for site in SITES}
    for site in ("sweep", "gram", "loo"):
        print("%s: %s" % (site, reached[site]))
        assert reached[site], site
    assert {k for _, k in reached["sweep"]} == {DMA8, TALL}
    assert {k for _, k in reached["gram"]} == {DMA8, TALL}
    assert {k for _, k in reached["loo"]} == {DMA8, TALL, TICKET, PERSIST}
    # beside_update: every launch of the sweep on the 3-stage ring, nothing on it elsewhere
    for route in ("la256_deep", "la256_shallow"):
        assert {k for s, _, k in got[route] if s in ("trsm", "sweep")} == {SMALL3}
        assert {k for s, _, k in got[route] if s in ("gram", "loo")} == {SMALL8}

    def changed(route, other):
        a, b = got[route], got[other]
        assert [(s, c) for s, c, _ in a] == [(s, c) for s, c, _ in b]
        return [(s, str(c), kb, ka) for (s, c, ka), (_, _, kb) in zip(a, b) if ka != kb]

    assert {(s, ka) for s, _, _, ka in changed("tall", "default")} == {("sweep", TALL)}
    assert {(s, ka) for s, _, _, ka in changed("tall_nb1024", "nb1024")} == {("sweep", TALL), ("gram", TALL), ("loo", TALL)}
    assert changed("nb3072", "persist0_nb3072") == [("loo", "3072x3072xK3072", DMA8, PERSIST)]
    # ticket2 against the same blocks without it
    base = kernels(route_check, "BIG", "ticket2_nb2048", gemm_ticket=0)
    assert [(s, str(c), kb, ka) for (s, c, ka), (_, _, kb) in zip(got["ticket2_nb2048"], base) if ka != kb] == [
        ("loo", "2048x3072xK3072", DMA8, TICKET)]
    # and why blocks of 512 and 1024 would not do: neither option changes a kernel there
    for route in ("default", "nb1024"):
        for more in (dict(gemm_ticket=2), dict(gemm_persist=0), dict(gemm_ticket=1)):
            assert kernels(route_check, "BIG", route, **more) == got[route], (route, more)


# ------------------------------------------------------------------------------------------------------------ the mirror
def cholesky_evaluation(name):
    """the quantities of a device run in float64 without numpy.linalg.inv: U = L^-T from a triangular solve on the identity,
    K_y^-1 = U U^T, alpha by two triangular solves -- the formulas of ard_ref.lml_and_grad and loo_ref.closed otherwise"""
    X, y, r = G.inputs(name)
    N, d, noise = G.PROBLEMS[name]
    sigma, l = G.SIGMA, G.ELL
    z = R.scaled(X, r)
    part = lambda k: (z[:, None, k] - z[None, :, k]) ** 2      # noqa: E731
    sq = np.zeros((N, N))
    for k in range(d):
        sq += part(k)
    K = sigma ** 2 * np.exp(-.5 / l ** 2 * sq)
    L = np.linalg.cholesky(K + noise * np.eye(N))
    Linv = solve_triangular(L, np.eye(N), lower=True)
    Kinv = Linv.T @ Linv
    m = solve_triangular(L, y, lower=True)
    alpha = solve_triangular(L, m, lower=True, trans="T")
    out = {"lml": -.5 * (m @ m) - np.sum(np.log(np.diag(L))) - .5 * N * np.log(2 * np.pi), "alpha": alpha}

    def trace(D):
        return .5 * (alpha @ D @ alpha) - .5 * np.sum(Kinv * D)

    g_l, g_sigma = trace(K * sq / l ** 3), trace(2 * K / sigma)
    out["lml_grad"] = (g_l, g_sigma)
    out["lml_grad_ard"] = (np.array([trace(K * part(k) / (l ** 2 * r[k])) for k in range(d)]), g_l, g_sigma, trace(np.eye(N)))
    kappa = np.sum(Linv * Linv, axis=0)                          # the squared norms of the rows of U
    mu, var = y - alpha / kappa, 1.0 / kappa
    logp = LR._logp(y, mu, var)
    out["loo"] = (mu, var, logp, float(np.sum(logp)))

    def loo_term(dK):
        Z = Kinv @ dK
        s = np.sum(Z * Kinv, axis=1)
        return float(np.sum(alpha * (Z @ alpha) / kappa - .5 * (1.0 + alpha ** 2 / kappa) * s / kappa))

    out["loo_grad"] = (loo_term(K * sq / l ** 3), loo_term(2 * K / sigma), loo_term(np.eye(N)))
    return out


@pytest.mark.parametrize("name", G.LOO_LONG_DOUBLE)
def test_float64_misses_the_loo_bars_at_small_and_mid(name):
    """why the LOO values of SMALL and MID are held to a long-double evaluation with measured bars
    (test_postfit_routes_gpu.loo_reference): the two float64 evaluations -- the mirror's explicit inverse and the
    Cholesky factor -- against long double, in the normalisation of test_loo_gpu._hold_values.  The log probabilities
    miss their plain bar by a factor 16 to 70, MID's means by 1.16 (Cholesky) where the mirror stays at 0.93.  The worse
    of the two is the table the GPU module takes its bars from, held here within a factor 2"""
    X, y, r, ard, loo = G.mirror(name)
    ref, bars = G.loo_reference(name)
    by_inverse = G.loo_errors(G.as_tuple(loo), ref, y)
    by_cholesky = G.loo_errors(G.as_tuple(G.loo_values(name, np.float64)), ref, y)
    apart = G.loo_errors(G.as_tuple(G.loo_values(name, np.float64)), loo, y)
    print("%s cond %.2e, float64 against long double / plain bar: explicit inverse %s | Cholesky %s | the two apart %s" % (
        name, loo["cond"], *("  ".join("%s %.2f" % (k, e[k] / G.LOO_PLAIN[k]) for k in e) for e in (by_inverse, by_cholesky, apart))))
    assert np.finfo(G.LD).eps < 1e-18                            # long double is wider than float64 here
    assert apart["logp"] > 10 * G.LOO_PLAIN["logp"]
    for k, recorded in G.LOO_FLOAT64_MISS[name].items():
        worse = max(by_inverse[k], by_cholesky[k])
        assert recorded / 2 <= worse <= 2 * recorded, (name, k, worse, recorded)
        assert bars[k] == (G.LOO_PLAIN[k] if recorded <= G.LOO_PLAIN[k] else 10 * recorded)
    assert {k for k in bars if bars[k] > G.LOO_PLAIN[k]} == ({"logp"} if name == "SMALL" else {"mu", "logp"})


def test_two_float64_evaluations_of_big_agree():
    """the explicit symmetrised inverse (the mirror) against the Cholesky evaluation: each quantity a tenth of its bar apart
    at the most, so the float64 mirror at N = 2950 does not use up the bars of the GPU test.  Measured: LOO values 0.029
    (the log probabilities), every other quantity below 1e-4; at noise 1e-2 the LOO values were 0.74 of their bar apart"""
    X, y, r, ard, loo = G.mirror("BIG")
    ratio = G.ratios(cholesky_evaluation("BIG"), ard, loo, y)
    print("BIG cond %.2e: two float64 evaluations, difference / bar  " % loo["cond"] + "  ".join("%s %.2e" % kv for kv in ratio.items()))
    assert sorted(ratio) == sorted(G.CALLS)
    assert 1e4 <= loo["cond"] <= 1e5
    for k, v in ratio.items():
        assert v <= 0.1, (k, v)
