"""What tests/test_predict_routes_gpu.py rests on, without a GPU:

* the GEMM launches of its (problem, test set) pairs in each of the three forms of a prediction, written out from
  csrc/driver.hip and csrc/regress.hip (site_launches; FORM_SITES says which form runs which):
    sweep      solve_sweep_factor with tri = false, m = np_ rows: trsm_rec's inner updates and the sweep's own, split in
               two under lookahead (two_call)
    fit        cholesky_inplace of the plain fit, ncols = Np, nrows = Np + 128: panel_rec's inner updates (lower,
               diag_off = r0 - c0) and the trailing updates (two_call)
    carried    the same with nrows = Np + 128 + np_: the test rows ride below the triangle (one_pass)
    augmented  ncols = Np + np_, nrows = Np + np_ + 128 (augmented)
    post_gemm  post_factor_device's one gemm_minus_lower, np_ x np_ at K = Np (every form that forms the factor in P)
    post_chol  cholesky_inplace of P, ncols = nrows = np_
  Under lookahead the trailing update is two launches, (a) the next block column with role 0 and (b) the rest with
  role 1; the Cholesky's own updates run beside_update, its panels chip_shared_only below shallow_min columns;
* the kernel gemm_route (csrc/gpmi_route.h, through tests/sanitize/gemm_route_check.cpp) answers for every one of them
  under every route, held against the names recorded below (RECORD);
* SMALL, MID and FULL: the launches have fewer than 128 tiles, and no value of gemm_tall, gemm_persist and gemm_ticket
  changes their kernel -- but for the launches of LARGE_BELOW_BIG, all of them trailing updates of a Cholesky on
  chol_trailing_update_dma_kernel: MID's augmented factorisation of 2304 columns and 2432 rows has a first update of
  1920 x 1792 (210 tiles) at blocks of 512, and blocks of 128 and 256 put the first updates of MID's fit, carried and
  augmented forms and of SMALL n = 700's augmented form over the line (BIG's routes run that site under the options);
* BIG: each of the sweep, the carried update, the augmented update and the posterior GEMM reaches the 128-tile LDS-DMA
  family under at least one route, and each of tall, ticket2 and persist changes at least one kernel of the prediction
  side against the route without it;
* whether carrying the test rows moves a launch of the fit to another kernel (fit against carried, launch by launch):
  the statement "lml, m, diag and alpha of one_pass equal two_call's bit for bit" is read against this list;
* SMALL, MID and FULL: both float64 evaluations of tests/predict_ref.py (LAPACK, and the factorisation in 384-wide
  blocks) against the long-double one, per quantity: the table the GPU module takes its bars from (FLOAT64_MISS), held
  within a factor 2;
* BIG (long double takes minutes): the distance between the two float64 evaluations (FLOAT64_APART), held the same way;
* the two breaks the bars are there for, done to a float64 evaluation: one entry of the posterior factor off by 1e-8,
  and the last K step of the posterior GEMM lost (FULL: the other problems end in padding)."""
import numpy as np
import pytest
from scipy.linalg import solve_triangular

import ard_ref as R
import gemm_route_table as T
import predict_ref as P
import test_postfit_routes_cpu as PC
import test_predict_routes_gpu as G
from test_gemm_route_cpu import MI355X_GROUPS, query, route_check       # noqa: F401 (route_check is a fixture)
from test_postfit_routes_cpu import (DMA8, LDS_DMA_FAMILY, LDS_DMA_OPTIONS, PERSIST, REG64, REG128, SMALL3, SMALL8, TALL,
                                     TICKET, np_of, tiles, trsm_updates)

C = T.Case
DMA8_TRAIL, TALL_TRAIL = "chol_trailing_update_dma_kernel", "chol_trailing_update_dma256_kernel"
PERSIST_TRAIL, TICKET_TRAIL = "chol_trailing_update_persist_kernel", "chol_trailing_update_ticket_kernel"
FAMILY = LDS_DMA_FAMILY + (DMA8_TRAIL, TALL_TRAIL, PERSIST_TRAIL, TICKET_TRAIL)
REG128X64 = "gemm_nt_kernel<4, 2, false>"
FORM_SITES = {"two_call": ("fit", "sweep", "post_gemm", "post_chol"), "one_pass": ("carried", "post_gemm", "post_chol"),
              "augmented": ("augmented", "post_gemm", "post_chol")}
SITES = ("fit", "sweep", "carried", "augmented", "post_gemm", "post_chol")
PREDICTION_SITES = SITES[1:]
ALONE, CHIP_SHARED, BESIDE = (0, 0), (0, 1), (1, 1)


# ---------------------------------------------------------------------------------------------------- the GEMM launches
def form(opts, ncols):
    """-> block size, lookahead, leaf width and shallow_min of a blocked sweep over ncols columns under a route's options
    (gpmi_ctx::block and lookahead_for below 12288 columns; the leaves of panel_rec and trsm_rec)"""
    o = dict(G.DEFAULTS, **opts)
    nb = o["nb"] or 512
    la = bool(o["lookahead"]) and ncols > nb and ncols >= o["la_min"]
    return nb, la, 128 if o["panel_fused"] else 64, o["shallow_min"]


def panel_updates(mrows, w, leaf, off=0):
    """panel_rec (driver.hip): the updates inside the factorisation of a block column of w columns, mrows rows from its
    diagonal block down.  Rows start at the 128-aligned row at or above the updated columns"""
    if w <= leaf:
        return []
    h = (w // 2) // leaf * leaf
    c0 = off + h
    r0 = c0 // 128 * 128
    return (panel_updates(mrows, h, leaf, off) + [C(mrows - r0, w - h, h, lower=1, diag_off=r0 - c0)] +
            panel_updates(mrows, w - h, leaf, c0))


def cholesky_launches(site, ncols, nrows, opts):
    """cholesky_inplace -> [(site, Case, sharing, role)] in launch order"""
    nb_, la, leaf, shallow_min = form(opts, ncols)
    out = []
    for k in range(0, ncols, nb_):
        nb = min(nb_, ncols - k)
        sharing = ALONE if not la else BESIDE if ncols - k >= shallow_min else CHIP_SHARED
        out += [(site, case, sharing, 0) for case in panel_updates(nrows - k, nb, leaf)]
        r0 = k + nb
        if r0 >= ncols:
            continue
        if not la:
            out.append((site, C(nrows - r0, ncols - r0, nb, lower=1), ALONE, 1))
            continue
        nbn = min(nb_, ncols - r0)
        out.append((site, C(nrows - r0, nbn, nb, lower=1), BESIDE, 0))
        if r0 + nbn < ncols:
            out.append((site, C(nrows - r0 - nbn, ncols - r0 - nbn, nb, lower=1), BESIDE, 1))
    return out


def sweep_launches(Np, m, opts):
    """solve_sweep_factor with tri = false: every launch has m rows"""
    nb_, la, leaf, _ = form(opts, Np)
    sharing = ALONE if not la else BESIDE if m >= 2048 else CHIP_SHARED
    out = []
    for k in range(0, Np, nb_):
        nb = min(nb_, Np - k)
        out += [("sweep", case, sharing, 0) for case in trsm_updates(m, nb, leaf)]
        r0 = k + nb
        if r0 >= Np:
            continue
        if not la:
            out.append(("sweep", C(m, Np - r0, nb), sharing, 0))
            continue
        nbn = min(nb_, Np - r0)
        out.append(("sweep", C(m, nbn, nb), sharing, 0))
        if r0 + nbn < Np:
            out.append(("sweep", C(m, Np - r0 - nbn, nb), sharing, 0))
    return out


def site_launches(site, N, n, opts):
    Np, np_ = np_of(N), np_of(n)
    if site == "sweep":
        return sweep_launches(Np, np_, opts)
    if site == "post_gemm":
        return [(site, C(np_, np_, Np, lower=1), ALONE, 0)]
    ncols, nrows = {"fit": (Np, Np + 128), "carried": (Np, Np + 128 + np_), "augmented": (Np + np_, Np + np_ + 128),
                    "post_chol": (np_, np_)}[site]
    return cholesky_launches(site, ncols, nrows, opts)


def routes_of(name):
    return G.BIG_ROUTES if name == "BIG" else G.ROUTES


def ask(case, sharing, role, **opts):
    words = query(MI355X_GROUPS, "small_dma8", case, sharing=sharing, **opts).split()
    words[3] = str(role)
    return " ".join(words)


def kernels(route_check, name, n, route, sites=SITES, **more):
    """-> [(site, Case, role, kernel)] of every launch of (problem, test set, route); more: options on top of the route's"""
    opts = routes_of(name)[route]
    gemm_opts = dict({k: v for k, v in opts.items() if k in PC.GEMM_OPTIONS}, **more)
    todo = [l for site in sites for l in site_launches(site, G.SIZES[name][0], n, opts)]
    got = route_check([ask(case, sharing, role, **gemm_opts) for _, case, sharing, role in todo])
    return [(site, case, role, g) for (site, case, _, role), g in zip(todo, got)]


def summary(answers):
    """-> {site: {kernel: launches}}"""
    out = {}
    for site, _, _, kernel in answers:
        out.setdefault(site, {}).setdefault(kernel, 0)
        out[site][kernel] += 1
    return out


def large(answers):
    return [(site, str(case), kernel) for site, case, _, kernel in answers if tiles(case) >= 128]


# ---------------------------------------------------------------------------------------------------- recorded kernels
# {(problem, n): [(routes, {site: {kernel: launches}})]}: what gemm_route answered when these tests were written.  A site
# without a GEMM launch (a posterior factor of one tile, of one leaf) has no entry
STEADY = "default lookahead0 trsv_vinv0 trsv_vinv1 trsv_vinv2"


def every(kernel, fit, sweep, carried, augmented, post_gemm, post_chol):
    """every launch on the same kernel: the launches per site"""
    return {site: {kernel: k} for site, k in zip(SITES, (fit, sweep, carried, augmented, post_gemm, post_chol)) if k}


RECORD = {
    ("SMALL", 37): [
        (STEADY + " nb128 nb256", every(SMALL8, 5, 5, 5, 6, 1, 0)),
        ("la256_deep", {"fit": {SMALL3: 5}, "sweep": {SMALL8: 5}, "carried": {SMALL3: 5}, "augmented": {SMALL3: 6}, "post_gemm": {SMALL8: 1}}),
        ("la256_shallow", {"fit": {SMALL8: 4, SMALL3: 1}, "sweep": {SMALL8: 5}, "carried": {SMALL8: 4, SMALL3: 1},
                           "augmented": {SMALL8: 5, SMALL3: 1}, "post_gemm": {SMALL8: 1}}),
        ("panel_fused0", every(SMALL8, 11, 11, 11, 13, 1, 1)),
        ("small_tiles0", every(REG128, 5, 5, 5, 6, 1, 0)),
        ("small_dma0", every(REG64, 5, 5, 5, 6, 1, 0)),
    ],
    ("SMALL", 300): [
        (STEADY + " nb128 nb256", every(SMALL8, 5, 5, 5, 8, 1, 2)),
        ("la256_deep", {"fit": {SMALL3: 5}, "sweep": {SMALL8: 5}, "carried": {SMALL3: 5}, "augmented": {SMALL3: 9}, "post_gemm": {SMALL8: 1},
                        "post_chol": {SMALL8: 2}}),
        ("la256_shallow", {"fit": {SMALL8: 4, SMALL3: 1}, "sweep": {SMALL8: 5}, "carried": {SMALL8: 4, SMALL3: 1},
                           "augmented": {SMALL8: 6, SMALL3: 3}, "post_gemm": {SMALL8: 1}, "post_chol": {SMALL8: 2}}),
        ("panel_fused0", every(SMALL8, 11, 11, 11, 17, 1, 5)),
        ("small_tiles0", every(REG128, 5, 5, 5, 8, 1, 2)),
        ("small_dma0", every(REG64, 5, 5, 5, 8, 1, 2)),
    ],
    ("SMALL", 700): [
        (STEADY + " nb256", every(SMALL8, 5, 5, 5, 11, 1, 5)),
        ("nb128", dict(every(SMALL8, 5, 5, 5, 0, 1, 5), augmented={DMA8_TRAIL: 1, SMALL8: 10})),
        ("la256_deep", {"fit": {SMALL3: 5}, "sweep": {SMALL8: 5}, "carried": {SMALL3: 5}, "augmented": {SMALL3: 12}, "post_gemm": {SMALL8: 1},
                        "post_chol": {SMALL3: 5}}),
        ("la256_shallow", {"fit": {SMALL8: 4, SMALL3: 1}, "sweep": {SMALL8: 5}, "carried": {SMALL8: 4, SMALL3: 1},
                           "augmented": {SMALL8: 9, SMALL3: 3}, "post_gemm": {SMALL8: 1}, "post_chol": {SMALL8: 4, SMALL3: 1}}),
        ("panel_fused0", every(SMALL8, 11, 11, 11, 23, 1, 11)),
        ("small_tiles0", every(REG128, 5, 5, 5, 11, 1, 5)),
        ("small_dma0", every(REG64, 5, 5, 5, 11, 1, 5)),
    ],
    ("MID", 700): [
        (STEADY, dict(every(SMALL8, 11, 11, 11, 0, 1, 5), augmented={SMALL8: 16, DMA8_TRAIL: 1})),
        ("nb128", {"fit": {DMA8_TRAIL: 1, SMALL8: 10}, "sweep": {SMALL8: 11}, "carried": {DMA8_TRAIL: 3, SMALL8: 8},
                   "augmented": {DMA8_TRAIL: 7, SMALL8: 10}, "post_gemm": {SMALL8: 1}, "post_chol": {SMALL8: 5}}),
        ("nb256", {"fit": {SMALL8: 11}, "sweep": {SMALL8: 11}, "carried": {SMALL8: 10, DMA8_TRAIL: 1}, "augmented": {SMALL8: 14, DMA8_TRAIL: 3},
                   "post_gemm": {SMALL8: 1}, "post_chol": {SMALL8: 5}}),
        ("la256_deep", {"fit": {SMALL3: 12}, "sweep": {SMALL8: 12}, "carried": {SMALL3: 12}, "augmented": {SMALL3: 20}, "post_gemm": {SMALL8: 1},
                        "post_chol": {SMALL3: 5}}),
        ("la256_shallow", {"fit": {SMALL8: 9, SMALL3: 3}, "sweep": {SMALL8: 12}, "carried": {SMALL8: 9, SMALL3: 3},
                           "augmented": {SMALL8: 13, SMALL3: 7}, "post_gemm": {SMALL8: 1}, "post_chol": {SMALL8: 4, SMALL3: 1}}),
        ("panel_fused0", dict(every(SMALL8, 23, 23, 23, 0, 1, 11), augmented={SMALL8: 34, DMA8_TRAIL: 1})),
        ("small_tiles0", dict(every(REG128, 11, 11, 11, 0, 1, 5), augmented={REG128: 16, DMA8_TRAIL: 1})),
        ("small_dma0", dict(every(REG64, 11, 11, 11, 0, 1, 5), augmented={REG64: 16, DMA8_TRAIL: 1})),
    ],
    ("BIG", 1000): [
        ("default", {"fit": {SMALL8: 20, DMA8_TRAIL: 3}, "sweep": {SMALL8: 21, DMA8: 2}, "carried": {SMALL8: 19, PERSIST_TRAIL: 1, DMA8_TRAIL: 3},
                     "augmented": {SMALL8: 26, PERSIST_TRAIL: 1, DMA8_TRAIL: 4}, "post_gemm": {SMALL8: 1}, "post_chol": {SMALL8: 7}}),
        ("nb1024", {"fit": {SMALL8: 22, DMA8_TRAIL: 1}, "sweep": {SMALL8: 22, DMA8: 1}, "carried": {SMALL8: 21, DMA8_TRAIL: 2},
                    "augmented": {SMALL8: 29, DMA8_TRAIL: 2}, "post_gemm": {SMALL8: 1}, "post_chol": {SMALL8: 7}}),
        ("la256_deep", {"fit": {SMALL3: 25, DMA8_TRAIL: 2}, "sweep": {SMALL8: 26, DMA8: 1}, "carried": {SMALL3: 24, DMA8_TRAIL: 3},
                        "augmented": {SMALL3: 33, DMA8_TRAIL: 4}, "post_gemm": {SMALL8: 1}, "post_chol": {SMALL3: 7}}),
        ("la256_shallow", {"fit": {SMALL8: 18, SMALL3: 7, DMA8_TRAIL: 2}, "sweep": {SMALL8: 26, DMA8: 1},
                           "carried": {SMALL8: 18, SMALL3: 6, DMA8_TRAIL: 3}, "augmented": {SMALL8: 24, SMALL3: 9, DMA8_TRAIL: 4},
                           "post_gemm": {SMALL8: 1}, "post_chol": {SMALL8: 6, SMALL3: 1}}),
        ("tall", {"fit": {SMALL8: 20, TALL_TRAIL: 3}, "sweep": {SMALL8: 21, TALL: 2}, "carried": {SMALL8: 19, PERSIST_TRAIL: 1, TALL_TRAIL: 3},
                  "augmented": {SMALL8: 26, PERSIST_TRAIL: 1, TALL_TRAIL: 4}, "post_gemm": {SMALL8: 1}, "post_chol": {SMALL8: 7}}),
        ("tall_nb1024", {"fit": {SMALL8: 22, TALL_TRAIL: 1}, "sweep": {SMALL8: 22, TALL: 1}, "carried": {SMALL8: 21, TALL_TRAIL: 2},
                         "augmented": {SMALL8: 29, TALL_TRAIL: 2}, "post_gemm": {SMALL8: 1}, "post_chol": {SMALL8: 7}}),
        ("ticket2_nb2048", {"fit": {SMALL8: 22, DMA8: 1}, "sweep": {SMALL8: 23}, "carried": {SMALL8: 21, DMA8: 1, DMA8_TRAIL: 1},
                            "augmented": {SMALL8: 29, DMA8: 1, DMA8_TRAIL: 1}, "post_gemm": {SMALL8: 1}, "post_chol": {SMALL8: 7}}),
        ("nb3072 persist0_nb3072", {"fit": {SMALL8: 22, DMA8: 1}, "sweep": {SMALL8: 23}, "carried": {SMALL8: 21, DMA8: 2},
                                    "augmented": {SMALL8: 29, DMA8: 2}, "post_gemm": {SMALL8: 1}, "post_chol": {SMALL8: 7}}),
    ],
    ("BIG", 2100): [
        ("default", {"fit": {SMALL8: 20, DMA8_TRAIL: 3}, "sweep": {SMALL8: 19, DMA8: 4}, "carried": {SMALL8: 19, PERSIST_TRAIL: 2, DMA8_TRAIL: 2},
                     "augmented": {SMALL8: 33, PERSIST_TRAIL: 3, DMA8_TRAIL: 4}, "post_gemm": {DMA8: 1}, "post_chol": {SMALL8: 15, DMA8_TRAIL: 1}}),
        ("nb1024", {"fit": {SMALL8: 22, DMA8_TRAIL: 1}, "sweep": {SMALL8: 21, DMA8: 2},
                    "carried": {SMALL8: 20, DMA8: 1, PERSIST_TRAIL: 1, DMA8_TRAIL: 1},
                    "augmented": {SMALL8: 36, DMA8: 1, PERSIST_TRAIL: 1, DMA8_TRAIL: 2}, "post_gemm": {DMA8: 1}, "post_chol": {SMALL8: 16}}),
        ("la256_deep", {"fit": {SMALL3: 25, DMA8_TRAIL: 2}, "sweep": {SMALL3: 24, DMA8: 3}, "carried": {SMALL3: 22, DMA8: 2, DMA8_TRAIL: 3},
                        "augmented": {SMALL3: 41, DMA8: 2, DMA8_TRAIL: 6}, "post_gemm": {DMA8: 1}, "post_chol": {SMALL3: 19}}),
        ("la256_shallow", {"fit": {SMALL8: 18, SMALL3: 7, DMA8_TRAIL: 2}, "sweep": {SMALL3: 24, DMA8: 3},
                           "carried": {SMALL8: 18, DMA8: 2, DMA8_TRAIL: 3, SMALL3: 4},
                           "augmented": {SMALL8: 30, DMA8: 2, DMA8_TRAIL: 6, SMALL3: 11}, "post_gemm": {DMA8: 1},
                           "post_chol": {SMALL8: 12, SMALL3: 7}}),
        ("tall", {"fit": {SMALL8: 20, TALL_TRAIL: 3}, "sweep": {SMALL8: 19, TALL: 4}, "carried": {SMALL8: 19, PERSIST_TRAIL: 2, TALL_TRAIL: 2},
                  "augmented": {SMALL8: 33, PERSIST_TRAIL: 3, TALL_TRAIL: 4}, "post_gemm": {TALL: 1}, "post_chol": {SMALL8: 15, TALL_TRAIL: 1}}),
        ("tall_nb1024", {"fit": {SMALL8: 22, TALL_TRAIL: 1}, "sweep": {SMALL8: 21, TALL: 2},
                         "carried": {SMALL8: 20, TALL: 1, PERSIST_TRAIL: 1, TALL_TRAIL: 1},
                         "augmented": {SMALL8: 36, TALL: 1, PERSIST_TRAIL: 1, TALL_TRAIL: 2}, "post_gemm": {TALL: 1}, "post_chol": {SMALL8: 16}}),
        ("ticket2_nb2048", {"fit": {SMALL8: 22, DMA8: 1}, "sweep": {SMALL8: 21, DMA8: 2},
                            "carried": {SMALL8: 20, DMA8: 1, TICKET: 1, DMA8_TRAIL: 1},
                            "augmented": {SMALL8: 36, DMA8: 2, TICKET: 1, TICKET_TRAIL: 1}, "post_gemm": {DMA8: 1}, "post_chol": {SMALL8: 16}}),
        ("nb3072 persist0_nb3072", {"fit": {SMALL8: 22, DMA8: 1}, "sweep": {SMALL8: 22, DMA8: 1}, "carried": {SMALL8: 20, DMA8: 3},
                                    "augmented": {SMALL8: 36, DMA8: 3, DMA8_TRAIL: 1}, "post_gemm": {DMA8: 1}, "post_chol": {SMALL8: 16}}),
    ],
}
# the launches of at least 128 tiles at SMALL and MID: (site, shape) per route; each is a trailing update of a Cholesky
# (role 1, alone on the chip) on chol_trailing_update_dma_kernel
AUG512 = [("augmented", "1920x1792xK512-lower+0")]
LARGE_BELOW_BIG = {
    ("SMALL", 700): {"nb128": [("augmented", "1536x1408xK128-lower+0")]},
    ("MID", 700): {
        **{route: AUG512 for route in (STEADY + " panel_fused0 small_tiles0 small_dma0").split()},
        "nb128": [("fit", "1536x1408xK128-lower+0")] + [("carried", "%dx%dxK128-lower+0" % (2304 - k, 1408 - k)) for k in (0, 128, 256)] +
                 [("augmented", "%dx%dxK128-lower+0" % (2304 - k, 2176 - k)) for k in range(0, 896, 128)],
        "nb256": [("carried", "2176x1280xK256-lower+0")] + [("augmented", "%dx%dxK256-lower+0" % (2176 - k, 2048 - k)) for k in (0, 256, 512)],
    },
}


def recorded(name, n):
    out = {}
    for routes, rec in RECORD[name, n]:
        for route in routes.split():
            assert route not in out
            out[route] = rec
    return out


@pytest.mark.parametrize("name,n", list(RECORD))
def test_every_launch_reaches_the_recorded_kernel(route_check, name, n):
    want = recorded(name, n)
    assert sorted(want) == sorted(routes_of(name)) and n in G.TEST_SETS[name]
    for route in routes_of(name):
        answers = kernels(route_check, name, n, route)
        assert summary(answers) == want[route], (name, n, route, summary(answers))
        # the family is entered by the tile count alone at these shapes
        for site, case, role, kernel in answers:
            assert (kernel in FAMILY) == (tiles(case) >= 128), (name, n, route, site, str(case), kernel)
            assert kernel.startswith("chol_trailing_update") == (role == 1 and kernel in FAMILY)
        if name != "BIG":
            big = [(site, str(case)) for site, case, _, kernel in answers if kernel in FAMILY]
            assert big == LARGE_BELOW_BIG.get((name, n), {}).get(route, []), (name, n, route, big)
            assert {kernel for _, _, _, kernel in answers if kernel in FAMILY} <= {DMA8_TRAIL}


def test_the_launch_shapes_are_the_ones_claimed():
    shapes = lambda todo: [str(c) for _, c, _, _ in todo]      # noqa: E731
    # BIG, n = 1000: the rectangular sweep's first update, the carried rows, the augmented columns
    assert shapes(sweep_launches(3072, 1024, {}))[3] == "1024x2560xK512" and tiles(C(1024, 2560, 512)) == 160
    carried = site_launches("carried", 2950, 1000, {})
    assert shapes(carried)[3] == "3712x2560xK512-lower+0" and 3712 + 512 == 3072 + 128 + 1024       # 4224 rows
    assert shapes(site_launches("augmented", 2950, 1000, {}))[3] == "3712x3584xK512-lower+0"
    # n = 2100: m >= 2048 puts the lookahead sweep beside_update; the posterior GEMM
    assert {sh for _, _, sh, _ in sweep_launches(3072, 2176, G.ROUTES["la256_deep"])} == {BESIDE}
    assert {sh for _, _, sh, _ in sweep_launches(3072, 1024, G.ROUTES["la256_deep"])} == {CHIP_SHARED}
    assert {sh for _, _, sh, _ in sweep_launches(3072, 2176, {})} == {ALONE}
    assert shapes(site_launches("post_gemm", 2950, 2100, {})) == ["2176x2176xK3072-lower+0"]
    # SMALL, n = 300: 1152 augmented columns, the block 512..1024 straddles the boundary at 768; MID: 2304 end in a half block
    aug = [(c.M, c.N, c.K) for _, c, _, role in site_launches("augmented", 641, 300, {}) if role == 1]
    assert aug == [(768, 640, 512), (256, 128, 512)]
    assert [(c.M, c.N, c.K) for _, c, _, role in site_launches("augmented", 1500, 700, {}) if role == 1][-1] == (384, 256, 512)
    # under lookahead every trailing update but the last is two launches: (a) role 0, (b) role 1, both beside_update
    la = [(str(c), sh, role) for _, c, sh, role in site_launches("carried", 1500, 700, G.ROUTES["la256_deep"]) if c.K == 512 and c.diag_off == 0 and c.N >= 512]
    assert la == [("1920x512xK512-lower+0", BESIDE, 0), ("1408x512xK512-lower+0", BESIDE, 1), ("1408x512xK512-lower+0", BESIDE, 0)]
    # the panels beside it: chip_shared_only below shallow_min columns (la256_shallow), beside_update from there (la256_deep)
    inner = lambda route: {sh for _, c, sh, role in site_launches("carried", 1500, 700, G.ROUTES[route]) if c.K < 512}      # noqa: E731
    assert inner("la256_deep") == {BESIDE} and inner("la256_shallow") == {CHIP_SHARED} and inner("default") == {ALONE}
    # first-generation leaves: 64-column updates on the odd offset inside panel_rec
    assert {(c.N, c.diag_off) for _, c, _, _ in site_launches("fit", 641, 37, G.ROUTES["panel_fused0"]) if c.K == 64} == {(64, -64)}
    # a posterior factor of one tile launches no GEMM
    assert site_launches("post_chol", 641, 37, {}) == []


@pytest.mark.parametrize("name,n", [k for k in RECORD if k[0] != "BIG"])
def test_the_lds_dma_options_cannot_reach_small_and_mid(route_check, name, n):
    """fewer than 128 tiles of 128 x 128 in every launch but those of LARGE_BELOW_BIG: the same kernel under every value of
    gemm_tall, gemm_persist and gemm_ticket -- those options get no route at these shapes.  The exceptions are trailing
    updates of a Cholesky (BIG's routes run that site under the options)"""
    for route in G.ROUTES:
        base = kernels(route_check, name, n, route)
        small = [i for i, (_, case, _, _) in enumerate(base) if tiles(case) < 128]
        assert len(base) - len(small) == len(LARGE_BELOW_BIG.get((name, n), {}).get(route, []))
        for more in LDS_DMA_OPTIONS:
            got = kernels(route_check, name, n, route, **more)
            assert [got[i] for i in small] == [base[i] for i in small], (name, n, route, more)
        assert {site for _, (site, case, _, _) in enumerate(base) if tiles(case) >= 128} <= {"fit", "carried", "augmented"}


def test_big_reaches_the_lds_dma_family_at_every_site(route_check):
    """the condition tests/test_predict_routes_gpu.py rests on: the rectangular sweep, the carried update, the augmented
    update and the posterior GEMM each run on a kernel of the 128-tile family under at least one BIG route, and each of
    tall, ticket2 and persist changes at least one kernel of the prediction side against the same route without it"""
    got = {(n, route): kernels(route_check, "BIG", n, route, sites=PREDICTION_SITES) for n in G.TEST_SETS["BIG"] for route in G.BIG_ROUTES}
    reached = {site: {k for ans in got.values() for s, _, _, k in ans if s == site and k in FAMILY} for site in PREDICTION_SITES}
    for site in PREDICTION_SITES:
        print("%s: %s" % (site, sorted(reached[site])))
    assert reached["sweep"] == {DMA8, TALL}
    assert reached["carried"] == {DMA8, TALL, TICKET, DMA8_TRAIL, TALL_TRAIL, PERSIST_TRAIL}
    assert reached["augmented"] == {DMA8, TALL, TICKET, DMA8_TRAIL, TALL_TRAIL, PERSIST_TRAIL, TICKET_TRAIL}
    assert reached["post_gemm"] == {DMA8, TALL}
    assert reached["post_chol"] == {DMA8_TRAIL, TALL_TRAIL}
    # the posterior GEMM needs n = 2100; at n = 1000 it has 64 tiles
    assert not {k for (n, _), ans in got.items() if n == 1000 for s, _, _, k in ans if s == "post_gemm"} & set(FAMILY)
    # m >= 2048: the lookahead sweep runs beside_update, every small launch of it on the 3-stage ring
    for route in ("la256_deep", "la256_shallow"):
        assert SMALL3 in {k for s, _, _, k in got[2100, route] if s == "sweep"}
        assert SMALL3 not in {k for s, _, _, k in got[1000, route] if s == "sweep"}

    def changed(n, route, **more):
        """(site, shape, without, with): the kernels the route's option changes against the same route with `more`"""
        a, b = got[n, route], kernels(route_check, "BIG", n, route, sites=PREDICTION_SITES, **more)
        assert [(s, c, r) for s, c, r, _ in a] == [(s, c, r) for s, c, r, _ in b]
        return [(s, str(c), kb, ka) for (s, c, _, ka), (_, _, _, kb) in zip(a, b) if ka != kb]

    for n in G.TEST_SETS["BIG"]:
        tall = changed(n, "tall", gemm_tall=0)
        assert {ka for _, _, _, ka in tall} == {TALL, TALL_TRAIL} and {s for s, _, _, _ in tall} >= {"sweep", "carried", "augmented"}
        # gemm_persist = 1 is the default: the first carried and augmented updates are the launches with two rounds of blocks
        persist = changed(n, "default", gemm_persist=0)
        assert persist and {(kb, ka) for _, _, kb, ka in persist} == {(DMA8_TRAIL, PERSIST_TRAIL)}
        assert {s for s, _, _, _ in persist} == {"carried", "augmented"}
        # one block of 3072 leaves no launch of this side with two rounds: persist0_nb3072 is nb3072 here
        assert changed(n, "persist0_nb3072", gemm_persist=1) == []
    assert changed(1000, "ticket2_nb2048", gemm_ticket=0) == []          # no launch with a round of 256 blocks at n = 1000
    assert changed(2100, "ticket2_nb2048", gemm_ticket=0) == [
        ("carried", "4352x1024xK1024-lower+0", DMA8, TICKET), ("augmented", "4352x1024xK1024-lower+0", DMA8, TICKET),
        ("augmented", "3328x3200xK2048-lower+0", DMA8_TRAIL, TICKET_TRAIL)]


def test_which_launches_of_the_fit_move_when_the_test_rows_ride(route_check):
    """one_pass carries np_ more rows through every panel and update launch of the fit: the launches are the same in
    number, K and columns, and some of them cross the 128-tile line (or the two rounds the persistent form asks for) and
    run on another kernel.  Every kernel of the update GEMM adds the K steps of a tile in the same order
    (tests/test_gemm_routes_gpu.py holds each route to the same exact reference), so the GPU module asserts lml, m, diag
    and alpha of one_pass equal to two_call's bit for bit on every route; this test names the launches that statement
    covers with two different kernels"""
    moved = {}
    for name in G.PROBLEMS:
        for n in G.TEST_SETS[name]:
            for route in routes_of(name):
                fit = kernels(route_check, name, n, route, sites=("fit",))
                carried = kernels(route_check, name, n, route, sites=("carried",))
                assert [(c.N, c.K, c.diag_off, r) for _, c, r, _ in fit] == [(c.N, c.K, c.diag_off, r) for _, c, r, _ in carried]
                assert {b.M - a.M for (_, a, _, _), (_, b, _, _) in zip(fit, carried)} == {np_of(n)}
                pairs = sorted({(ka, kb) for (_, _, _, ka), (_, _, _, kb) in zip(fit, carried) if ka != kb})
                if pairs:
                    moved[name, n, route] = pairs
    assert not [k for k in moved if k[0] == "SMALL"]
    assert {k[2]: v for k, v in moved.items() if k[0] == "MID"} == {"nb128": [(SMALL8, DMA8_TRAIL)], "nb256": [(SMALL8, DMA8_TRAIL)]}
    assert set(moved["BIG", 1000, "default"]) == {(DMA8_TRAIL, PERSIST_TRAIL), (SMALL8, DMA8_TRAIL)}
    assert set(moved["BIG", 2100, "la256_deep"]) == {(SMALL3, DMA8), (SMALL3, DMA8_TRAIL)}
    assert set(moved["BIG", 2100, "ticket2_nb2048"]) == {(SMALL8, DMA8), (SMALL8, DMA8_TRAIL), (DMA8, TICKET)}
    assert {k[2] for k in moved if k[0] == "BIG"} == set(G.BIG_ROUTES)


# ------------------------------------------------------------------------------------------------------------ the bars
OLD = ("lml", "alpha", "m", "diag", "mu")


def float64_evaluations(name, n, other_k=False):
    """-> the LAPACK and the blocked float64 evaluation of (problem, test set)"""
    X, y, r = G.problem_inputs(name)
    Xs, Z = G.points_at(name, n), G.normals(n)
    return (P.predict(G.reference_fit(name, np.float64), Xs, G.JITTERS, Z),
            P.blocked(X, y, r, Xs, G.SIGMA, G.ELL, G.SIZES[name][2], G.JITTERS, Z, other_k=other_k))


def show(tag, err):
    print("%s  " % tag + "  ".join("%s %.2e" % kv for kv in err.items()))


def test_the_test_sets_are_the_ones_claimed():
    """a third of the points leave the training box: variances from 3e-5 to 0.14 and means up to 20 at MID"""
    Xs = G.points_at("MID", 700)
    assert Xs.shape == (700, 8) and Xs[2::3].min() >= 3.0 and Xs[2::3].max() > 4.9 and np.delete(Xs, np.s_[2::3], 0).max() < 4.0
    ref = P.predict(G.reference_fit("MID", np.float64), Xs, G.JITTERS, G.normals(700))
    assert 2e-5 < ref["var"].min() < 5e-5 and 0.1 < ref["var"].max() < 0.2 and 15 < np.abs(ref["mu"]).max() < 25
    cond = [np.linalg.cond(ref["post"][j]["Sigma"]) for j in G.JITTERS]
    print("MID n=700: cond Sigma %.1e at jitter 1e-6, %.1e at 1e-2" % tuple(cond))
    assert 1e6 < cond[0] < 1e7 and cond[1] < 1e3
    assert G.normals(700).shape == (700, 17) and [G.TEST_SETS[k] for k in G.PROBLEMS] == [(37, 300, 700), (700,), (1000, 2100)]


@pytest.mark.parametrize("name,n", list(G.FLOAT64_MISS))
def test_float64_misses_of_the_long_double_evaluation(name, n):
    """SMALL and MID: what the two float64 evaluations miss of the long-double one, per quantity -- the worse of the two
    is FLOAT64_MISS, held here within a factor 2, and ten times it is the bar of the variance, Sigma, L_ and L_ @ Z in
    the GPU module (every one of them below the plain bar it replaces).  The quantities that keep their plain bar leave
    float64 the same factor 10"""
    ref = G.reference(name, n)
    lapack, blocked = float64_evaluations(name, n)
    ea, eb = P.errors(lapack, ref), P.errors(blocked, ref)
    show("%s n=%d LAPACK " % (name, n), ea)
    show("%s n=%d blocked" % (name, n), eb)
    assert np.finfo(G.LD).eps < 1e-18 and ref["mu"].dtype == G.LD            # long double is wider than float64 here
    table, bars = G.FLOAT64_MISS[name, n], G.bars(name, n)
    assert sorted(table) == sorted(ea) == sorted(eb) == sorted(bars)
    for k, recorded in table.items():
        worse = max(ea[k], eb[k])
        assert recorded / 2 <= worse <= 2 * recorded, (name, n, k, worse, recorded)
    for k in OLD:
        assert bars[k] == G.PLAIN[k] and 10 * table[k] <= bars[k], k
    for k in G.NEW:
        assert bars[k] == 10 * table[k] < G.PLAIN[k] / 10, k


@pytest.mark.parametrize("name,n", list(G.FLOAT64_APART))
def test_two_float64_evaluations_of_big_agree(name, n):
    """BIG in long double takes minutes, so there the reference is the LAPACK float64 evaluation and the bar of the new
    quantities 10 x the distance of the blocked evaluation from it (FLOAT64_APART, held within a factor 2).  cond K_y is
    2e4 there: the two agree to a few ulp in everything but the factor of Sigma at jitter 1e-6 (cond Sigma 4e7).

    The blocked evaluation rounds every operation otherwise, the covariance included (predict_ref.kernel_other_rounding:
    elements 2e-15 apart in relative terms at the most).  From the same bits of K the two are closer -- L_ 6e-12 against
    4e-11, L_ at jitter 1e-2 1e-14 against 5e-14, Sigma 2e-15 against 5e-15 -- because they share the rounding of K, and
    that is the larger part of what float64 misses: in long double (n = 1000, once, 2.5 minutes) either evaluation
    misses L_ by 5e-11 and 6e-14 and Sigma by 6e-15.  The distance with the covariance rounded otherwise is within
    1.6 x of that miss, the distance from the same bits of K a fifth to an eighth of it"""
    lapack, blocked = float64_evaluations(name, n, other_k=True)
    assert lapack is not G.reference(name, n) and lapack["mu"].dtype == np.float64 == G.reference(name, n)["mu"].dtype
    apart = P.errors(blocked, G.reference(name, n))
    show("%s n=%d blocked - LAPACK" % (name, n), apart)
    same_k = P.errors(float64_evaluations(name, n)[1], G.reference(name, n))
    show("%s n=%d blocked - LAPACK, the same bits of K" % (name, n), same_k)
    assert all(same_k[k] < apart[k] for k in ("L_@1e-06", "L_@0.01", "Sigma@1e-06", "Sigma@0.01"))
    z = G.reference_fit(name, np.float64)["z"][:400]
    Ka, Kb = P.kernel(z, z, G.SIGMA, G.ELL, np.float64), P.kernel_other_rounding(z, z, G.SIGMA, G.ELL)
    assert 0 < np.max(np.abs(Ka - Kb) / Ka) < 4e-15
    table, bars = G.FLOAT64_APART[name, n], G.bars(name, n)
    assert sorted(table) == sorted(apart) == sorted(bars)
    for k, recorded in table.items():
        assert recorded / 2 <= apart[k] <= 2 * recorded, (name, n, k, apart[k], recorded)
    for k in OLD:
        assert bars[k] == G.PLAIN[k] and 10 * table[k] <= bars[k], k
    for k in G.NEW:
        assert bars[k] == 10 * table[k] < G.PLAIN[k] / 10, k


# ------------------------------------------------------------------------------------- what the bars would not let pass
def test_full_has_no_padding_and_every_other_problem_has(route_check):
    """the last K step (16 columns) of every sum over the training points is padding at SMALL, MID and BIG; FULL is there
    so that it is not.  Its launches have fewer than 128 tiles on every route"""
    assert all(np_of(N) - N >= 16 for N, _, _ in G.PROBLEMS.values())
    N, n = G.SIZES["FULL"][0], G.TEST_SETS["FULL"][0]
    assert N == np_of(N) == 768 and n == np_of(n) == 256 and "FULL" in G.LONG_DOUBLE
    for route in G.ROUTES:
        answers = kernels(route_check, "FULL", n, route)
        assert answers and max(tiles(case) for _, case, _, _ in answers) < 128
        assert {k for _, _, _, k in answers} <= {SMALL8, SMALL3, REG128, REG64}, route


@pytest.mark.parametrize("name,n", [("SMALL", 700), ("FULL", 256), ("BIG", 1000)])
def test_the_bars_see_the_eighth_digit_of_the_factor_and_a_lost_k_step(name, n):
    """two ways to break the library that the suite let pass before: one entry of the posterior factor off by 1e-8 (the old
    bars: 1e-6 and 1e-7), and the last K step of the posterior GEMM lost.  Done here to a float64 evaluation that keeps
    every bar: the first breaks the bar of L_ at both jitters in every problem; the second takes 4e-3 out of Sigma at
    FULL -- and nothing at SMALL and BIG, whose last 16 columns of v are padding, which is why FULL exists"""
    ref, bars = G.reference(name, n), G.bars(name, n)
    good = float64_evaluations(name, n, other_k=name not in G.LONG_DOUBLE)[1 if name not in G.LONG_DOUBLE else 0]
    err = P.errors(good, ref)
    assert all(err[k] <= bars[k] for k in bars)
    # one entry of the factor, 1e-8
    bad = dict(good, post={j: dict(p, L_=p["L_"].copy()) for j, p in good["post"].items()})
    for p in bad["post"].values():
        p["L_"][n // 2, n // 3] += 1e-8
    err = P.errors(bad, ref)
    assert all(err["L_@%g" % j] > 10 * bars["L_@%g" % j] for j in G.JITTERS), err
    # the last K step of v^T v, as the padded device layout has it: columns Np - 16 .. Np of v^T, zero from N on
    f = G.reference_fit(name, np.float64)
    N, Np = len(f["z"]), np_of(len(f["z"]))
    v = np.zeros((Np, n))
    v[:N] = solve_triangular(f["L"], P.kernel(f["z"], R.scaled(G.points_at(name, n), f["r"]), G.SIGMA, G.ELL, np.float64), lower=True)
    lost = v[Np - 16:].T @ v[Np - 16:]
    if name != "FULL":
        assert not lost.any()
        return
    bad = dict(good, post={})
    for j, p in good["post"].items():
        L_ = np.linalg.cholesky(np.asarray(p["Sigma"], dtype=np.float64) + lost)
        bad["post"][j] = dict(L_=L_, LZ=L_ @ G.normals(n))
    err = P.errors(bad, ref)
    print("FULL, the last K step lost: Sigma %.2e off (bar %.2e), L_ %.2e (bar %.2e)" % (
        err["Sigma@0.01"], bars["Sigma@0.01"], err["L_@0.01"], bars["L_@0.01"]))
    for j in G.JITTERS:
        assert err["Sigma@%g" % j] > 1e3 * bars["Sigma@%g" % j] and err["L_@%g" % j] > 1e3 * bars["L_@%g" % j]
