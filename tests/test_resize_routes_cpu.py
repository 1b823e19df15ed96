"""What tests/test_resize_routes_gpu.py rests on, without a GPU:

* the GEMM launches of one gpmi_append, written out from csrc/append.hip and csrc/driver.hip (resize_launches): the
  updates inside trsm_block with m = border and the sweep's own with block size and lookahead from N0, the sharing state
  by the 2048-row rule; the one gemm_minus_lower of (border + 128) x border x N0; the updates inside panel_rec with rows
  border + 128 - r0 and the trailing updates with block size and lookahead from border, split into the next block column
  (role 0) and the rest (role 1) under lookahead, each with its Sharing, shallow_min included;
* the kernel gemm_route (csrc/gpmi_route.h, through tests/sanitize/gemm_route_check.cpp) answers for every one of them
  under every route, held against the names recorded below (RECORD), and each claim of the GPU module's docstring: WIDE
  reaches no LDS-DMA kernel under any value of gemm_tall, gemm_ticket and gemm_persist; WIDER's rank-N0 update reaches
  gemm_nt_dma_kernel<2, false> and gemm_nt_dma_tall_kernel<false>, its sweep gemm_nt_small_kernel<3> under la256_*; the
  TICKET and PERSIST sizes are the smallest that reach their kernels and one tile row less does not.  The sizes worked
  out by hand from live tiles (borders of 2816 and 3968) were too large: the resident forms count the blocks of whole
  supertiles, and gemm_route answers 2560 and 3584;
* append_plan and remove_plan (the headers, compiled with g++ -fsanitize=address,undefined like
  tests/sanitize/append_plan_check.cpp) for every case: N0, border, skinny, in_place, yrow_moves; the sweeps and J0 of
  the removals; and the same from the Python restatement the stand-in below uses;
* the float64 mirror of the largest problem (PERSIST, 4097 points): ard_ref.lml_and_grad with the LOO closed forms of
  loo_ref.from_Ky on its explicit inverse, against a second float64 evaluation from the Cholesky factor by triangular
  solves -- every quantity a tenth of the bar the device is held to apart at the most (FLOAT64_APART has the figures);
* the GPU module's own helpers and test functions on a stand-in for the device: MirrorContext implements fit, append and
  remove as a NumPy fit of the resulting data, with the layout bookkeeping of gpmi_append_plan.h and driver.hip, so that
  the module's bookkeeping (orders, keys of the caches, layouts, options put back) is checked before the first GPU run."""
import os
import shutil
import subprocess

import numpy as np
import pytest
from scipy.linalg import cho_solve, lapack, solve_triangular

import ard_ref
import gemm_route_table as T
import loo_ref
import test_remove_gpu as TR
import test_resize_routes_gpu as G
from conftest import ROOT
from test_gemm_route_cpu import MI355X_GROUPS, query, route_check       # noqa: F401 (route_check is a fixture)

C = T.Case
DEFAULTS = {k: G.DEFAULTS[k] for k in ("nb", "lookahead", "la_min", "shallow_min", "panel_fused")}
assert DEFAULTS == dict(nb=0, lookahead=1, la_min=6144, shallow_min=6144, panel_fused=1)
GEMM_OPTIONS = ("gemm_small_tiles", "gemm_small_dma", "gemm_tall", "tall_min_tiles", "gemm_ticket", "gemm_persist")
SMALL8, SMALL3 = "gemm_nt_small_kernel<8>", "gemm_nt_small_kernel<3>"
REG128, REG64 = "gemm_nt_kernel<4, 4, false>", "gemm_nt_kernel<2, 2, false>"
DMA8, TALL = "gemm_nt_dma_kernel<2, false>", "gemm_nt_dma_tall_kernel<false>"
TICKET, PERSIST = "gemm_nt_dma_ticket_kernel", "gemm_nt_dma_persist_kernel"
ALONE, CHIP_SHARED, BESIDE_UPDATE = (0, 0), (0, 1), (1, 1)      # Sharing: (small_lds, chip_shared)


def block(o, ncols):
    """gpmi_ctx::block"""
    return o["nb"] or (2048 if ncols >= 32768 else 1024 if ncols >= 12288 else 512)


def lookahead_for(o, ncols):
    """gpmi_ctx::lookahead_for (every context has its panel stream)"""
    return bool(o["lookahead"]) and ncols > block(o, ncols) and ncols >= o["la_min"]


def leaf_of(o, w, off, m=0):
    return 128 if o["panel_fused"] and w % 128 == 0 and off % 128 == 0 and m % 128 == 0 else 64


def trsm_updates(o, m, off, w):
    """trsm_rec (driver.hip): the updates inside the triangular solve of one block of w columns, m rows"""
    leaf = leaf_of(o, w, off, m)
    if w <= leaf:
        return []
    h = (w // 2) // leaf * leaf
    return trsm_updates(o, m, off, h) + [C(m, w - h, h)] + trsm_updates(o, m, off + h, w - h)


def panel_updates(o, mrows, off, w):
    """panel_rec (driver.hip): the lower updates inside the factorisation of one block column of w columns, mrows rows
    from its diagonal block on; rows start at the 128-aligned row at or above off + h"""
    leaf = leaf_of(o, w, off)
    if w <= leaf:
        return []
    h = (w // 2) // leaf * leaf
    c0 = off + h
    r0 = c0 // 128 * 128
    return (panel_updates(o, mrows, off, h) + [C(mrows - r0, w - h, h, lower=1, diag_off=r0 - c0)] +
            panel_updates(o, mrows, off + h, w - h))


def resize_launches(N, k, opts, append_skinny=-1):
    """-> [(site, Case, (small_lds, chip_shared), role)]: the GEMM launches of one padded gpmi_append of k points behind a
    fit of N, in launch order, as csrc/append.hip strings them together from csrc/driver.hip:
      trsm, sweep   solve_sweep_factor(A, N0, V = rows [N0, Np1) of A, m = border): block size and lookahead from N0;
                    alone without lookahead, and_chip_shared below 2048 rows, beside_update from there
      rank          the one gemm_minus_lower, (border + 128) x border x N0, diag_off 0, under the caller's sharing (alone)
      panel, trail  cholesky_inplace(A + N0 (ld + 1), ncols = border, nrows = border + 128): block size and lookahead from
                    border; without lookahead the panels under large_lds and one trailing update (role 1) per step; with
                    it the panels under beside_update while at least shallow_min columns are left and chip_shared_only
                    after, the next block column (role 0) and the rest (role 1) under beside_update
    A skinny append (k <= 16 on a fused factor of at least 128 points, option append_skinny not 0) has no sweep launches:
    its W comes from the <= 16-row border-sweep kernel."""
    o = dict(DEFAULTS, **{n: v for n, v in opts.items() if n in DEFAULTS})
    N0 = N // 128 * 128
    Np1 = (N + k + 127) // 128 * 128
    border = Np1 - N0
    skinny = k <= 16 and o["panel_fused"] and N0 > 0 and append_skinny != 0
    out = []
    if N0 > 0 and not skinny:
        NB, la = block(o, N0), lookahead_for(o, N0)
        sharing = ALONE if not la else BESIDE_UPDATE if border >= 2048 else CHIP_SHARED
        for c in range(0, N0, NB):
            nb = min(NB, N0 - c)
            out += [("trsm", case, sharing, 0) for case in trsm_updates(o, border, 0, nb)]
            r0 = c + nb
            if r0 >= N0:
                continue
            if not la:
                out.append(("sweep", C(border, N0 - r0, nb), sharing, 0))
                continue
            nbn = min(NB, N0 - r0)
            out.append(("sweep", C(border, nbn, nb), sharing, 0))
            if r0 + nbn < N0:
                out.append(("sweep", C(border, N0 - r0 - nbn, nb), sharing, 0))
    if N0 > 0:
        out.append(("rank", C(border + 128, border, N0, lower=1, diag_off=0), ALONE, 0))
    ncols, nrows = border, border + 128
    NB, la = block(o, ncols), lookahead_for(o, ncols)
    for c in range(0, ncols, NB):
        nb = min(NB, ncols - c)
        forms = ALONE if not la else BESIDE_UPDATE if ncols - c >= o["shallow_min"] else CHIP_SHARED
        out += [("panel", case, forms, 0) for case in panel_updates(o, nrows - c, 0, nb)]
        r0 = c + nb
        if r0 >= ncols:
            continue
        if not la:
            out.append(("trail", C(nrows - r0, ncols - r0, nb, lower=1, diag_off=0), ALONE, 1))
            continue
        nbn = min(NB, ncols - r0)
        out.append(("trail", C(nrows - r0, nbn, nb, lower=1, diag_off=0), BESIDE_UPDATE, 0))
        if r0 + nbn < ncols:
            out.append(("trail", C(nrows - r0 - nbn, ncols - r0 - nbn, nb, lower=1, diag_off=0), BESIDE_UPDATE, 1))
    return out


def tiles(case):
    return (case.M // 128) * ((case.N + 127) // 128)


def ask(case, sharing, role, **gemm_opts):
    """query of tests/test_gemm_route_cpu.py, with the launch's role in its fourth word"""
    words = query(MI355X_GROUPS, "small_dma8", case, sharing=sharing, **gemm_opts).split()
    words[3] = str(role)
    return " ".join(words)


def kernels(route_check, N, k, opts, append_skinny=-1, **more):
    """-> [(site, Case, sharing, role, kernel)] of every launch of the append under a route; more: options on top"""
    todo = resize_launches(N, k, opts, append_skinny)
    gemm_opts = dict({n: v for n, v in opts.items() if n in GEMM_OPTIONS}, **more)
    got = route_check([ask(case, sharing, role, **gemm_opts) for _, case, sharing, role in todo])
    return [t + (g,) for t, g in zip(todo, got)]


def case_kernels(route_check, name, route, **more):
    N, k, skinny = G.APPENDS[name]
    return kernels(route_check, N, k, G.APPEND_ROUTES[name][route], skinny, **more)


def summary(answers):
    """-> {site: {kernel: launches}}"""
    out = {}
    for site, _, _, _, kernel in answers:
        out.setdefault(site, {}).setdefault(kernel, 0)
        out[site][kernel] += 1
    return out


def large(answers):
    return [(site, str(case), kernel) for site, case, _, _, kernel in answers if tiles(case) >= 128]


def test_the_launch_shapes_are_the_ones_claimed():
    shapes = lambda N, k, opts, site, **kw: [str(c) for s, c, _, _ in resize_launches(N, k, opts, **kw) if s == site]   # noqa: E731
    # WIDE at the default blocks: the sweep over 512 + 128 columns with m = 1024, one rank-640 update with the y block as
    # its ninth row tile, two panels of 512 and one trailing update between them
    assert shapes(700, 900, {}, "trsm") == ["1024x128xK128", "1024x256xK256", "1024x128xK128"]
    assert shapes(700, 900, {}, "sweep") == ["1024x128xK512"]
    assert shapes(700, 900, {}, "rank") == ["1152x1024xK640-lower+0"]
    assert shapes(700, 900, {}, "trail") == ["640x512xK512-lower+0"]
    assert shapes(700, 900, {}, "panel") == ["1024x128xK128-lower+0", "896x256xK256-lower+0", "768x128xK128-lower+0",
                                             "512x128xK128-lower+0", "384x256xK256-lower+0", "256x128xK128-lower+0"]
    # first-generation leaves: 64 columns, the panel's updates start 64 rows above their diagonal
    gen1 = resize_launches(700, 900, G.ROUTES["panel_fused0"])
    assert min(c.N for s, c, _, _ in gen1 if s == "trsm") == 64 and {c.diag_off for s, c, _, _ in gen1 if s == "panel"} == {0, -64}
    # lookahead is decided from N0 for the sweep and from border for the Cholesky, each against its own block size: under
    # la256_* WIDE's sweep (640 > 512 columns) and Cholesky (1024 > 512) both run it; with blocks of 128 and la_min 256 too
    la = G.ROUTES["la256_deep"]
    assert shapes(700, 900, la, "sweep") == ["1024x128xK512"] and shapes(700, 900, la, "trail") == ["640x512xK512-lower+0"]
    assert shapes(700, 2000, la, "trail")[:2] == ["1792x512xK512-lower+0", "1280x1152xK512-lower+0"]
    assert [r for s, _, _, r in resize_launches(700, 2000, la) if s == "trail"] == [0, 1, 0, 1, 0, 1, 0]
    assert [r for s, _, _, r in resize_launches(700, 2000, {}) if s == "trail"] == [1, 1, 1, 1]
    # the sharing state of the sweep follows m = border at 2048 rows; the panels' follows shallow_min
    sharing = lambda N, k, opts, site: {sh for s, _, sh, _ in resize_launches(N, k, opts) if s == site}   # noqa: E731
    assert sharing(700, 900, la, "trsm") == sharing(700, 900, la, "sweep") == {CHIP_SHARED}
    assert sharing(700, 2000, la, "trsm") == sharing(700, 2000, la, "sweep") == {BESIDE_UPDATE}
    assert sharing(700, 2000, {}, "trsm") == sharing(700, 2000, {}, "panel") == sharing(700, 2000, {}, "trail") == {ALONE}
    assert sharing(700, 2000, la, "panel") == {BESIDE_UPDATE} and sharing(700, 2000, G.ROUTES["la256_shallow"], "panel") == {CHIP_SHARED}
    assert sharing(700, 2000, la, "rank") == {ALONE}
    # a sweep that decided its lookahead from c->Np would run it where N0 says no (and the reverse): N0 = 640 against
    # Np1 = 1664 under la_min = 1024
    o = dict(DEFAULTS, la_min=1024)
    assert not lookahead_for(o, 640) and lookahead_for(o, 1664) and lookahead_for(o, 1024)
    # the skinny append: no sweep launch, a rank-1408 update of the one border tile and the y block, one panel
    assert [(s, str(c)) for s, c, _, _ in resize_launches(1500, 16, G.ROUTES["nb256"], 1)] == [("rank", "256x128xK1408-lower+0")]
    assert [s for s, _, _, _ in resize_launches(1500, 16, G.ROUTES["panel_fused0"], 1)][:3] == ["trsm"] * 3      # refused there
    # the padded append behind a removal: N' = 1084 and 900 survivors plus 300
    assert shapes(1084, 300, {}, "rank") == ["512x384xK1024-lower+0"] and shapes(900, 300, {}, "rank") == ["512x384xK896-lower+0"]


# ---------------------------------------------------------------------------------------------------- recorded kernels
def one(kernel, trsm, sweep, rank, panel, trail):
    """every launch on the same kernel: the launches per site"""
    return {site: {kernel: n} for site, n in zip(("trsm", "sweep", "rank", "panel", "trail"), (trsm, sweep, rank, panel, trail)) if n}


# {problem: {route: {site: {kernel: launches}}}}: what gemm_route answered when these tests were written
TRAIL, TRAIL_TALL = "chol_trailing_update_dma_kernel", "chol_trailing_update_dma256_kernel"      # role 1: the Cholesky's own symbols
LDS_DMA_FAMILY = (DMA8, TALL, TICKET, PERSIST, TRAIL, TRAIL_TALL)


def wider(rank, trsm=(SMALL8, 3), sweep=(SMALL8, 1), panel=(SMALL8, 12), trail=((TRAIL, 1), (SMALL8, 3))):
    return {"trsm": dict([trsm]), "sweep": dict([sweep]), "rank": {rank: 1}, "panel": dict([panel]), "trail": dict(trail)}


RECORD = {
    "WIDE": {
        "default": one(SMALL8, 3, 1, 1, 6, 1), "nb128": one(SMALL8, 0, 4, 1, 0, 7), "nb256": one(SMALL8, 2, 2, 1, 4, 3),
        "lookahead0": one(SMALL8, 3, 1, 1, 6, 1),
        # and_chip_shared keeps the deep ring in the sweep (m = 1024 < 2048); the Cholesky runs beside_update
        "la256_deep": dict(one(SMALL8, 3, 1, 1, 0, 0), panel={SMALL3: 6}, trail={SMALL3: 1}),
        "la256_shallow": dict(one(SMALL8, 3, 1, 1, 6, 0), trail={SMALL3: 1}),
        "panel_fused0": one(SMALL8, 8, 1, 1, 14, 1), "trsv_vinv0": one(SMALL8, 3, 1, 1, 6, 1), "trsv_vinv1": one(SMALL8, 3, 1, 1, 6, 1),
        "trsv_vinv2": one(SMALL8, 3, 1, 1, 6, 1), "small_tiles0": one(REG128, 3, 1, 1, 6, 1), "small_dma0": one(REG64, 3, 1, 1, 6, 1),
    },
    "WIDER": {
        "default": wider(DMA8),
        "nb128": {"sweep": {SMALL8: 4}, "rank": {DMA8: 1}, "trail": {TRAIL: 6, SMALL8: 10}},
        "la256_deep": wider(DMA8, (SMALL3, 3), (SMALL3, 1), (SMALL3, 12), ((SMALL3, 7),)),
        "la256_shallow": wider(DMA8, (SMALL3, 3), (SMALL3, 1), (SMALL8, 12), ((SMALL3, 7),)),
        "panel_fused0": wider(DMA8, (SMALL8, 8), panel=(SMALL8, 29)),
        "tall": wider(TALL, trail=((TRAIL_TALL, 1), (SMALL8, 3))),
        "persist0": wider(DMA8),
    },
    "TICKET": {"ticket2": wider(TICKET, panel=(SMALL8, 15), trail=((TRAIL, 2), (SMALL8, 2)))},
    "PERSIST": {"default": wider(PERSIST, panel=(SMALL8, 21), trail=((TRAIL, 4), (SMALL8, 2))),
                "persist0": wider(DMA8, panel=(SMALL8, 21), trail=((TRAIL, 4), (SMALL8, 2)))},
    "SKINNY": {route: {"rank": {SMALL8: 1}} for route in G.APPEND_ROUTES["SKINNY"]},
}
# the launches of at least 128 tiles: the rank-N0 update, and -- not in the sizes worked out by hand -- the first trailing
# updates of the border's Cholesky (role 1: the symbols of the fit's own trailing update), which lookahead splits below
# 128 tiles.  (site, shape, kernel) in launch order
LARGE = {
    "WIDER": {
        "default": [("rank", "2304x2176xK640-lower+0", DMA8), ("trail", "1792x1664xK512-lower+0", TRAIL)],
        "nb128": [("rank", "2304x2176xK640-lower+0", DMA8)] + [("trail", "%dx%dxK128-lower+0" % (2176 - 128 * i, 2048 - 128 * i), TRAIL)
                                                                for i in range(6)],
        "la256_deep": [("rank", "2304x2176xK640-lower+0", DMA8)],
        "la256_shallow": [("rank", "2304x2176xK640-lower+0", DMA8)],
        "panel_fused0": [("rank", "2304x2176xK640-lower+0", DMA8), ("trail", "1792x1664xK512-lower+0", TRAIL)],
        "tall": [("rank", "2304x2176xK640-lower+0", TALL), ("trail", "1792x1664xK512-lower+0", TRAIL_TALL)],
        "persist0": [("rank", "2304x2176xK640-lower+0", DMA8), ("trail", "1792x1664xK512-lower+0", TRAIL)],
    },
    "TICKET": {"ticket2": [("rank", "2688x2560xK640-lower+0", TICKET), ("trail", "2176x2048xK512-lower+0", TRAIL),
                           ("trail", "1664x1536xK512-lower+0", TRAIL)]},
    "PERSIST": {route: [("rank", "3712x3584xK640-lower+0", kern)] + [("trail", "%dx%dxK512-lower+0" % (3200 - 512 * i, 3072 - 512 * i), TRAIL)
                                                                      for i in range(4)]
                for route, kern in (("default", PERSIST), ("persist0", DMA8))},
}


@pytest.mark.parametrize("name", list(G.APPENDS))
def test_every_launch_reaches_the_recorded_kernel(route_check, name):
    assert sorted(RECORD[name]) == sorted(G.APPEND_ROUTES[name])
    for route in G.APPEND_ROUTES[name]:
        answers = case_kernels(route_check, name, route)
        assert summary(answers) == RECORD[name][route], (name, route, summary(answers))
        assert large(answers) == LARGE.get(name, {}).get(route, []), (name, route, large(answers))
        # the LDS-DMA family is entered by the tile count alone
        for site, case, _, _, kernel in answers:
            assert (kernel in LDS_DMA_FAMILY) == (tiles(case) >= 128), (name, route, site, str(case), kernel)


LDS_DMA_OPTIONS = [dict(gemm_tall=1, tall_min_tiles=0), dict(gemm_tall=0), dict(gemm_persist=0), dict(gemm_persist=1),
                   dict(gemm_ticket=1), dict(gemm_ticket=2)]


def test_the_lds_dma_options_cannot_reach_wide(route_check):
    """fewer than 128 tiles in every launch of every route of WIDE (and of SKINNY and the appends behind a removal): the
    same kernel under every value of gemm_tall, gemm_persist and gemm_ticket"""
    for name, N, k, skinny in [("WIDE",) + G.APPENDS["WIDE"], ("SKINNY",) + G.APPENDS["SKINNY"], ("EDGES + 300", 1084, 300, 0),
                               ("THIRDS + 300", 900, 300, 0), ("MIDDLE + 300", 1097, 300, 0)]:
        worst = 0
        for route, opts in G.ROUTES.items():
            base = kernels(route_check, N, k, opts, skinny)
            worst = max(worst, max(tiles(case) for _, case, _, _, _ in base))
            assert base and not {kern for _, _, _, _, kern in base} & set(LDS_DMA_FAMILY)
            for more in LDS_DMA_OPTIONS:
                assert kernels(route_check, N, k, opts, skinny, **more) == base, (name, route, more)
        print("%s: the largest launch has %d tiles" % (name, worst))
        assert worst < 128


def test_wider_reaches_what_it_is_there_for(route_check):
    got = {route: case_kernels(route_check, "WIDER", route) for route in G.APPEND_ROUTES["WIDER"]}
    rank = {route: [(str(c), kern) for s, c, _, _, kern in ans if s == "rank"] for route, ans in got.items()}
    for route in got:
        want = TALL if route == "tall" else DMA8
        assert rank[route] == [("2304x2176xK640-lower+0", want)], (route, rank[route])
    for route in ("la256_deep", "la256_shallow"):
        assert {kern for s, _, _, _, kern in got[route] if s in ("trsm", "sweep")} == {SMALL3}
        assert {sh for s, _, sh, _, _ in got[route] if s in ("trsm", "sweep")} == {BESIDE_UPDATE}
        assert {kern for s, _, _, _, kern in got[route] if s == "trail"} == {SMALL3}
    assert {kern for s, _, _, _, kern in got["la256_deep"] if s == "panel"} == {SMALL3}
    assert {kern for s, _, _, _, kern in got["la256_shallow"] if s == "panel"} == {SMALL8}        # chip_shared_only keeps the deep ring
    assert {kern for _, _, _, _, kern in got["default"]} == {SMALL8, DMA8, TRAIL}
    # persist0 changes nothing here (18 x 17 tiles lower are one round at the most): it is the contrast to PERSIST
    assert [a[1:] for a in got["persist0"]] == [a[1:] for a in got["default"]]


def border_of(N, k):
    return (N + k + 127) // 128 * 128 - N // 128 * 128


def test_ticket_and_persist_are_the_smallest_sizes_that_reach_their_kernels(route_check):
    rank = lambda N, k, opts: [kern for s, _, _, _, kern in kernels(route_check, N, k, opts) if s == "rank"]   # noqa: E731
    for name, route, want, hand in (("TICKET", "ticket2", TICKET, 2816), ("PERSIST", "default", PERSIST, 3968)):
        N, k, _ = G.APPENDS[name]
        opts = G.APPEND_ROUTES[name][route]
        assert rank(N, k, opts) == [want], name
        assert rank(N, k - 1, opts) == [DMA8], "%s: one point less is one tile row less, and the plain kernel" % name
        assert (N + k - 1) % 128 == 0 and border_of(N, k) == border_of(N, k - 1) + 128
        for fewer in range(border_of(N, k) - 128, 2048, -128):          # and no smaller border reaches it
            assert rank(N, fewer - 128 + N // 128 * 128 - N + 1, opts) == [DMA8], (name, fewer)
        print("%s: border %d (by hand from live tiles: %d)" % (name, border_of(N, k), hand))
        assert border_of(N, k) < hand
    assert (border_of(*G.APPENDS["TICKET"][:2]), border_of(*G.APPENDS["PERSIST"][:2])) == (2560, 3584)
    N, k, _ = G.APPENDS["PERSIST"]
    assert rank(N, k, G.APPEND_ROUTES["PERSIST"]["persist0"]) == [DMA8]
    assert rank(N, k, {"gemm_ticket": 2}) == [TICKET] and rank(*G.APPENDS["TICKET"][:2], {}) == [DMA8]


# ------------------------------------------------------------------------------------------------------------ the plans
PLAN_DRIVER = r"""
// one line per plan: "a N k ld rows yrow ld_pad reserve fused skinny_opt" or "r N ld rows yrow ld_pad k idx*"
#include <cstdio>
#include <iostream>
#include <sstream>
#include <string>
#include <vector>
#include "gpmi_append_plan.h"
#include "gpmi_remove_plan.h"
int main() {
    std::string line;
    while (std::getline(std::cin, line)) {
        std::istringstream is(line);
        std::string what;
        is >> what;
        if (what == "a") {
            long long N, k, ld, rows, yrow, pad, reserve; int fused, opt;
            is >> N >> k >> ld >> rows >> yrow >> pad >> reserve >> fused >> opt;
            const gpmi::AppendPlan p = gpmi::append_plan(N, k, ld, rows, yrow, pad, reserve, fused, opt);
            printf("%lld %lld %lld %d %d %d %lld %lld %lld\n", (long long)p.N0, (long long)p.Np1, (long long)p.border, (int)p.skinny,
                   (int)p.in_place, (int)p.yrow_moves, (long long)p.ld, (long long)p.rows, (long long)p.yrow);
        } else if (what == "r") {
            long long N, ld, rows, yrow, pad, k;
            is >> N >> ld >> rows >> yrow >> pad >> k;
            std::vector<int64_t> idx((size_t)k);
            for (int64_t& v : idx) { long long t; is >> t; v = t; }
            const gpmi::RemovePlan p = gpmi::remove_plan(N, idx.data(), k, ld, rows, yrow, pad);
            printf("%d %lld %lld %lld %lld %lld %zu", (int)p.ok, (long long)p.J0, (long long)p.N_out, (long long)p.Np_out,
                   (long long)p.ld, (long long)p.rows, p.sweeps.size());
            for (const gpmi::RemoveSweep& s : p.sweeps) printf(" %lld", (long long)s.J0);
            printf("\n");
        }
    }
    return 0;
}
"""
LD_PAD = 544                    # gpmi_ctx::ld_pad


@pytest.fixture(scope="module")
def plans(tmp_path_factory):
    """append_plan and remove_plan of the headers, built the way tests/test_append_plan_cpu.py builds append_plan_check"""
    if shutil.which("g++") is None:
        pytest.skip("needs g++")
    tmp = tmp_path_factory.mktemp("plans")
    src, exe = str(tmp / "plans.cpp"), str(tmp / "plans")
    open(src, "w").write(PLAN_DRIVER)
    subprocess.check_call([shutil.which("g++"), "-O1", "-g", "-std=c++17", "-fno-omit-frame-pointer", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=all", "-Wall", "-Wextra", "-Werror", "-I",
                           os.path.join(ROOT, "gaussian_process_amd", "csrc"), "-o", exe, src])

    def ask(lines):
        env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")
        p = subprocess.run([exe], input="".join(" ".join(str(w) for w in q) + "\n" for q in lines), env=env, capture_output=True,
                           text=True, timeout=600)
        assert p.returncode == 0, p.stdout[-2000:] + p.stderr[-4000:]
        assert "runtime error" not in p.stderr and "AddressSanitizer" not in p.stderr, p.stderr[-4000:]
        out = [[int(w) for w in row.split()] for row in p.stdout.splitlines()]
        assert len(out) == len(lines)
        return out
    return ask


def round_up(n):
    return (n + 127) // 128 * 128


def fit_layout(N, reserve=0, n_test=0):
    """ensure_train_buffers (driver.hip) -> ld, rows, yrow; n_test: the one-pass fit with the posterior factor, whose test
    rows have columns of their own and come before the y rows"""
    cap, npt = round_up(N + reserve), round_up(n_test)
    return cap + npt + LD_PAD, cap + 128 + npt, round_up(N) + npt


def append_plan(N, k, ld, rows, yrow, reserve, fused, skinny_opt):
    """gpmi_append_plan.h restated -> dict(N0, Np1, border, skinny, in_place, yrow_moves, ld, rows, yrow)"""
    p = dict(N0=N // 128 * 128, Np1=round_up(N + k))
    p["border"] = p["Np1"] - p["N0"]
    p["skinny"] = bool(k <= 16 and fused and p["N0"] > 0 and skinny_opt != 0)
    p["in_place"] = p["Np1"] <= ld - LD_PAD and p["Np1"] + 128 <= rows
    p["yrow_moves"] = p["Np1"] != yrow
    p["ld"], p["rows"] = (ld, rows) if p["in_place"] else (round_up(N + k + reserve) + LD_PAD, round_up(N + k + reserve) + 128)
    p["yrow"] = p["Np1"]
    return p


PLAN_WORDS = ("N0", "Np1", "border", "skinny", "in_place", "yrow_moves", "ld", "rows", "yrow")
# name: (N, k, reserve, test points of a one-pass fit, append_skinny) -> N0, Np1, border, skinny, in_place, yrow_moves
APPEND_PLANS = {
    "WIDE": ((700, 900, 0, 0, -1), (640, 1664, 1024, 0, 0, 1)),
    "WIDER": ((700, 2000, 0, 0, -1), (640, 2816, 2176, 0, 0, 1)),
    "TICKET": ((700, 2373, 0, 0, -1), (640, 3200, 2560, 0, 0, 1)),
    "PERSIST": ((700, 3397, 0, 0, -1), (640, 4224, 3584, 0, 0, 1)),
    "SKINNY": ((1500, 16, 0, 0, 1), (1408, 1536, 128, 1, 1, 0)),
    "WIDE reserve1000": ((700, 900, 1000, 0, -1), (640, 1664, 1024, 0, 1, 1)),
    "WIDE one_pass900": ((700, 900, 0, 900, -1), (640, 1664, 1024, 0, 1, 1)),
    "EDGES + 300": ((1084, 300, 0, 0, 0), (1024, 1408, 384, 0, 0, 1)),
    "THIRDS + 300": ((900, 300, 0, 0, 0), (896, 1280, 384, 0, 0, 1)),
    "MIDDLE + 300": ((1097, 300, 0, 0, 0), (1024, 1408, 384, 0, 0, 1)),
}


def test_append_plans(plans):
    """N0, border, the route, in place or not and the y row's move of every append of the GPU module, from the header and
    from the restatement above"""
    for name, (N, k, skinny) in G.APPENDS.items():
        assert APPEND_PLANS[name][0] == (N, k, 0, 0, skinny)
    for how, (reserve, n_test) in G.IN_PLACE.items():
        assert APPEND_PLANS["WIDE %s" % how][0] == G.APPENDS["WIDE"][:2] + (reserve, n_test, -1)
    for which, idx in G.REMOVALS.items():
        assert APPEND_PLANS["%s + 300" % which][0] == (G.REMOVE_N - len(idx), G.REMOVE_APPEND, 0, 0, 0)
    for fused in (1, 0):
        lines, want = [], []
        for name, ((N, k, reserve, n_test, skinny), claimed) in APPEND_PLANS.items():
            # behind a removal the allocation is still the one of the fit of 1100 points
            ld, rows, yrow = fit_layout(G.REMOVE_N if "+" in name else N, reserve, n_test)
            yrow = round_up(N) if "+" in name else yrow
            lines.append(("a", N, k, ld, rows, yrow, LD_PAD, reserve, fused, skinny))
            p = append_plan(N, k, ld, rows, yrow, reserve, fused, skinny)
            want.append([int(p[w]) for w in PLAN_WORDS])
            claimed = claimed[:3] + (claimed[3] if fused else 0,) + claimed[4:]
            assert tuple(int(p[w]) for w in PLAN_WORDS[:6]) == claimed, (name, fused, p)
        assert plans(lines) == want
    # the skinny append of 5 behind both: inside the padding of the allocation the padded append left
    for n in (1084 + 300, 900 + 300, 1097 + 300):
        ld, rows = round_up(n) + LD_PAD, round_up(n) + 128
        p = append_plan(n, G.REMOVE_SKINNY, ld, rows, round_up(n), 0, 1, 1)
        assert p["skinny"] and p["in_place"] and not p["yrow_moves"] and [[int(p[w]) for w in PLAN_WORDS]] == plans(
            [("a", n, G.REMOVE_SKINNY, ld, rows, round_up(n), LD_PAD, 0, 1, 1)])
    # the one-pass layout: 900 test points give 1024 columns and rows behind the 768 of the fit, the y row at 1792
    assert fit_layout(700, 0, 900) == (1792 + LD_PAD, 1920, 1792) and fit_layout(700, 1000) == (1792 + LD_PAD, 1920, 768)


def test_remove_plans(plans):
    """EDGES is one sweep from J0 = 0; every third index below 600 is 13 sweeps in descending groups of 16, the first from
    J0 = 512, the last from 0 -- the call's J0, from which the stored inverses are written once, at the end; MIDDLE is one
    sweep from J0 = 256 with the 16 x 16 tiles 16 and 17 in front of its first index; the layout stays"""
    ld, rows, yrow = fit_layout(G.REMOVE_N)
    out = plans([("r", G.REMOVE_N, ld, rows, yrow, LD_PAD, len(idx)) + tuple(idx) for idx in G.REMOVALS.values()])
    edges, thirds, middle = out
    assert middle == [1, 256, 1097, 1152, ld, rows, 1, 256] and min(G.REMOVALS["MIDDLE"]) // 16 - 256 // 16 == 2
    assert edges == [1, 0, 1084, 1152, ld, rows, 1, 0]
    assert thirds[:7] == [1, 0, 900, 1024, ld, rows, 13]
    assert thirds[7:] == [512, 384, 384, 384, 256, 256, 256, 128, 128, 0, 0, 0, 0]
    groups = [sorted(G.REMOVALS["THIRDS"])[max(0, 200 - 16 * (i + 1)):200 - 16 * i] for i in range(13)]
    assert [g[0] // 128 * 128 for g in groups] == thirds[7:]
    assert groups[0][0] == 552 and groups[0][0] // 16 - thirds[7] // 16 == 2           # tiles 32 and 33 hold no removed index
    assert [len(g) for g in groups] == [16] * 12 + [8]


# ------------------------------------------------------------------------------------------------------------ the mirror
def two_float64_evaluations(X, y):
    """-> (A, B): the quantities the device is held to, in float64 twice.  A: ard_ref.lml_and_grad (the explicit
    symmetrised inverse) with the LOO closed forms of loo_ref.from_Ky on that inverse.  B: from the Cholesky factor --
    m and alpha by triangular solves, K_y^-1 = L^-T L^-1 from L^-1 by a triangular solve on the identity, kappa the squared
    column norms of L^-1"""
    N, d = X.shape
    r = np.ones(d)
    ard = ard_ref.lml_and_grad(X, y, r, G.SIGMA, G.ELL, G.NOISE)
    kappa = np.diag(ard["Kinv"]).copy()
    mu, var = y - ard["alpha"] / kappa, 1.0 / kappa
    logp = loo_ref._logp(y, mu, var)
    A = dict(lml=ard["lml"], alpha=ard["alpha"], grad=(ard["g_r"], ard["g_l"], ard["g_sigma"], ard["g_noise"]),
             loo=(mu, var, logp, float(np.sum(logp))))
    part = lambda k: (X[:, None, k] - X[None, :, k]) ** 2      # noqa: E731
    sq = np.zeros((N, N))
    for k in range(d):
        sq += part(k)
    K = G.SIGMA ** 2 * np.exp(-.5 / G.ELL ** 2 * sq)
    L = np.linalg.cholesky(K + G.NOISE * np.eye(N))
    Linv = solve_triangular(L, np.eye(N), lower=True, check_finite=False)
    Kinv = Linv.T @ Linv
    m = solve_triangular(L, y, lower=True)
    alpha = solve_triangular(L, m, lower=True, trans="T")
    trace = lambda Dm: .5 * (alpha @ Dm @ alpha) - .5 * np.sum(Kinv * Dm)      # noqa: E731
    kappa = np.sum(Linv * Linv, axis=0)
    mu, var = y - alpha / kappa, 1.0 / kappa
    logp = loo_ref._logp(y, mu, var)
    B = dict(lml=-.5 * (m @ m) - np.sum(np.log(np.diag(L))) - .5 * N * np.log(2 * np.pi), alpha=alpha,
             grad=(np.array([trace(K * part(k) / G.ELL ** 2) for k in range(d)]), trace(K * sq / G.ELL ** 3), trace(2 * K / G.SIGMA),
                   trace(np.eye(N))),
             loo=(mu, var, logp, float(np.sum(logp))))
    return A, B, ard


def apart(A, B, ard, y):
    """difference / bar of the quantities a GPU case holds, in hold()'s normalisation"""
    filler = dict(ratio=0.0, m=np.ones(1), diag=np.ones(1), mu=np.zeros(1), sd=np.zeros(1))
    e = G.errors(dict(A, **filler), dict(B, **filler), dict(lml=B["lml"], alpha=B["alpha"], scales=lambda: ard), y)
    return {k: e[k] for k in ("lml", "alpha", "grad", "loo")}


# what the two float64 evaluations of PERSIST's final data were apart when this was written, over the bar
FLOAT64_APART = dict(lml=0.0, alpha=1.4e-5, grad=4.0e-7, loo=1.2e-2)


def test_two_float64_evaluations_of_the_largest_problem_agree():
    name = max(G.APPENDS, key=lambda n: sum(G.APPENDS[n][:2]))
    assert name == "PERSIST" and sum(G.APPENDS[name][:2]) == 4097 > G.REMOVE_N + G.REMOVE_APPEND + G.REMOVE_SKINNY
    X, y, _ = G.append_data(name)
    A, B, ard = two_float64_evaluations(X, y)
    e = apart(A, B, ard, y)
    print("%s, %d points: two float64 evaluations, difference / bar  " % (name, len(y)) + "  ".join("%s %.2e" % kv for kv in e.items()))
    for k, v in e.items():
        assert v <= 0.1, (k, v)
        assert v <= max(3 * FLOAT64_APART[k], 1e-3), (k, v)


# ------------------------------------------------------------------------------------------- a stand-in for the device
class MirrorContext:
    """GPContext as tests/test_resize_routes_gpu.py uses it, on NumPy: fit, append and remove are a float64 Cholesky fit of
    the resulting data; the layout follows ensure_train_buffers, append_plan and remove_plan; what the device refuses is
    refused in its words.  Options are recorded, not obeyed: every route gives the same bits here, which is all the
    module asserts BETWEEN routes."""

    def __init__(self):
        self.opts = dict(G.DEFAULTS)
        self.set_calls = 0
        self.N = self.d = 0
        self.L = None

    def set_option(self, name, value):
        assert name in G.DEFAULTS, name
        self.opts[name] = value
        self.set_calls += 1

    def set_lengthscales(self, r):
        assert r is None

    def rbf(self, a, b, sigma, l):
        sq = np.zeros((len(a), len(b)))
        for k in range(a.shape[1]):
            sq += (a[:, None, k] - b[None, :, k]) ** 2
        return sigma ** 2 * np.exp(-.5 / l ** 2 * sq)

    def set_train(self, X, y):
        self.X, self.y = np.array(X, dtype=np.float64), np.array(y, dtype=np.float64)
        self.N, self.d = self.X.shape
        self.L = None

    def set_test(self, Xs):
        self.Xs = np.array(Xs)

    def _factorize(self, lead=None):
        """lead: (L0, m0), the leading block of a resident factor that the rows of X still in front belong to -- the factor
        is then bordered (W = K_b0 L0^-T, chol(K_bb - W W^T)) as the device does it, and the block keeps its bits"""
        self.L = None
        Ky = self.rbf(self.X, self.X, self.sigma, self.ell) + self.noise * np.eye(self.N)
        n0 = 0 if lead is None else len(lead[1])
        L, m = np.zeros_like(Ky), np.zeros(self.N)
        S, yb = Ky[n0:, n0:], self.y[n0:]
        if n0:
            L[:n0, :n0], m[:n0] = lead
            W = solve_triangular(lead[0], Ky[n0:, :n0].T, lower=True).T
            L[n0:, :n0], S, yb = W, S - W @ W.T, yb - W @ lead[1]
        c, info = lapack.dpotrf(S, lower=1, clean=1)
        if info > 0:
            err = np.linalg.LinAlgError("Matrix is not positive definite")
            err.bad_pivot = n0 + int(info)
            raise err
        L[n0:, n0:] = c
        m[n0:] = solve_triangular(c, yb, lower=True)
        self.L, self.Ky, self._m = L, Ky, m
        return -.5 * (m @ m) - np.sum(np.log(np.diag(L))) - .5 * self.N * np.log(2 * np.pi)

    def factorize(self, sigma, l, noise_var):
        self.sigma, self.ell, self.noise = sigma, l, noise_var
        self.fused = self.opts["panel_fused"]
        self.ld, self.rows, self.yrow = fit_layout(self.N, self.opts["reserve"])
        self.route = getattr(self, "route", -1)
        return self._factorize()

    def fit(self, X, y, sigma, l, noise_var, *, lengthscales):
        assert lengthscales is None
        self.set_train(X, y)
        return self.factorize(sigma, l, noise_var)

    def fit_predict_sample_resident(self, sigma, l, noise_var, jitter, want_sd=True, want_factor=True):
        lml = self.factorize(sigma, l, noise_var)
        self.ld, self.rows, self.yrow = fit_layout(self.N, self.opts["reserve"], len(self.Xs))
        return lml, None, None, None

    def _resident(self):
        if self.L is None:
            raise ValueError("gpmi: no factorisation resident")

    def append(self, Xnew, ynew):
        self._resident()
        p = append_plan(self.N, len(ynew), self.ld, self.rows, self.yrow, self.opts["reserve"], self.fused, self.opts["append_skinny"])
        lead = (self.L[:p["N0"], :p["N0"]].copy(), self._m[:p["N0"]].copy())
        self.X, self.y = np.vstack([self.X, Xnew]), np.concatenate([self.y, ynew])
        self.N = len(self.y)
        self.ld, self.rows, self.yrow, self.route = p["ld"], p["rows"], p["yrow"], int(p["skinny"])
        return self._factorize(lead)

    def remove(self, idx):
        self._resident()
        keep = np.setdiff1d(np.arange(self.N), np.asarray(idx))
        assert len(keep) == self.N - len(idx) > 0
        J0 = int(np.min(idx)) // 128 * 128
        lead = (self.L[:J0, :J0].copy(), self._m[:J0].copy())
        self.X, self.y, self.N = self.X[keep], self.y[keep], len(keep)
        self.yrow = round_up(self.N)
        return self._factorize(lead)

    def layout(self):
        return dict(N=self.N, Np=round_up(self.N), ld=self.ld, rows=self.rows, route=self.route)

    def factor(self, r0=0, r1=None, c0=0, c1=None):
        self._resident()
        return np.array(self.L[r0:self.N if r1 is None else r1, c0:self.N if c1 is None else c1])

    def m(self):
        self._resident()
        return self._m.copy()

    def diag(self):
        self._resident()
        return np.diag(self.L).copy()

    def alpha(self):
        self._resident()
        return solve_triangular(self.L, self._m, lower=True, trans="T")

    def predict(self, Xs, want_sd=True):
        self._resident()
        v = solve_triangular(self.L, self.rbf(self.X, np.asarray(Xs), self.sigma, self.ell), lower=True)
        var = self.sigma ** 2 - np.sum(v * v, axis=0)
        return v.T @ self._m, np.sqrt(var) if want_sd else var

    def _inverse(self):
        return cho_solve((self.L, True), np.eye(self.N))

    def lml_grad_ard(self):
        self._resident()
        Kinv, alpha, K = self._inverse(), self.alpha(), self.Ky - self.noise * np.eye(self.N)
        trace = lambda Dm: .5 * (alpha @ Dm @ alpha) - .5 * np.sum(Kinv * Dm)      # noqa: E731
        parts = [(self.X[:, None, k] - self.X[None, :, k]) ** 2 for k in range(self.d)]
        return (np.array([trace(K * q / self.ell ** 2) for q in parts]), trace(K * sum(parts) / self.ell ** 3),
                trace(2 * K / self.sigma), trace(np.eye(self.N)))

    def loo(self):
        self._resident()
        kappa, alpha = np.diag(self._inverse()).copy(), self.alpha()
        mu, var = self.y - alpha / kappa, 1.0 / kappa
        logp = loo_ref._logp(self.y, mu, var)
        return mu, var, logp, float(np.sum(logp))


@pytest.fixture(scope="module")
def mirrors():
    a, f = MirrorContext(), MirrorContext()
    yield a, f
    # every option of both contexts is back at its default, and options were set at all
    for c in (a, f):
        assert c.opts == G.DEFAULTS and c.set_calls > 0


def test_the_lean_row_ratio_is_the_one_of_the_removal_tests():
    """ratio_rows converts only the slices it needs to long double: the same figure as test_remove_gpu._ratio_rows"""
    X, y, _ = TR._problem(300, 8)
    c = MirrorContext()
    c.fit(X, y, G.SIGMA, G.ELL, G.NOISE, lengthscales=None)
    rows = G.sample_rows(300, 128, cap=20)
    assert 18 <= len(rows) <= 20 and rows[0] == 128 and rows[-1] == 299      # the sample may draw the first or the last row again
    assert G.ratio_rows(c.Ky, c.factor(), rows) == TR._ratio_rows(c.Ky, c.factor(), rows) > 0
    # beyond 700 points the rows are sampled, fewer as n grows: about n^2 long-double flops each
    for n, cap in ((1600, 64), (2700, 64), (3073, 52), (4097, 29)):
        assert cap - 2 <= len(G.sample_rows(n, 640)) <= cap, n
    assert G.factor_ratio(c.Ky, c.factor(), 0) <= 1.0


STAND_IN_APPENDS = [("WIDE", "default"), ("WIDE", "la256_deep"), ("SKINNY", "nb128")]


@pytest.mark.parametrize("name,route", STAND_IN_APPENDS)
def test_append_cases_on_the_stand_in(mirrors, name, route):
    G.test_append_on_every_route(*mirrors, name, route)


@pytest.mark.parametrize("how", list(G.IN_PLACE))
def test_in_place_cases_on_the_stand_in(mirrors, how):
    G.test_append_in_place(*mirrors, how, "default")


@pytest.mark.parametrize("which,route", [("EDGES", "default"), ("THIRDS", "lookahead0"), ("MIDDLE", "panel_fused0")])
def test_remove_cases_on_the_stand_in(mirrors, which, route):
    G.test_remove_on_every_route(*mirrors, which, route)


def test_the_flipped_removal_on_the_stand_in(mirrors):
    G.test_removal_follows_the_resident_factor(*mirrors, 0)


def test_the_failing_pivot_on_the_stand_in(mirrors):
    """K - I / 2 of the grid is positive definite up to the duplicated point, whose pivot is -1.5: LAPACK names the same
    column as the device must"""
    N, N0, X, y = G.pivot_problem()
    Ky = MirrorContext().rbf(X, X, 1.0, 1.0) - .5 * np.eye(len(X))
    assert np.max(np.abs(Ky - .5 * np.eye(len(X)) - (Ky > .25) * (1 - np.eye(len(X))))) < 1e-20       # the identity but for one pair
    assert lapack.dpotrf(Ky, lower=1)[1] == N0 + G.PIVOT_COLUMN + 1 == 1241
    G.test_failed_pivot_in_the_second_block(*mirrors, "la256_deep")
    G.test_worst_figures()
    assert set(G.WORST) >= {"factor", "fresh_factor", "lml", "m", "diag", "alpha", "mu", "sd", "grad", "loo", "f64_lml", "f64_alpha"}
