"""What tests/test_sparse_routes_gpu.py rests on, without a GPU:

* the plan header of the sparse fit (gaussian_process_amd/csrc/gpmi_sparse_plan.h: gram_plan, sparse_slabs) under g++
  AddressSanitizer + UBSan, held against brute force by tests/sanitize/sparse_plan_check.cpp -- a program of its own,
  nothing is loaded into Python;
* the plans that program prints for the GPU test's shapes: they are the edges its docstring claims;
* the kernels gemm_route (csrc/gpmi_route.h, through tests/sanitize/gemm_route_check.cpp) answers for every GEMM launch
  of those problems: MID, P600, RAGGED and the N = 641 case stay below 128 tiles, where gemm_tall, gemm_persist and
  gemm_ticket cannot change a kernel; TILES reaches the LDS-DMA family, and the kernels are recorded here;
* the float64 mirror (tests/sgpr_ref.py: fit) against its own long-double run at P600: every gap is at most half of the
  device's bar, so the mirror does not use up the bars."""
import os
import shutil
import subprocess

import numpy as np
import pytest

import gemm_route_table as T
import sgpr_ref as S
import test_sparse_gpu as TS
import test_sparse_routes_gpu as G
from conftest import ROOT
from test_gemm_route_cpu import MI355X_GROUPS, query, route_check       # noqa: F401 (route_check is a fixture)

C = T.Case


# ---------------------------------------------------------------------------------------------------- the plan header
@pytest.fixture(scope="module")
def plan_check(tmp_path_factory):
    if shutil.which("g++") is None:
        pytest.skip("needs g++")
    exe = str(tmp_path_factory.mktemp("sparse_plan") / "sparse_plan_check")
    subprocess.check_call([shutil.which("g++"), "-O1", "-g", "-std=c++17", "-fno-omit-frame-pointer", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=all", "-Wall", "-Wextra", "-Werror", "-I",
                           os.path.join(ROOT, "gaussian_process_amd", "csrc"), "-o", exe,
                           os.path.join(ROOT, "tests", "sanitize", "sparse_plan_check.cpp")])

    def run(*args):
        env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")
        p = subprocess.run([exe] + [str(a) for a in args], env=env, capture_output=True, text=True, timeout=600)
        assert p.returncode == 0, p.stdout[-2000:] + p.stderr[-4000:]
        assert "runtime error" not in p.stderr and "AddressSanitizer" not in p.stderr, p.stderr[-4000:]
        return p.stdout
    return run


def test_plan_header_under_asan_ubsan(plan_check):
    """m_p in 128..4096 and rows in 128..20480: the chunks are multiples of 128, in order, disjoint and cover the rows,
    nsplit <= units and <= 65535, the chunk is the shortest the target of 1024 workgroups allows; for every (N_p, slab
    option, m_p): the slabs cover N_p, part_doubles takes every slab of the fit and the gemv scratch every slab"""
    assert "sparse_plan_check: ok (5120 plans" in plan_check()


def plan(plan_check, N, slab, mp):
    """-> (the fit's figures, [the figures of each slab]) as dicts"""
    lines = [ln.split() for ln in plan_check("plan", N, slab, mp).splitlines()]
    assert lines[0][0] == "fit" and all(ln[0] == "slab" for ln in lines[1:])
    lines[0] = lines[0][1:]                  # "fit Np 768 S 512 ...", then "slab 0 rows 512 ..."
    rows = [dict(zip(ln[0::2], map(int, ln[1::2]))) for ln in lines]
    assert len(rows) == 1 + rows[0]["nslabs"]
    return rows[0], rows[1:]


def mp_of(m):
    return (m + 127) // 128 * 128


def test_the_gpu_shapes_are_the_edges_claimed(plan_check):
    mp = {name: mp_of(shape[2]) for name, shape in G.PROBLEMS.items()}
    assert mp == {"MID": 384, "P600": 640, "TILES": 2304, "RAGGED": 1152}
    # every launch of the other sparse tests: one unit per split, at most 6 tiles
    for N, d, m, noise in S.CASES + [S.MID, (129, 2, 40, 1e-2), (641, 5, 130, 5e-4)]:
        for slab in (0, 128, 256):
            fit, slabs = plan(plan_check, N, slab, mp_of(m))
            assert fit["ntiles"] <= 6 and all(s["chunk"] == 128 and s["nsplit"] == s["units"] for s in slabs)
    # P600: two panel blocks at the default nb (512 + 128), and the contraction grid (ceil(m_p / 256) column groups of
    # 256 lanes) has a third group whose upper half is beyond m_p
    fit, slabs = plan(plan_check, G.PROBLEMS["P600"][0], 0, mp["P600"])
    assert mp["P600"] > 512 and mp["P600"] - 512 == 128 and mp["P600"] % 256 == 128 and (mp["P600"] + 255) // 256 == 3
    assert fit["ntiles"] == 15 and [s["rows"] for s in slabs] == [768]
    # TILES, one slab: 19 units in 5 splits of 512 rows, the last 384
    fit, slabs = plan(plan_check, G.PROBLEMS["TILES"][0], 0, mp["TILES"])
    assert fit["ntiles"] == 171 and slabs == [dict(slab=0, rows=2432, real=2400, units=19, nsplit=5, chunk=512, last_chunk=384)]
    # TILES, sparse_slab 1408: 6 splits of 256 with a 128-row tail, then a last slab of 1024 rows
    fit, slabs = plan(plan_check, G.PROBLEMS["TILES"][0], G.TILES_SLAB, mp["TILES"])
    assert slabs == [dict(slab=0, rows=1408, real=1408, units=11, nsplit=6, chunk=256, last_chunk=128),
                     dict(slab=1, rows=1024, real=992, units=8, nsplit=4, chunk=256, last_chunk=256)]
    # RAGGED: 45 tiles; 12 splits of 256, then 1664 rows in 13 splits of 128 -- more than the full slab has, which is what
    # part_doubles is the max of two plans for; the last unit holds 92 real rows
    fit, slabs = plan(plan_check, G.PROBLEMS["RAGGED"][0], G.RAGGED_SLAB, mp["RAGGED"])
    assert fit["ntiles"] == 45
    assert slabs == [dict(slab=0, rows=3072, real=3072, units=24, nsplit=12, chunk=256, last_chunk=256),
                     dict(slab=1, rows=1664, real=1628, units=13, nsplit=13, chunk=128, last_chunk=128)]
    assert slabs[1]["nsplit"] > slabs[0]["nsplit"] and fit["part_doubles"] == 45 * 13 * 128 * 128
    assert slabs[1]["real"] - (slabs[1]["units"] - 1) * 128 == 92
    # the ragged last slab: 512 + 256 rows, 129 of the latter real
    (N, d, m, noise), slab = G.LAST_SLAB
    fit, slabs = plan(plan_check, N, slab, mp_of(m))
    assert [(s["rows"], s["real"]) for s in slabs] == [(512, 512), (256, 129)]


# ---------------------------------------------------------------------------------------------------- the GEMM launches
def panel_updates(mrows, w, leaf, off=0):
    """the GEMMs of panel_rec (driver.hip) for a panel of w columns and mrows rows"""
    if w <= leaf:
        return []
    h = (w // 2) // leaf * leaf
    c0 = off + h
    r0 = c0 // 128 * 128
    return (panel_updates(mrows, h, leaf, off) + [(C(mrows - r0, w - h, h, lower=1, diag_off=r0 - c0), 0)]
            + panel_updates(mrows, w - h, leaf, off + h))


def chol_launches(ncols, nrows, nb, la, leaf):
    """cholesky_inplace: the panels' updates and the trailing updates (role 1; under lookahead the next block column
    goes first, with role 0)"""
    out = []
    for k in range(0, ncols, nb):
        w = min(nb, ncols - k)
        out += panel_updates(nrows - k, w, leaf)
        r0 = k + w
        if r0 >= ncols:
            continue
        if not la:
            out.append((C(nrows - r0, ncols - r0, w, lower=1), 1))
            continue
        nbn = min(nb, ncols - r0)
        out.append((C(nrows - r0, nbn, w, lower=1), 0))
        if r0 + nbn < ncols:
            out.append((C(nrows - r0 - nbn, ncols - r0 - nbn, w, lower=1), 1))
    return out


def trsm_updates(m, w, leaf):
    if w <= leaf:
        return []
    h = (w // 2) // leaf * leaf
    return trsm_updates(m, h, leaf) + [(C(m, w - h, h), 0)] + trsm_updates(m, w - h, leaf)


def sweep_launches(Np, m, nb, la, leaf, tri=False):
    """solve_sweep_factor: the updates inside trsm_block and the sweep's own"""
    out = []
    for k in range(0, Np, nb):
        w = min(nb, Np - k)
        rows = min(m, k + w) if tri else m
        out += trsm_updates(rows, w, leaf)
        r0 = k + w
        if r0 >= Np:
            continue
        if not la:
            out.append((C(rows, Np - r0, w), 0))
            continue
        nbn = min(nb, Np - r0)
        out.append((C(rows, nbn, w), 0))
        if r0 + nbn < Np:
            out.append((C(rows, Np - r0 - nbn, w), 0))
    return out


def launches(mp, slab_rows, nb, la=False, leaf=128, grad=False):
    """every GEMM launch of a fit, a prediction of 64 points (one 128-row block) and, with grad, a gradient"""
    out = chol_launches(mp, mp, nb, la, leaf) + chol_launches(mp, mp + 128, nb, la, leaf)
    for rows in set(slab_rows) | {128}:
        out += sweep_launches(mp, rows, nb, la, leaf)
    if grad:
        out += sweep_launches(mp, mp, nb, la, leaf, tri=True)
        out += [(C(rows, mp, mp), 0) for rows in set(slab_rows) | {mp}]          # neg_product
    return out


def tiles(case):
    return (case.M // 128) * ((case.N + 127) // 128)


def ask(case, role, sharing=None, **more):
    words = query(MI355X_GROUPS, "small_dma8", case, sharing=sharing, **more).split()
    words[3] = str(role)
    return " ".join(words)


SMALL8, SMALL3 = "gemm_nt_small_kernel<8>", "gemm_nt_small_kernel<3>"
LDS_DMA_OPTIONS = [dict(gemm_tall=1, tall_min_tiles=0), dict(gemm_tall=0), dict(gemm_persist=0), dict(gemm_persist=1),
                   dict(gemm_ticket=1), dict(gemm_ticket=2)]
# (m_p, the slabs' rows, with a gradient): the problems that run on ROUTES, RAGGED and the ragged last slab
SMALL_PROBLEMS = {"MID": (384, [1536], True), "P600": (640, [768], True), "RAGGED": (1152, [3072, 1664], False),
                  "N641": (256, [512, 256], True)}


def small_launches(name):
    mp, slab_rows, grad = SMALL_PROBLEMS[name]
    # RAGGED runs at the default block size alone (512 below 12288 columns); the others under nb = 128, nb = 256 and
    # the lookahead split too, with both kinds of leaves
    forms = [(512, False, 128)] if name == "RAGGED" else [(nb, la, leaf) for nb in (128, 256, 512) for la in (False, True)
                                                          for leaf in (128, 64)]
    seen = []
    for nb, la, leaf in forms:
        for item in launches(mp, slab_rows, nb, la, leaf, grad):
            if item not in seen:
                seen.append(item)
    return seen


@pytest.mark.parametrize("name", list(SMALL_PROBLEMS))
def test_the_lds_dma_options_cannot_reach_these_launches(route_check, name):
    """fewer than 128 tiles of 128 x 128 in every launch: the 64 x 64 ring under every value of gemm_tall, gemm_persist
    and gemm_ticket, alone on the chip and beside a lookahead panel -- those options get no GPU route"""
    todo = small_launches(name)
    assert todo and max(tiles(case) for case, _ in todo) < 128
    print("%s: %d distinct launches, the largest %s (%d tiles)" % (name, len(todo), max(todo, key=lambda it: tiles(it[0]))[0],
                                                                    max(tiles(case) for case, _ in todo)))
    asked, want = [], []
    for case, role in todo:
        for more in LDS_DMA_OPTIONS:
            for sharing, kernel in (((0, 0), SMALL8), ((0, 1), SMALL8), ((1, 1), SMALL3)):
                asked.append(ask(case, role, sharing=sharing, **more))
                want.append(kernel)
    got = route_check(asked)
    wrong = ["%s: want %s, gemm_route %s" % (q, w, g) for q, w, g in zip(asked, want, got) if g != w]
    assert not wrong, "\n".join(wrong[:20])


def test_the_small_tile_options_can(route_check):
    todo = [(case, role) for name in ("MID", "P600") for case, role in small_launches(name) if case.N % 128 == 0]
    asked = [ask(case, role, **more) for case, role in todo for more in (dict(gemm_small_tiles=0), dict(gemm_small_dma=0))]
    got = route_check(asked)
    assert set(got[0::2]) == {"gemm_nt_kernel<4, 4, false>"} and set(got[1::2]) == {"gemm_nt_kernel<2, 2, false>"}


TRAIL, TRAIL_TALL = "chol_trailing_update_dma_kernel", "chol_trailing_update_dma256_kernel"
DMA8, TALL, TICKET = "gemm_nt_dma_kernel<2, false>", "gemm_nt_dma_tall_kernel<false>", "gemm_nt_dma_ticket_kernel"
# TILES (m_p 2304, default block size 512, no lookahead below 6144 columns): the launches of at least 128 tiles, with the
# kernel under the defaults, under gemm_tall = 1 with tall_min_tiles = 0, and under gemm_ticket = 2
TILES_LARGE = {
    (C(1792, 1792, 512, lower=1), 1): (TRAIL, TRAIL_TALL, TRAIL),       # first trailing update of K_uu
    (C(1920, 1792, 512, lower=1), 1): (TRAIL, TRAIL_TALL, TRAIL),       # ... of B, with the riding rows
    (C(2432, 1792, 512), 0): (DMA8, TALL, TICKET),                      # first sweep update, one slab of 2432 rows
    (C(1408, 1792, 512), 0): (DMA8, TALL, DMA8),                        # ... the slab of 1408 rows (154 tiles: under a round of 256)
    (C(2432, 1280, 512), 0): (DMA8, TALL, DMA8),                        # second sweep update of the one slab (190 tiles)
}


def test_tiles_reaches_the_lds_dma_family(route_check):
    """gemm_tall and gemm_ticket = 2 change a kernel of TILES and are routes of test_gram_plan_edges; gemm_persist and
    gemm_ticket = 1 change none (fewer than two rounds of blocks; no lookahead)"""
    assert set(G.GEMM_ROUTES) == {"default", "tall", "ticket2"}
    todo = []
    for item in launches(2304, [2432, 1408, 1024], 512):
        if item not in todo:
            todo.append(item)
    large = [it for it in todo if tiles(it[0]) >= 128]
    assert set(large) == set(TILES_LARGE), [str(c) for c, _ in large]
    variants = [G.GEMM_ROUTES["default"], G.GEMM_ROUTES["tall"], G.GEMM_ROUTES["ticket2"]]
    got = route_check([ask(case, role, **more) for case, role in large for more in variants])
    for i, item in enumerate(large):
        assert tuple(got[3 * i:3 * i + 3]) == TILES_LARGE[item], (str(item[0]), got[3 * i:3 * i + 3])
    base = route_check([ask(case, role) for case, role in todo])
    for more in (dict(gemm_persist=0), dict(gemm_persist=1), dict(gemm_ticket=1)):
        assert route_check([ask(case, role, **more) for case, role in todo]) == base, more


# ------------------------------------------------------------------------------------------------------------ the mirror
@pytest.mark.parametrize("method", TS.METHODS)
def test_the_float64_mirror_at_p600(method):
    """K_uu of P600 has condition 3.7e5.  float64 (LAPACK) against the same formulas in long double: each gap at most
    half of the bar the device is held to (test_sparse_gpu._hold)"""
    N, d, m, noise = G.PROBLEMS["P600"]
    X, y, Z, Xs, f64 = TS._mirror(N, d, m, noise, method)
    ld = S.fit(X, y, Z, S.SIGMA, S.ELL, noise, method=method, Xs=Xs, dtype=np.longdouble)
    f = lambda v: np.asarray(v, dtype=np.float64)        # noqa: E731
    gap = dict(value=float(abs(f64["value"] - ld["value"]) / ld["scale"]),
               c=np.max(np.abs(f(f64["c"] - ld["c"]))) / np.max(np.abs(f(ld["c"]))),
               q=np.max(np.abs(f(f64["q"] - ld["q"]))) / S.SIGMA ** 2,
               mean=np.max(np.abs(f(f64["mean"] - ld["mean"]))),
               var=np.max(np.abs(f(f64["var"] - ld["var"]))) / S.SIGMA ** 2)
    bar = dict(value=TS.LML_RTOL, c=1e-8, q=1e-10, mean=1e-9 * max(1.0, np.max(np.abs(y))), var=1e-10)
    print("P600 %s cond %.2e: float64 against long double  " % (method, f64["cond"])
          + "  ".join("%s %.1e (bar %.0e)" % (k, gap[k], bar[k]) for k in gap))
    assert 1e5 < f64["cond"] < 1e6
    for k in gap:
        assert gap[k] <= 0.5 * bar[k], (k, gap[k], bar[k])
