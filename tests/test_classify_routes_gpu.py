"""Both classifiers on every factor route a small problem can reach: the options of gpmi_set_option that
tests/test_parity_gpu.py drives for regression, under the Newton drivers of laplace.hip and softmax.hip, which use the
factor drivers in ways regression does not (C factorisations per step sharing one pivot word, a zeroed riding row,
solve_sweep(tri) on a diagonal seed, the lower GEMM with diag_off = r0 and K = Np - r0, one sweep over C * np_ rows,
panel_fused = 0 without the single-launch backward solve and its give-up word).

Problems: N = 641 (Np = 768: six tiles, the last holds one real row) for both classifiers, and N = 1100 with C = 4
(Np = 1152 is no multiple of the 512-wide blocks: two and a short one), sigma = 1.5, l = 3.0, d = 8.  Each mirror fit is
computed once.  Every route is held to the bounds of tests/test_laplace_gpu.py and tests/test_softmax_gpu.py, and fits
twice with the same bits.

The GEMM options gemm_tall (with tall_min_tiles = 0), gemm_persist and gemm_ticket choose among the kernels of the
128-tile LDS-DMA family, which gemm_route enters from 128 tiles of 128 x 128 on (tests/gemm_route_table.py: the cases of
"dma8", "tall", "persist", "ticket" all have at least 128).  The largest launch of these problems is 9 x 9 = 81 tiles,
so none of the three can change a kernel here; tests/test_classify_routes_cpu.py asks gemm_route and holds that.  They
have no case below.  What these shapes can reach is the 64 x 64 ring (gemm_small_tiles = 1, the default route), the
first-generation 64 x 64 kernel (gemm_small_dma = 0) and the first-generation 128 x 128 kernel (gemm_small_tiles = 0).

Bit equality BETWEEN routes is asserted for the lookahead routes alone: DESIGN.md (section 4, threshold table, la_min:
"same bits") and tests/test_parity_gpu.py::test_lookahead_threshold_does_not_change_the_bits claim it for
cholesky_inplace and solve_sweep."""
import functools

import numpy as np
import pytest

import laplace_ref as LR
import softmax_ref as SR

pytestmark = pytest.mark.gpu

SIGMA, ELL, D = 1.5, 3.0, 8
DEFAULTS = dict(nb=0, lookahead=1, la_min=6144, shallow_min=6144, panel_fused=1, trsv_vinv=2, gemm_small_tiles=1,
                gemm_small_dma=1)
ROUTES = {
    "default": {},                                           # gemm_small_tiles = 1: the 64 x 64 LDS-DMA ring
    "nb128": {"nb": 128},
    "nb256": {"nb": 256},
    "lookahead0": {"lookahead": 0},
    "la256_deep": {"lookahead": 1, "la_min": 256, "shallow_min": 0},          # never the one-launch panel kernels
    "la256_shallow": {"lookahead": 1, "la_min": 256, "shallow_min": 1 << 20},  # always
    "panel_fused0": {"panel_fused": 0},
    "trsv_vinv0": {"trsv_vinv": 0},
    "trsv_vinv1": {"trsv_vinv": 1},
    "trsv_vinv2": {"trsv_vinv": 2},
    "small_tiles0": {"gemm_small_tiles": 0},                 # first-generation 128 x 128 kernel
    "small_dma0": {"gemm_small_dma": 0},                     # first-generation 64 x 64 kernel
}
SAME_BITS_AS_DEFAULT = ("lookahead0", "la256_deep", "la256_shallow")
PROBLEMS = ("binary641", "softmax641_C3", "softmax1100_C4")
GAPS = {}                                                    # (problem, route) -> figures, for the report


class options:
    def __init__(self, ctx, opts):
        self.ctx, self.opts = ctx, opts

    def __enter__(self):
        for k, v in self.opts.items():
            self.ctx.set_option(k, v)

    def __exit__(self, *exc):
        for k in self.opts:
            self.ctx.set_option(k, DEFAULTS[k])


@functools.lru_cache(maxsize=None)
def data(name):
    """-> X, labels, X_test (300 points), classes (None: binary), normals"""
    if name == "binary641":
        rng = np.random.default_rng(641)                     # problem(641, 8, 641) of tests/test_laplace_gpu.py
        y = np.where(rng.random(641 + 300) < 0.5, -1.0, 1.0)
        X = rng.standard_normal((641 + 300, D)) * 1.5 + y[:, None] * (1.0 / np.sqrt(D))
        return X[:641], y[:641], X[641:], None, None
    N, C = (641, 3) if name == "softmax641_C3" else (1100, 4)
    X, lab, Xs = SR.blobs(N, D, C, N, n=300)
    return X, lab, Xs, C, np.random.default_rng(N).standard_normal((200, C))


@functools.lru_cache(maxsize=None)
def reference(name):
    X, lab, Xs, C, z = data(name)
    if C is None:
        ft = LR.laplace_fit(X, lab, SIGMA, ELL)
        mean, cov, prob, _ = LR.laplace_predict(ft, X, Xs, SIGMA, ELL)
        return dict(F=ft["f"], log_q=ft["log_q"], iters=ft["iters"], converged=ft["converged"], mean=mean, cov=cov, prob=prob)
    ft = SR.fit(X, lab, C, SIGMA, ELL)
    mean, cov = SR.predict(ft, X, Xs, SIGMA, ELL)
    return dict(F=ft["F"], log_q=ft["log_q"], iters=ft["iters"], converged=ft["converged"], mean=mean, cov=cov,
                prob=SR.proba(mean, cov, z))


def gpu_fit(ctx, name):
    X, lab, Xs, C, z = data(name)
    if C is None:
        return ctx.laplace_fit(X, lab, SIGMA, ELL)
    return ctx.softmax_fit(X, lab, C, SIGMA, ELL)


def gpu_predict(ctx, name):
    X, lab, Xs, C, z = data(name)
    return ctx.laplace_predict(Xs) if C is None else ctx.softmax_predict(Xs, z)


def gpu_run(ctx, name):
    log_q, F, iters, conv = gpu_fit(ctx, name)
    mean, cov, prob = gpu_predict(ctx, name)
    return dict(F=F, log_q=log_q, iters=iters, converged=conv, mean=mean, cov=cov, prob=prob)


def same_bits(a, b):
    return (a["log_q"] == b["log_q"] and a["iters"] == b["iters"]
            and all(np.array_equal(a[q], b[q]) for q in ("F", "mean", "cov", "prob")))


def hold_to_the_mirror(out, ref, tag):
    """the bounds of test_laplace_gpu.py / test_softmax_gpu.py: F 1e-9, log q 1e-11, mean 1e-9, cov 1e-10 sigma^2,
    prob 1e-10"""
    gap = dict(F=np.max(np.abs(out["F"] - ref["F"])) / np.max(np.abs(ref["F"])),
               log_q=abs(out["log_q"] - ref["log_q"]) / abs(ref["log_q"]),
               mean=np.max(np.abs(out["mean"] - ref["mean"])) / np.max(np.abs(ref["mean"])),
               cov=np.max(np.abs(out["cov"] - ref["cov"])) / SIGMA ** 2,
               prob=np.max(np.abs(out["prob"] - ref["prob"])))
    GAPS[tag] = gap
    print("%s iters %d / %d  " % (tag, out["iters"], ref["iters"]) + "  ".join("%s %.2e" % kv for kv in gap.items()))
    assert out["converged"] and ref["converged"]
    assert abs(out["iters"] - ref["iters"]) <= 1
    assert out["F"].shape == ref["F"].shape
    assert gap["F"] <= 1e-9
    assert gap["log_q"] <= 1e-11
    assert gap["mean"] <= 1e-9
    assert gap["cov"] <= 1e-10
    assert gap["prob"] <= 1e-10


@functools.lru_cache(maxsize=None)
def default_run(ctx, name):
    return gpu_run(ctx, name)


@pytest.mark.parametrize("route", list(ROUTES))
@pytest.mark.parametrize("name", PROBLEMS)
def test_route_matches_the_mirror_and_itself(ctx, name, route):
    ref = reference(name)
    with options(ctx, ROUTES[route]):
        a = gpu_run(ctx, name)
        b = gpu_run(ctx, name)
    hold_to_the_mirror(a, ref, "%s %s" % (name, route))
    assert same_bits(a, b)
    if route in SAME_BITS_AS_DEFAULT:
        assert same_bits(a, default_run(ctx, name))


@pytest.mark.parametrize("name", PROBLEMS)
def test_predict_uses_the_leaves_of_the_resident_factor(ctx, name):
    """fit with panel_fused = 0, switch back to 1, predict -- and the reverse: *_predict_impl solves with factor_fused of
    the resident factor, so the prediction equals, bit for bit, the one taken under the option of the fit"""
    ref = reference(name)
    for fit_with in (0, 1):
        with options(ctx, {"panel_fused": fit_with}):
            log_q, F, iters, conv = gpu_fit(ctx, name)
            want = gpu_predict(ctx, name)
            ctx.set_option("panel_fused", 1 - fit_with)
            got = gpu_predict(ctx, name)
        for u, v in zip(want, got):
            assert np.array_equal(u, v)
        out = dict(F=F, log_q=log_q, iters=iters, converged=conv, mean=got[0], cov=got[1], prob=got[2])
        hold_to_the_mirror(out, ref, "%s fit with panel_fused %d, predicted with %d" % (name, fit_with, 1 - fit_with))
