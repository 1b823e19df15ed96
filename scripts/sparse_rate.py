"""Rates of sparse GP regression with inducing points (profiles/r09_sparse_rate.txt, profiles/r10_sparse_grad.txt).

    python scripts/sparse_rate.py gram       [--m 1024,4096,8192] [--slab 16384] [--repeats 5]
    python scripts/sparse_rate.py fit        [--N 1048576] [--d 8] [--m 4096] [--n 4096] [--repeats 2]
    python scripts/sparse_rate.py crossover  [--m 2048] [--sizes 16384,65536] [--repeats 3]
    python scripts/sparse_rate.py grad       [--N 262144] [--d 8] [--m 2048] [--repeats 3]

gram:      the Gram accumulation alone (gpmi_probe_gram: B_lower += V^T V, split launch + reduction) against
           gpmi_probe_gemm(M = m, N = m, K = S, lower = 1), the NT route on the same flop count; TF/s on S m^2 flops.
fit:       sparse_fit + sparse_predict of n test points: seconds, TF/s on 2 N m^2 + 2 m^3 / 3 flops, the stage timers and
           the peak device memory (hipMemGetInfo through torch, read after the calls: the workspaces stay allocated).
crossover: sparse_fit with m inducing points against gpmi_factorize on the same training set.
grad:      gpmi_sparse_grad against gpmi_sparse_fit on the same resident training set (device spans, GPMI_T_SPARSE), the
           gradient's stage split, and the bytes per second of its contraction spans -- the reads of W and E, and the same
           with the write and the read of the chunks' partial sums -- against the streaming-read probe.
One process, one call after the other; every timed call is preceded by a warm-up call."""
import argparse
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from gaussian_process_amd import GPContext, choose_inducing  # noqa: E402


def problem(N, d, seed=0):
    rng = np.random.default_rng(seed)
    X = rng.uniform(0.0, 4.0, size=(N, d))
    y = np.sin(X.sum(1)) + 0.05 * rng.standard_normal(N)
    return X, y


def used_bytes():
    import torch
    free, total = torch.cuda.mem_get_info(0)
    return total - free


def gram(ctx, a):
    S = a.slab
    for m in [int(v) for v in a.m.split(",")]:
        tf, ms = ctx.probe_gram(S, m, reps=a.repeats)
        tfg, msg = ctx.probe_gemm(m, m, S, lower=1, variant=32, reps=a.repeats)
        alg = float(S) * m * m
        print("gram S=%d m=%d: TN split kernel + reduction %.3f ms = %.2f TF/s on S m^2 (%.2f on its tiles) | NT route "
              "probe_gemm(M=m, N=m, K=S, lower=1) %.3f ms = %.2f TF/s on S m^2 (%.2f on its tiles) | ratio %.3f"
              % (S, m, ms, alg / ms / 1e9, tf, msg, alg / msg / 1e9, tfg, msg / ms), flush=True)


def fit(ctx, a):
    X, y = problem(a.N, a.d)
    Z = choose_inducing(X, a.m, seed=1)
    Xs = np.random.default_rng(5).uniform(0.0, 4.0, size=(a.n, a.d))
    l = 1.3 * np.sqrt(a.d)
    base = used_bytes()
    for rep in range(a.repeats):
        t0 = time.perf_counter()
        val = ctx.sparse_fit(X, y, Z, 1.2, l, 5e-4, method=a.method)
        t1 = time.perf_counter()
        tm = ctx.timers()
        mu, sd = ctx.sparse_predict(Xs)
        t2 = time.perf_counter()
        flops = 2.0 * a.N * a.m ** 2 + 2.0 * a.m ** 3 / 3
        print("fit N=%d d=%d m=%d %s run %d: sparse_fit %.3f s wall (upload of X included), device span %.3f s = %.2f TF/s "
              "on 2 N m^2 + 2 m^3 / 3; sparse_predict of %d points %.3f s; value %.6e, finite mean %s"
              % (a.N, a.d, a.m, a.method, rep, t1 - t0, tm["sparse"] / 1e3, flops / tm["sparse"] / 1e9, a.n, t2 - t1, val,
                 bool(np.all(np.isfinite(mu)) and np.all(np.isfinite(sd)))), flush=True)
        print("    split of the device span (ms): cross build %.1f, sweep through L %.1f, row pass + g %.1f, Gram %.1f, "
              "the two factorisations %.1f; sum %.1f of %.1f"
              % (tm["ks"], tm["solve_v"], tm["meanvar"], tm["postchol"], tm["chol"],
                 tm["ks"] + tm["solve_v"] + tm["meanvar"] + tm["postchol"] + tm["chol"], tm["sparse"]), flush=True)
    print("    device memory in use after the calls: %.2f GB (%.2f GB before the first fit)" % (used_bytes() / 1e9, base / 1e9),
          flush=True)


def crossover(ctx, a):
    for N in [int(v) for v in a.sizes.split(",")]:
        X, y = problem(N, a.d)
        Z = choose_inducing(X, a.m, seed=1)
        l = 1.3 * np.sqrt(a.d)
        ctx.set_train(X, y)
        sp, ex = [], []
        for rep in range(a.repeats + 1):
            ctx.sparse_fit(X, y, Z, 1.2, l, 5e-4)
            sp.append(ctx.timers()["sparse"])
            t0 = time.perf_counter()
            ctx.factorize(1.2, l, 5e-4)
            ex.append((time.perf_counter() - t0) * 1e3)
        sp, ex = sp[1:], ex[1:]
        print("crossover N=%d d=%d m=%d: sparse_fit device span median %.2f ms (min %.2f) | gpmi_factorize wall median "
              "%.2f ms (min %.2f) | exact / sparse %.2f" % (N, a.d, a.m, np.median(sp), min(sp), np.median(ex), min(ex),
                                                            np.median(ex) / np.median(sp)), flush=True)


def grad(ctx, a):
    X, y = problem(a.N, a.d)
    Z = choose_inducing(X, a.m, seed=1)
    l = 1.3 * np.sqrt(a.d)
    hbm = max(ctx.probe_hbm_ex(1 << 30, 4, blocks) for blocks in (2048, 4096, 65536))
    ctx.set_train(X, y)
    keys = ("sparse", "chol", "ks", "solve_v", "postchol", "meanvar")
    fits, grads, walls = [], [], []
    for rep in range(a.repeats + 1):
        val = ctx.sparse_fit_resident(Z, 1.2, l, 5e-4)
        fits.append(ctx.timers())
        t0 = time.perf_counter()
        g = ctx.sparse_grad()
        walls.append((time.perf_counter() - t0) * 1e3)
        grads.append(ctx.timers())
    fits, grads, walls = fits[1:], grads[1:], walls[1:]              # the first pair is the warm-up (and the allocations)
    f = {k: float(np.median([t[k] for t in fits])) for k in keys}
    t = {k: float(np.median([t[k] for t in grads])) for k in keys}
    mp = -(-a.m // 128) * 128
    chunks = -(-a.m // 128) + sum(-(-min(16384, a.N - r0) // 128) for r0 in range(0, a.N, 16384))
    main = 16.0 * (a.N + a.m) * mp
    part = 16.0 * chunks * (2 * a.d + 1) * mp
    finite = bool(np.isfinite(g["l"]) and np.isfinite(g["sigma"]) and np.isfinite(g["noise"]) and np.all(np.isfinite(g["r"]))
                  and np.all(np.isfinite(g["Z"])))
    print("grad N=%d d=%d m=%d (%d timed pairs, medians): gpmi_sparse_fit device span %.2f ms (min %.2f) | gpmi_sparse_grad "
          "device span %.2f ms (min %.2f), wall %.2f ms | grad / fit %.3f; bound %.6e, finite gradient %s"
          % (a.N, a.d, a.m, a.repeats, f["sparse"], min(x["sparse"] for x in fits), t["sparse"],
             min(x["sparse"] for x in grads), float(np.median(walls)), t["sparse"] / f["sparse"], val, finite), flush=True)
    print("    split of the fit's span (ms): cross build %.2f, sweep through L %.2f, row pass + g %.2f, Gram %.2f, the two "
          "factorisations %.2f" % (f["ks"], f["solve_v"], f["meanvar"], f["postchol"], f["chol"]), flush=True)
    print("    split of the gradient's span (ms): the m-sized part %.2f, covariance builds %.2f, beta %.2f, E = W T %.2f "
          "(%.2f TF/s on 2 N m_p^2), contractions %.2f; sum %.2f of %.2f"
          % (t["chol"], t["ks"], t["solve_v"], t["postchol"], 2.0 * a.N * mp * mp / t["postchol"] / 1e9, t["meanvar"],
             t["chol"] + t["ks"] + t["solve_v"] + t["postchol"] + t["meanvar"], t["sparse"]), flush=True)
    print("    contraction spans (kernel + the chunks' fixed-order sum): %.3f GB of W and E in %.2f ms = %.0f GB/s, with the "
          "partial sums' write and read (%.3f GB) %.0f GB/s | streaming-read probe %.0f GB/s"
          % (main / 1e9, t["meanvar"], main / t["meanvar"] / 1e6, part / 1e9, (main + part) / t["meanvar"] / 1e6, hbm),
          flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("what", choices=["gram", "fit", "crossover", "grad"])
    ap.add_argument("--m", default=None)
    ap.add_argument("--slab", type=int, default=16384)
    ap.add_argument("--N", type=int, default=None)
    ap.add_argument("--d", type=int, default=8)
    ap.add_argument("--n", type=int, default=4096)
    ap.add_argument("--sizes", default="16384,65536")
    ap.add_argument("--method", default="vfe")
    ap.add_argument("--repeats", type=int, default=None)
    a = ap.parse_args()
    with GPContext(0) as ctx:
        if a.what == "gram":
            a.m = a.m or "1024,4096,8192"
            a.repeats = a.repeats or 5
            gram(ctx, a)
        elif a.what == "grad":
            a.m = int(a.m or 2048)
            a.N = a.N or 262144
            a.repeats = a.repeats or 3
            grad(ctx, a)
        elif a.what == "fit":
            a.N = a.N or 1048576
            a.m = int(a.m or 4096)
            a.repeats = a.repeats or 2
            fit(ctx, a)
        else:
            a.m = int(a.m or 2048)
            a.repeats = a.repeats or 3
            crossover(ctx, a)


if __name__ == "__main__":
    main()
