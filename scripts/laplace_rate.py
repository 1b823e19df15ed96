"""Cost of one Newton iteration of the Laplace classifier against one regression factorisation, same process, same
sizes (d = 8).  One iteration = laplace_fit(max_iter=2) - laplace_fit(max_iter=1): a K build, f = K a, the Newton
pass, the fused u = K b / B pass, the Cholesky of B with the right-hand side riding, the backward solve and the update.

    python scripts/laplace_rate.py [--sizes 4096,16384,65536] [--reps 3]

Prints one JSON line per size: ms per iteration, ms per gpmi_factorize (K build + Cholesky + LML), their ratio, and the
algorithmic bytes of the two matrix-vector passes (the lower triangle read; read and written) for rocprofv3 stats."""
import argparse
import json
import os
import sys
import time
import warnings

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from gaussian_process_amd import GPContext  # noqa: E402


def timed(fn, reps):
    best = float("inf")
    for _ in range(reps):
        t = time.perf_counter()
        fn()
        best = min(best, time.perf_counter() - t)
    return best * 1e3


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="4096,16384,65536")
    ap.add_argument("--reps", type=int, default=3)
    args = ap.parse_args()
    warnings.simplefilter("ignore", RuntimeWarning)
    with GPContext(0) as ctx:
        for N in (int(s) for s in args.sizes.split(",")):
            rng = np.random.default_rng(N)
            y = np.where(rng.random(N) < 0.5, -1.0, 1.0)
            X = rng.standard_normal((N, 8)) + 0.5 * y[:, None]
            sigma, ell = 1.5, 3.0
            ctx.set_train(X, y)
            ctx.laplace_fit(X, y, sigma, ell, max_iter=1)                 # warm-up: allocations, code objects
            t1 = timed(lambda: ctx.laplace_fit(X, y, sigma, ell, max_iter=1), args.reps)
            t2 = timed(lambda: ctx.laplace_fit(X, y, sigma, ell, max_iter=2), args.reps)
            ctx.set_train(X, y)
            ctx.factorize(sigma, ell, 1e-3)
            tf = timed(lambda: ctx.factorize(sigma, ell, 1e-3), args.reps)
            Np = -(-N // 128) * 128
            tri = Np * (Np + 128) // 2 * 8
            print(json.dumps({"N": N, "d": 8, "iteration_ms": round(t2 - t1, 3), "factorize_ms": round(tf, 3),
                              "ratio": round((t2 - t1) / tf, 4), "fit_max_iter1_ms": round(t1, 3),
                              "fit_max_iter2_ms": round(t2, 3), "symv_bytes": tri, "symv_scale_bytes": 2 * tri}),
                  flush=True)


if __name__ == "__main__":
    main()
