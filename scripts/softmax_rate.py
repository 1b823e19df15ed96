"""Cost of one Newton iteration of the softmax (multi-class Laplace) classifier against one regression factorisation,
same process, same sizes (d = 8).  One iteration = softmax_fit(max_iter=2) - softmax_fit(max_iter=1): F = A K, the Newton
pass, C x [B_c from K, its Cholesky, the triangular sweep S_c L_c^-T, the lower NT GEMM that forms E_c], K B and the
E_c products, the Cholesky of sum_c E_c with the right-hand side riding, the backward solve and the update.  By flop
count that is 3 C + 1 factorisations.

    python scripts/softmax_rate.py [--cases 4096:3,16384:3,65536:3,16384:10] [--reps 3]

Prints one JSON line per case: ms per iteration, ms per gpmi_factorize (K build + Cholesky + LML), their ratio beside
3 C + 1, and the algorithmic bytes of one pass over a lower triangle for the rocprofv3 stats of the symv launches."""
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
    ap.add_argument("--cases", default="4096:3,16384:3,65536:3,16384:10", help="N:C,...")
    ap.add_argument("--reps", type=int, default=3)
    args = ap.parse_args()
    warnings.simplefilter("ignore", RuntimeWarning)
    with GPContext(0) as ctx:
        for N, C in (tuple(int(v) for v in s.split(":")) for s in args.cases.split(",")):
            rng = np.random.default_rng(N + C)
            lab = rng.integers(0, C, N)
            X = rng.standard_normal((C, 8))[lab] * 0.7 + rng.standard_normal((N, 8))
            sigma, ell = 1.5, 3.0
            ctx.softmax_fit(X, lab, C, sigma, ell, max_iter=1)            # warm-up: allocations, code objects
            t1 = timed(lambda: ctx.softmax_fit(X, lab, C, sigma, ell, max_iter=1), args.reps)
            t2 = timed(lambda: ctx.softmax_fit(X, lab, C, sigma, ell, max_iter=2), args.reps)
            ctx.set_train(X, lab.astype(np.float64))
            ctx.factorize(sigma, ell, 1e-3)
            tf = timed(lambda: ctx.factorize(sigma, ell, 1e-3), args.reps)
            Np = -(-N // 128) * 128
            print(json.dumps({"N": N, "C": C, "d": 8, "iteration_ms": round(t2 - t1, 3), "factorize_ms": round(tf, 3),
                              "ratio": round((t2 - t1) / tf, 3), "flop_ratio_3C_plus_1": 3 * C + 1,
                              "fit_max_iter1_ms": round(t1, 3), "fit_max_iter2_ms": round(t2, 3),
                              "lower_triangle_bytes": Np * (Np + 128) // 2 * 8}), flush=True)


if __name__ == "__main__":
    main()
