"""The Matern kinds against the squared exponential in one process (profiles/r11_matern_rate.txt).

    python scripts/matern_rate.py [--size 16384] [--dim 8] [--warmup 1] [--repeats 3]

For kinds 0 (rbf), 4, 5 and 6 (Matern nu = 1/2, 3/2, 5/2) at one (N, d): after the warm-up calls, the median of
`repeats` runs of
  - the K build alone (the GPMI_T_KBUILD stage timer of a factorize: device events around the symmetric build),
  - a whole factorize (wall clock around the call: K build, Cholesky, forward solve, LML, one synchronisation),
  - lml_grad_ard (the GPMI_T_GRAD stage timer: alpha, U = L^-T, -K_y^-1 = -U U^T and the fused d + 3 trace pass).
Kind 0 runs the code it always ran, so it is the yardstick: every Matern figure is also given as a ratio to kind 0 in
the same run.  The K build writes the lower tiles only; its share of the HBM write peak is not computed here."""
import argparse
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from gaussian_process_amd import GPContext  # noqa: E402

KINDS = ("rbf", "matern12", "matern32", "matern52")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--size", type=int, default=16384)
    ap.add_argument("--dim", type=int, default=8)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--repeats", type=int, default=3)
    a = ap.parse_args()
    N, d = a.size, a.dim
    rng = np.random.default_rng(0)
    X = rng.uniform(0.0, 4.0, size=(N, d))
    y = np.sin(X.sum(1)) + 0.05 * rng.standard_normal(N)
    sigma, l, noise = 1.2, 1.3 * np.sqrt(d), 5e-4
    res = {}
    with GPContext(0) as ctx:
        ctx.set_option("timing", 1)
        for kind in KINDS:
            ctx.set_kernel(kind)
            ctx.set_train(X, y)
            kb, fit, grad = [], [], []
            for i in range(a.warmup + a.repeats):
                t0 = time.perf_counter()
                lml = ctx.factorize(sigma, l, noise)
                t1 = time.perf_counter()
                k = ctx.timers()["kbuild"]
                ctx.lml_grad_ard()
                g = ctx.timers()["grad"]
                if i >= a.warmup:
                    kb.append(k)
                    fit.append(1e3 * (t1 - t0))
                    grad.append(g)
            res[kind] = (float(np.median(kb)), float(np.median(fit)), float(np.median(grad)), lml)
        ctx.set_kernel("rbf")
    print("N=%d d=%d sigma=%g l=%g noise=%g: medians of %d runs after %d warm-up, ms (ratio to rbf in the same run)"
          % (N, d, sigma, l, noise, a.repeats, a.warmup))
    print("%-9s %22s %22s %22s   %s" % ("kind", "K build (T_KBUILD)", "factorize (wall)", "lml_grad_ard (T_GRAD)", "lml"))
    base = res["rbf"]
    for kind in KINDS:
        kbm, fm, gm, lml = res[kind]
        print("%-9s %12.3f (%5.2fx) %13.3f (%5.2fx) %13.3f (%5.2fx)   %.6f"
              % (kind, kbm, kbm / base[0], fm, fm / base[1], gm, gm / base[2], lml))


if __name__ == "__main__":
    main()
