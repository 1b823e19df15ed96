"""GPMI_T_GRAD of gpmi_lml_grad_ard against gpmi_lml_grad on one resident factor (profiles/r07_ard_grad.txt).

    python scripts/ard_grad_rate.py [--sizes 16384] [--dims 8,16] [--warmup 2] [--repeats 7] [--once]

Per (N, d): warm-up calls, then `repeats` timed calls of each gradient; median, min and max of the stage timer (device
events around alpha, U = L^-T, -K_y^-1 = -U U^T and the fused trace pass).  --once makes one call of each per size and
prints nothing but the sizes: the run to put under `rocprofv3 --kernel-trace --stats` for the kernels' own times."""
import argparse
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from gaussian_process_amd import GPContext  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="16384")
    ap.add_argument("--dims", default="8,16")
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--once", action="store_true")
    a = ap.parse_args()
    rng = np.random.default_rng(0)
    with GPContext(0) as ctx:
        for N in [int(v) for v in a.sizes.split(",")]:
            for d in [int(v) for v in a.dims.split(",")]:
                X = rng.uniform(0.0, 4.0, size=(N, d))
                y = np.sin(X.sum(1)) + 0.05 * rng.standard_normal(N)
                ctx.set_train(X, y)
                ctx.set_lengthscales(rng.uniform(0.5, 3.0, d) * np.sqrt(d))
                ctx.factorize(1.2, 1.3, 5e-4)
                lower = N * (N + 1) // 2
                if a.once:
                    ctx.lml_grad()
                    ctx.lml_grad_ard()
                    print("N=%d d=%d: one call of each" % (N, d))
                    continue
                for name, call in (("gpmi_lml_grad", ctx.lml_grad), ("gpmi_lml_grad_ard", ctx.lml_grad_ard)):
                    for _ in range(a.warmup):
                        call()
                    ms = []
                    for _ in range(a.repeats):
                        call()
                        ms.append(ctx.timers()["grad"])
                    print("N=%d d=%d %-18s GPMI_T_GRAD median %.3f ms (min %.3f, max %.3f, %d repeats after %d warm-up)"
                          % (N, d, name, np.median(ms), min(ms), max(ms), a.repeats, a.warmup))
                print("N=%d: HBM-read floor of one pass over the lower triangle: %.3f GB (8 B x %d elements)"
                      % (N, 8 * lower / 1e9, lower))
            ctx.set_lengthscales(None)


if __name__ == "__main__":
    main()
