"""GPMI_T_LOO of gpmi_loo and gpmi_loo_grad against GPMI_T_GRAD of gpmi_lml_grad on one resident factor
(profiles/r08_loo_rate.txt).

    python scripts/loo_rate.py [--sizes 16384] [--dims 8] [--warmup 2] [--repeats 7] [--once]

Per (N, d): warm-up calls, then `repeats` timed calls of each; median, min and max of the stage timer (device events around
the whole device span of the call), the ratios to gpmi_lml_grad beside the flop count's, and the HBM floor of the new N^2
passes.  --once makes one call of each per size and prints nothing but the sizes: the run to put under
`rocprofv3 --kernel-trace --stats` for the kernels' own times."""
import argparse
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from gaussian_process_amd import GPContext  # noqa: E402

HBM_BYTES_PER_S = 8e12


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="16384")
    ap.add_argument("--dims", default="8")
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
                ctx.factorize(1.2, 1.3 * np.sqrt(d), 5e-4)
                if a.once:
                    ctx.lml_grad()
                    ctx.loo()
                    ctx.loo_grad()
                    print("N=%d d=%d: one call of each" % (N, d))
                    continue
                med = {}
                for name, call, slot in (("gpmi_lml_grad", ctx.lml_grad, "grad"), ("gpmi_loo", ctx.loo, "loo"),
                                         ("gpmi_loo_grad", ctx.loo_grad, "loo")):
                    for _ in range(a.warmup):
                        call()
                    ms = []
                    for _ in range(a.repeats):
                        call()
                        ms.append(ctx.timers()[slot])
                    med[name] = float(np.median(ms))
                    print("N=%d d=%d %-14s GPMI_T_%-4s median %.3f ms (min %.3f, max %.3f, %d repeats after %d warm-up)"
                          % (N, d, name, slot.upper(), med[name], min(ms), max(ms), a.repeats, a.warmup))
                base = med["gpmi_lml_grad"]
                print("N=%d d=%d gpmi_loo / gpmi_lml_grad = %.3f (flop count: N^3/3 against 2N^3/3 = 0.5)"
                      % (N, d, med["gpmi_loo"] / base))
                print("N=%d d=%d gpmi_loo_grad / gpmi_lml_grad = %.3f (flop count: 2N^3/3 + 2N^3 against 2N^3/3 = 4)"
                      % (N, d, med["gpmi_loo_grad"] / base))
                # the N^2 passes of gpmi_loo_grad beside the products: kappa reads the upper triangle of U, the mirror reads
                # and writes half of Kn, D is written once and read once, Kn is read once, every NB x N row block of the
                # product is zeroed once, and the row dot reads it and Kn once more
                full = 8.0 * N * N
                for what, nbytes in (("kappa (upper triangle of U)", full / 2), ("mirror Kn (read + write a triangle)", full),
                                     ("D build (write)", full), ("t = D alpha (read D)", full),
                                     ("c, q, Kn t (read Kn)", full), ("row dots (read product and Kn)", 2 * full),
                                     ("workspace zeroing (write)", full)):
                    print("N=%d   HBM floor at 8 TB/s, %-38s %.3f GB -> %.3f ms" % (N, what + ":", nbytes / 1e9,
                                                                                  nbytes / HBM_BYTES_PER_S * 1e3))


if __name__ == "__main__":
    main()
