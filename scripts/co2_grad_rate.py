"""gpmi_lml_grad_co2 (the CO2 composite kernel, kind 3) beside gpmi_lml_grad of a squared-exponential fit of the same N and
d on one MI355X (profiles/r15_co2_grad.txt).

    python scripts/co2_grad_rate.py [--cases 4096x1,16384x1,65536x1,16384x11] [--warmup 1] [--repeats 5] [--limit 900]
                                    [--out FILE] [--once]

One process.  Per case: a kind-3 fit and `repeats` timed calls of its gradient after `warmup`, then a kind-0 fit of the
same inputs and the same for gpmi_lml_grad; median, min and max of the wall time around the call (every call ends with a
synchronisation) and of the stage timer GPMI_T_GRAD (device events around alpha, U = L^-T, -K_y^-1 = -U U^T and the trace
pass).  The two calls share that whole N^3 front, so their difference is the new N^2 pass.  gpmi_lml_grad runs the code
of the parent commit: this change left its launches and its kernels' instructions as they were.  d = 1: the months of
CO2_example.py (x = 1958 + i / 12) with HYPERMS_BOOK; d > 1: inputs uniform in [0, 4)^d / sqrt(d) and a theta whose
kernel_2 is weak (kernel_2 of the Euclidean norm is a valid covariance for d = 1 only).  A case whose matrix is not
positive definite is reported and skipped.  --limit: the process ends itself (with a traceback) after that many seconds.
--once makes one call of each and writes nothing: the run to put under `rocprofv3 --kernel-trace --stats` for the trace
kernels' own times."""
import argparse
import faulthandler
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from gaussian_process_amd import GPContext  # noqa: E402
from gaussian_process_amd.CO2_example import HYPERMS_BOOK, NOISE_VAR  # noqa: E402

THETA_MD = np.array([1.5, 1.2, 0.05, 2.0, 8.0, 0.7, 0.9, 1.3, 0.3, 0.5, 1.0])


def problem(N, d, rng):
    if d == 1:
        X = (1958.0 + np.arange(N) / 12.0).reshape(-1, 1)
        y = 3.0 * np.sin(2 * np.pi * X[:, 0]) + 2.0 * np.sin(X[:, 0] / 5.0) + 0.3 * rng.standard_normal(N)
        return X, y, HYPERMS_BOOK
    X = rng.uniform(0.0, 4.0, size=(N, d)) / np.sqrt(d)
    return X, np.sin(X.sum(1)) + 0.05 * rng.standard_normal(N), THETA_MD


def timed(call, warmup, repeats, timer):
    for _ in range(warmup):
        call()
    wall, stage = [], []
    for _ in range(repeats):
        t = time.perf_counter()
        call()
        wall.append(1e3 * (time.perf_counter() - t))
        stage.append(timer())
    return wall, stage


def stats(ms):
    return "median %9.3f ms (min %.3f, max %.3f)" % (np.median(ms), min(ms), max(ms))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--cases", default="4096x1,16384x1,65536x1,16384x11")
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--limit", type=int, default=900)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r15_co2_grad.txt"))
    ap.add_argument("--once", action="store_true")
    a = ap.parse_args()
    faulthandler.dump_traceback_later(a.limit, exit=True)
    cases = [tuple(int(v) for v in c.split("x")) for c in a.cases.split(",")]
    warmup, repeats = (0, 1) if a.once else (a.warmup, a.repeats)
    rng = np.random.default_rng(0)
    out = ["gpmi_lml_grad_co2 (kind 3) beside gpmi_lml_grad (kind 0) at the same N and d, one MI355X",
           "`python scripts/co2_grad_rate.py --cases %s`: %d warm-up calls, %d timed" % (a.cases, a.warmup, a.repeats), ""]
    with GPContext(0) as ctx:
        grad_ms = lambda: ctx.timers()["grad"]      # noqa: E731
        for N, d in cases:
            X, y, th = problem(N, d, rng)
            tag = "N=%d d=%d" % (N, d)
            try:
                ctx.set_kernel("co2", th)
                lml = ctx.fit(X, y, 1.0, 1.0, NOISE_VAR)
                co2, co2_t = timed(ctx.lml_grad_co2, warmup, repeats, grad_ms)
                g = ctx.lml_grad_co2()
                ctx.set_kernel("rbf")
                ctx.factorize(1.5, 3.0, NOISE_VAR)
                rbf, rbf_t = timed(ctx.lml_grad, warmup, repeats, grad_ms)
            except np.linalg.LinAlgError as e:
                out.append("%s: not positive definite (pivot %s): skipped" % (tag, getattr(e, "bad_pivot", "?")))
                print(out[-1], flush=True)
                continue
            finally:
                ctx.set_kernel("rbf")
            lines = ["%s gpmi_lml_grad_co2  GPMI_T_GRAD %s   wall %s" % (tag, stats(co2_t), stats(co2)),
                     "%s gpmi_lml_grad      GPMI_T_GRAD %s   wall %s" % (tag, stats(rbf_t), stats(rbf)),
                     "%s ratio of the GPMI_T_GRAD medians %.4f, difference %+.3f ms; lower triangle %d elements; "
                     "kind-3 lml %.6f, |d_theta| %.6g, d_noise %.6g"
                     % (tag, np.median(co2_t) / np.median(rbf_t), np.median(co2_t) - np.median(rbf_t),
                        N * (N + 1) // 2, lml, np.linalg.norm(g[0]), g[1]), ""]
            print("\n".join(lines), flush=True)
            out += lines
    if a.once:
        return
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write("\n".join(out) + "\n")


if __name__ == "__main__":
    main()
