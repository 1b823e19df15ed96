"""gpmi_softmax_grad against gpmi_factorize and one Newton step of gpmi_softmax_fit on one MI355X
(profiles/r13_softmax_grad.txt).

    python scripts/softmax_grad_rate.py [--N 16384] [--d 8] [--classes 3,10] [--warmup 1] [--repeats 3] [--limit 900]
                                        [--out FILE] [--once]

One process.  Per number of classes: a regression factorisation of the same inputs and lengthscales, softmax fits with
max_iter = 1 and max_iter = 2 (their difference is one whole Newton step: C factorisations, sweeps and products, the
factorisation of sum_c E_c and the matrix-vector chain), the fit at tol = 1e-13 and its gradient.  Per call: warm-up
calls, then `repeats` timed ones; median, min and max of the wall time around the call (every call ends with a
synchronisation) and, for the gradient, of the stage timer GPMI_T_GRAD.  --limit: the process ends itself (with a
traceback) after that many seconds, whatever it is waiting for.  --once makes one fit and one gradient per class count
and writes nothing: the run to put under `rocprofv3 --kernel-trace --stats` for the kernels' own times."""
import argparse
import faulthandler
import os
import sys
import time
import warnings

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from gaussian_process_amd import GPContext  # noqa: E402


def timed(call, warmup, repeats, timer=None):
    for _ in range(warmup):
        call()
    wall, stage = [], []
    for _ in range(repeats):
        t = time.perf_counter()
        call()
        wall.append(1e3 * (time.perf_counter() - t))
        if timer:
            stage.append(timer())
    return wall, stage


def line(name, ms):
    return "%-26s median %9.3f ms (min %.3f, max %.3f)" % (name, np.median(ms), min(ms), max(ms))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--N", type=int, default=16384)
    ap.add_argument("--d", type=int, default=8)
    ap.add_argument("--classes", default="3,10")
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--limit", type=int, default=900)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r13_softmax_grad.txt"))
    ap.add_argument("--once", action="store_true")
    a = ap.parse_args()
    faulthandler.dump_traceback_later(a.limit, exit=True)
    N, d = a.N, a.d
    warmup, repeats = (0, 1) if a.once else (a.warmup, a.repeats)
    sigma, l, noise = 1.5, 3.0, 5e-4
    out = ["gpmi_softmax_grad against gpmi_factorize and one Newton step of gpmi_softmax_fit, one MI355X, N = %d, d = %d" % (N, d),
           "`python scripts/softmax_grad_rate.py`: %d warm-up calls, %d timed; lengthscales set" % (a.warmup, a.repeats)]
    warnings.simplefilter("ignore", RuntimeWarning)          # the fits with max_iter = 1, 2 are not meant to converge
    with GPContext(0) as ctx:
        grad_ms = lambda: ctx.timers()["grad"]      # noqa: E731
        for C in [int(x) for x in a.classes.split(",")]:
            rng = np.random.default_rng(C)
            cen = rng.standard_normal((C, d)) * 2.0
            lab = rng.integers(0, C, N)
            X = cen[lab] + rng.standard_normal((N, d)) * 1.2
            y = np.sin(X.sum(1)) + 0.05 * rng.standard_normal(N)
            r = rng.uniform(0.6, 1.8, d)
            if a.once:
                ctx.softmax_fit(X, lab, C, sigma, l, tol=1e-13, lengthscales=r)
                ctx.softmax_grad()
                print("N=%d d=%d C=%d: one fit and one gradient" % (N, d, C))
                continue
            ctx.set_train(X, y)
            ctx.set_lengthscales(r)
            fac, _ = timed(lambda: ctx.factorize(sigma, l, noise), warmup, repeats)
            fit1, _ = timed(lambda: ctx.softmax_fit(X, lab, C, sigma, l, max_iter=1, lengthscales=r), warmup, repeats)
            fit2, _ = timed(lambda: ctx.softmax_fit(X, lab, C, sigma, l, max_iter=2, lengthscales=r), warmup, repeats)
            t = time.perf_counter()
            fit = ctx.softmax_fit(X, lab, C, sigma, l, tol=1e-13, lengthscales=r)
            fit_ms = 1e3 * (time.perf_counter() - t)
            grd, grd_t = timed(ctx.softmax_grad, warmup, repeats, grad_ms)
            g = ctx.softmax_grad()
            step = np.median(fit2) - np.median(fit1)
            out.append("")
            out.append("C = %d: the fit at tol 1e-13 took %d Newton steps (converged %s) and %.1f ms, log q = %.6f"
                       % (C, fit[2], fit[3], fit_ms, fit[0]))
            out.append("wall time around the call:")
            out.append("  " + line("gpmi_factorize", fac))
            out.append("  " + line("gpmi_softmax_fit max_iter=1", fit1))
            out.append("  " + line("gpmi_softmax_fit max_iter=2", fit2))
            out.append("  one Newton step (difference of the medians) %9.3f ms" % step)
            out.append("  " + line("gpmi_softmax_grad", grd))
            out.append("stage timer GPMI_T_GRAD:")
            out.append("  " + line("gpmi_softmax_grad", grd_t))
            out.append("ratios of the medians (wall): gpmi_softmax_grad / gpmi_factorize = %.2f; gpmi_softmax_grad / one "
                       "Newton step = %.2f (flop count 15 C / (3 C + 1) = %.2f)"
                       % (np.median(grd) / np.median(fac), np.median(grd) / step, 15.0 * C / (3 * C + 1)))
            out.append("5 C N^3 flops / GPMI_T_GRAD = %.1f Tflop/s; (3 C + 1) N^3 / 3 flops / Newton step = %.1f Tflop/s; "
                       "N^3 / 3 flops / gpmi_factorize = %.1f Tflop/s"
                       % (5.0 * C * N ** 3 / np.median(grd_t) * 1e-9, (3 * C + 1) * N ** 3 / 3.0 / step * 1e-9,
                          N ** 3 / 3.0 / np.median(fac) * 1e-9))
            out.append("gradient: d_l = %.9g, d_sigma = %.9g, |d_r| = %.9g" % (g[1], g[2], np.linalg.norm(g[0])))
    if a.once:
        return
    text = "\n".join(out) + "\n"
    sys.stdout.write(text)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(text)


if __name__ == "__main__":
    main()
