"""gpmi_laplace_grad against gpmi_lml_grad_ard and gpmi_factorize on one MI355X (profiles/r12_laplace_grad.txt).

    python scripts/laplace_grad_rate.py [--N 16384] [--d 8] [--warmup 2] [--repeats 7] [--limit 300] [--out FILE] [--once]

One process: a regression factorisation and its ARD gradient, then a Laplace fit (tol = 1e-13) of two-blob labels on the
same inputs and lengthscales and its gradient.  Per call: warm-up calls, then `repeats` timed ones; median, min and max
of the wall time around the call (every call ends with a synchronisation) and, for the two gradients, of the stage timer
GPMI_T_GRAD (device events around U = L^-T, -U U^T and the passes behind them).  The regression calls run the code of the
parent commit: this change left their launches and their kernels' instructions as they were.  --limit: the process ends
itself (with a traceback) after that many seconds, whatever it is waiting for.  --once makes one call of each and
writes nothing: the run to put under `rocprofv3 --kernel-trace --stats` for the kernels' own times."""
import argparse
import faulthandler
import os
import sys
import time

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
    return "%-22s median %8.3f ms (min %.3f, max %.3f)" % (name, np.median(ms), min(ms), max(ms))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--N", type=int, default=16384)
    ap.add_argument("--d", type=int, default=8)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--limit", type=int, default=300)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r12_laplace_grad.txt"))
    ap.add_argument("--once", action="store_true")
    a = ap.parse_args()
    faulthandler.dump_traceback_later(a.limit, exit=True)
    N, d = a.N, a.d
    rng = np.random.default_rng(0)
    lab = np.where(rng.random(N) < 0.5, -1.0, 1.0)
    X = rng.standard_normal((N, d)) * 1.5 + lab[:, None] / np.sqrt(d)
    y = np.sin(X.sum(1)) + 0.05 * rng.standard_normal(N)
    r = rng.uniform(0.6, 1.8, d)
    sigma, l, noise = 1.5, 3.0, 5e-4
    warmup, repeats = (0, 1) if a.once else (a.warmup, a.repeats)
    out = []
    with GPContext(0) as ctx:
        grad_ms = lambda: ctx.timers()["grad"]      # noqa: E731
        ctx.set_train(X, y)
        ctx.set_lengthscales(r)
        fac, _ = timed(lambda: ctx.factorize(sigma, l, noise), warmup, repeats)
        ard, ard_t = timed(ctx.lml_grad_ard, warmup, repeats, grad_ms)
        fit = ctx.laplace_fit(X, lab, sigma, l, tol=1e-13, lengthscales=r)
        lap, lap_t = timed(ctx.laplace_grad, warmup, repeats, grad_ms)
        g = ctx.laplace_grad()
    if a.once:
        print("N=%d d=%d: one call of each" % (N, d))
        return
    out.append("gpmi_laplace_grad against gpmi_lml_grad_ard and gpmi_factorize, one MI355X, N = %d, d = %d" % (N, d))
    out.append("`python scripts/laplace_grad_rate.py`: %d warm-up calls, %d timed; lengthscales set; the Laplace fit took %d "
               "Newton steps (tol 1e-13, converged %s), log q = %.6f" % (a.warmup, a.repeats, fit[2], fit[3], fit[0]))
    out.append("")
    out.append("wall time around the call:")
    out.append("  " + line("gpmi_factorize", fac))
    out.append("  " + line("gpmi_lml_grad_ard", ard))
    out.append("  " + line("gpmi_laplace_grad", lap))
    out.append("stage timer GPMI_T_GRAD:")
    out.append("  " + line("gpmi_lml_grad_ard", ard_t))
    out.append("  " + line("gpmi_laplace_grad", lap_t))
    out.append("")
    out.append("ratios of the medians: gpmi_laplace_grad / gpmi_lml_grad_ard = %.3f (wall), %.3f (GPMI_T_GRAD); "
               "gpmi_laplace_grad / gpmi_factorize = %.3f (wall)"
               % (np.median(lap) / np.median(ard), np.median(lap_t) / np.median(ard_t), np.median(lap) / np.median(fac)))
    out.append("gradient: d_l = %.9g, d_sigma = %.9g, |d_r| = %.9g" % (g[1], g[2], np.linalg.norm(g[0])))
    text = "\n".join(out) + "\n"
    sys.stdout.write(text)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(text)


if __name__ == "__main__":
    main()
