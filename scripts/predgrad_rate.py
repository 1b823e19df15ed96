"""gpmi_predict_grad_resident on both routes against gpmi_predict_resident (profiles/r17_predgrad_rate.txt).

    python scripts/predgrad_rate.py [--sizes 4096,16384,65536] [--ns 16,128,1024,4096] [--dim 8] [--repeats 3]
                                    [--out profiles/r17_predgrad_rate.txt]

One child process per size, each under a time limit of its own; the first that fails or runs out of time ends the run.
Per (N, n), behind one fit of N points and with v resident (a prediction precedes, so that GPMI_T_SOLVE_V holds the
route to W alone):

    the wall time of GPContext.predict_grad on the sweep route ("pgrad_sweep" 1) and on the inverse route (0), and of the
    call without dvar, with the timer split alpha / route (GPMI_T_SOLVE_V) / row dots + pass (GPMI_T_MEANVAR);
    the sweep alone: GPMI_T_SOLVE_V of the sweep route (the copy of v and the launch chain) in us per launch (N / 128
    launches) and the bytes of L it streams (the lower triangle once per 16-row group) per second against the
    streaming-read figure of the HBM probe (gpmi_probe_hbm_ex mode 4);
    the pass alone: GPMI_T_MEANVAR less the row dots' time (GPMI_T_MEANVAR of gpmi_predict_resident) against its HBM
    floor of 8 n N bytes (W read once);
    the yardstick: the wall time of gpmi_predict_resident on the same state.

n = 4096 at N = 65536 needs 2 GB for W and as much for V: it runs where the device has the memory.  No time here is a
pass or fail condition."""
import argparse
import os
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIMITS = {4096: 180, 16384: 300, 65536: 540}          # seconds per child


def _data(N, n, d):
    rng = np.random.default_rng(N + n)
    X = rng.uniform(0.0, 4.0, size=(N, d))
    y = np.sin(X.sum(1)) + 0.05 * rng.standard_normal(N)
    return X, y, rng.uniform(0.0, 4.4, size=(n, d))


def _wall(fn):
    t = time.perf_counter()
    fn()
    return (time.perf_counter() - t) * 1e3


def child(N, ns, d, repeats):
    sys.path.insert(0, ROOT)
    from gaussian_process_amd import GPContext
    sig, ell, noise = 1.2, 1.3 * np.sqrt(d), 1e-2
    with GPContext(0) as ctx:
        hbm = max(ctx.probe_hbm_ex(4 << 30, 4, blocks) for blocks in (2048, 4096, 65536))
        print("N=%d HBM streaming read (gpmi_probe_hbm_ex mode 4): %.0f GB/s" % (N, hbm), flush=True)
        X, y, _ = _data(N, 1, d)
        ctx.fit(X, y, sig, ell, noise)
        nblk = (N + 127) // 128
        tri_bytes = nblk * (nblk + 1) // 2 * 128 * 128 * 8
        for n in ns:
            Xs = _data(N, n, d)[2]
            ctx.set_test(Xs)
            ctx.predict_resident()                               # warm-up; v resident from here on
            pred = [_wall(ctx.predict_resident) for _ in range(repeats)]
            dots = ctx.timers()["meanvar"]
            print("N=%d n=%d predict_resident median %.3f ms (min %.3f); row dots %.3f ms" % (N, n, float(np.median(pred)), min(pred), dots),
                  flush=True)
            for label, opt, want in (("sweep", 1, True), ("inverse", 0, True), ("no dvar", -1, False)):
                ctx.set_option("pgrad_sweep", opt)
                ctx.predict_grad(want_var_grad=want)             # warm-up: buffers, code objects
                ms, al, rt, mv = [], [], [], []
                for _ in range(repeats):
                    ms.append(_wall(lambda: ctx.predict_grad(want_var_grad=want)))
                    t = ctx.timers()
                    al.append(t["alpha"]); rt.append(t["solve_v"]); mv.append(t["meanvar"])
                r, p = float(np.median(rt)), max(float(np.median(mv)) - dots, 1e-6)
                line = ("N=%d n=%d predict_grad %-8s median %.3f ms (min %.3f): alpha %.3f  route %.3f  dots + pass %.3f ms"
                        % (N, n, label, float(np.median(ms)), min(ms), float(np.median(al)), r, float(np.median(mv))))
                if want:
                    line += ";  pass alone %.3f ms = %.0f GB/s of W (floor 8 n N = %.3f GB: %.2f of the probe)" % (
                        p, 8.0 * n * N / (p * 1e-3) / 1e9, 8.0 * n * N / 1e9, 8.0 * n * N / (p * 1e-3) / 1e9 / hbm)
                if label == "sweep":
                    groups = (n + 15) // 16
                    line += (";  sweep %.1f us per launch (%d launches, %d row groups), %.2f GB of L: %.0f GB/s = %.2f of the probe"
                             % (r * 1e3 / nblk, nblk, groups, groups * tri_bytes / 1e9, groups * tri_bytes / (r * 1e-3) / 1e9,
                                groups * tri_bytes / (r * 1e-3) / 1e9 / hbm))
                print(line, flush=True)
            ctx.set_option("pgrad_sweep", -1)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="4096,16384,65536")
    ap.add_argument("--ns", default="16,128,1024,4096")
    ap.add_argument("--dim", type=int, default=8)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r17_predgrad_rate.txt"))
    ap.add_argument("--child", action="store_true")
    ap.add_argument("--size", type=int, default=0)
    a = ap.parse_args()
    ns = [int(v) for v in a.ns.split(",")]
    if a.child:
        return child(a.size, ns, a.dim, a.repeats)
    lines = ["gpmi_predict_grad_resident, both routes, against gpmi_predict_resident: scripts/predgrad_rate.py --sizes %s --ns %s "
             "--dim %d --repeats %d" % (a.sizes, a.ns, a.dim, a.repeats),
             "wall ms of the call (one synchronisation inside), v resident; alpha / route / dots + pass: the stage timers "
             "GPMI_T_ALPHA, GPMI_T_SOLVE_V, GPMI_T_MEANVAR"]
    status = 0
    for N in [int(v) for v in a.sizes.split(",")]:
        cmd = [sys.executable, os.path.abspath(__file__), "--child", "--size", str(N), "--ns", a.ns, "--dim", str(a.dim),
               "--repeats", str(a.repeats if N < 65536 else 1)]
        try:
            p = subprocess.run(cmd, capture_output=True, text=True, timeout=LIMITS.get(N, 540))
        except subprocess.TimeoutExpired:
            lines.append("N=%d: time limit" % N)
            status = 124
            break
        lines += p.stdout.splitlines()
        print(p.stdout, flush=True)
        if p.returncode != 0:
            lines.append("N=%d: exit status %d\n%s" % (N, p.returncode, p.stderr[-2000:]))
            status = p.returncode
            break
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        f.write("\n".join(lines) + "\n")
    return status


if __name__ == "__main__":
    sys.exit(main() or 0)
