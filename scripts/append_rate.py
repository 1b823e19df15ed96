"""gpmi_append against a refit (profiles/r14_append_rate.txt).

    python scripts/append_rate.py [--sizes 4096,16384,65536] [--ks 1,16,128,1024] [--dim 8] [--repeats 3]
                                  [--out profiles/r14_append_rate.txt] [--parent-root DIR]

One child process per size, each under a time limit of its own; the first that fails or runs out of time ends the run.
Per (N, k): the wall time of GPContext.append (the call ends with its one synchronisation) behind a fit of N points --
for k <= 16 on both routes (option "append_skinny" 1 / 0), and each once reallocating (reserve 0: every N here is a
multiple of 128, so one more point does not fit) and once in place (option "reserve" = k) -- beside the wall time of
gpmi_factorize of the N + k points in the same process; the sweep's stage timer (GPMI_T_SOLVE_V) as bytes of L per second
against the streaming-read figure of the HBM probe that `bench.py --full` reports; and per size gpmi_factorize of the
N points with "reserve" 0 and 1024 (the reserve widens the leading dimension and adds rows nothing computes on).
--parent-root: a checkout of the parent commit with its library built; gpmi_factorize of the same sizes is then timed
there too (a child per size)."""
import argparse
import os
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIMITS = {4096: 180, 16384: 240, 65536: 480}          # seconds per child


def _data(N, d):
    rng = np.random.default_rng(N)
    X = rng.uniform(0.0, 4.0, size=(N, d))
    y = np.sin(X.sum(1)) + 0.05 * rng.standard_normal(N)
    return X, y


def _wall(fn):
    t = time.perf_counter()
    fn()
    return (time.perf_counter() - t) * 1e3


def child_factorize(root, N, ks, d, repeats):
    """gpmi_factorize of N + k points from the tree at `root` (this one or the parent's)"""
    sys.path.insert(0, root)
    from gaussian_process_amd import GPContext
    X, y = _data(N + max(ks), d)
    with GPContext(0) as ctx:
        for k in ks:
            ctx.set_train(X[:N + k], y[:N + k])
            ctx.factorize(1.2, 1.3 * np.sqrt(d), 1e-2)
            ms = [_wall(lambda: ctx.factorize(1.2, 1.3 * np.sqrt(d), 1e-2)) for _ in range(repeats)]
            print("N=%d k=%d factorize(N+k) median %.3f ms (min %.3f, %d repeats)" % (N, k, float(np.median(ms)), min(ms), repeats),
                  flush=True)


def child_append(N, ks, d, repeats):
    sys.path.insert(0, ROOT)
    from gaussian_process_amd import GPContext
    X, y = _data(N + max(ks), d)
    sig, ell, noise = 1.2, 1.3 * np.sqrt(d), 1e-2
    with GPContext(0) as ctx:
        hbm = max(ctx.probe_hbm_ex(4 << 30, 4, blocks) for blocks in (2048, 4096, 65536))
        print("N=%d HBM streaming read (the probe of bench.py --full): %.0f GB/s" % (N, hbm), flush=True)
        nblk = N // 128
        sweep_bytes = nblk * (nblk + 1) // 2 * 128 * 128 * 8
        for k in ks:
            for route in ((1, 0) if k <= 16 else (0,)):
                for reserve in (0, k):
                    ctx.set_option("append_skinny", route)
                    ctx.set_option("reserve", reserve)
                    ms, sweep, ks_ms, chol = [], [], [], []
                    for _ in range(repeats + 1):              # the first is the warm-up
                        ctx.set_train(X[:N], y[:N])
                        ctx.factorize(sig, ell, noise)
                        before = ctx.layout()
                        ms.append(_wall(lambda: ctx.append(X[N:N + k], y[N:N + k])))
                        t = ctx.timers()
                        sweep.append(t["solve_v"]); ks_ms.append(t["ks"]); chol.append(t["chol"])
                        moved = ctx.layout()["ld"] != before["ld"]
                    ms, sweep, ks_ms, chol = ms[1:], sweep[1:], ks_ms[1:], chol[1:]
                    s = float(np.median(sweep))
                    print("N=%d k=%d append %-7s %-10s median %.3f ms (min %.3f)  build %.3f  sweep %.3f  border %.3f ms;  "
                          "sweep reads %.2f GB of L: %.0f GB/s = %.2f of the probe"
                          % (N, k, "skinny" if route else "padded", "realloc" if moved else "in place", float(np.median(ms)), min(ms),
                             float(np.median(ks_ms)), s, float(np.median(chol)), sweep_bytes / 1e9, sweep_bytes / (s * 1e-3) / 1e9,
                             sweep_bytes / (s * 1e-3) / 1e9 / hbm), flush=True)
            ctx.set_option("reserve", 0)
            ctx.set_train(X[:N + k], y[:N + k])
            ctx.factorize(sig, ell, noise)
            ref = [_wall(lambda: ctx.factorize(sig, ell, noise)) for _ in range(repeats)]
            print("N=%d k=%d factorize(N+k) median %.3f ms (min %.3f, %d repeats), this build" % (N, k, float(np.median(ref)), min(ref), repeats),
                  flush=True)
        # what the reserve costs a fit: the same factorisation of N points with A laid out for N + 1024
        ctx.set_train(X[:N], y[:N])
        for reserve in (0, 1024):
            ctx.set_option("reserve", reserve)
            ctx.factorize(sig, ell, noise)
            ref = [_wall(lambda: ctx.factorize(sig, ell, noise)) for _ in range(repeats)]
            lay = ctx.layout()
            print("N=%d factorize(N) with reserve %4d (ld %d, rows %d): median %.3f ms (min %.3f, %d repeats)"
                  % (N, reserve, lay["ld"], lay["rows"], float(np.median(ref)), min(ref), repeats), flush=True)
        ctx.set_option("reserve", 0)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="4096,16384,65536")
    ap.add_argument("--ks", default="1,16,128,1024")
    ap.add_argument("--dim", type=int, default=8)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r14_append_rate.txt"))
    ap.add_argument("--parent-root", default=None)
    ap.add_argument("--child", default=None)
    ap.add_argument("--size", type=int, default=0)
    a = ap.parse_args()
    ks = [int(v) for v in a.ks.split(",")]
    if a.child == "append":
        return child_append(a.size, ks, a.dim, a.repeats)
    if a.child == "factorize":
        return child_factorize(a.parent_root, a.size, ks, a.dim, a.repeats)
    lines = ["gpmi_append against gpmi_factorize: scripts/append_rate.py --sizes %s --ks %s --dim %d --repeats %d%s"
             % (a.sizes, a.ks, a.dim, a.repeats, " --parent-root <checkout of the parent commit, built>" if a.parent_root else ""),
             "wall ms of the call (one synchronisation inside); build / sweep / border: the stage timers GPMI_T_KS, GPMI_T_SOLVE_V, GPMI_T_CHOL"]
    status = 0
    for N in [int(v) for v in a.sizes.split(",")]:
        reps = a.repeats if N < 65536 else 1
        jobs = [("append", None)] + ([("factorize", a.parent_root)] if a.parent_root else [])
        for child, root in jobs:
            cmd = [sys.executable, os.path.abspath(__file__), "--child", child, "--size", str(N), "--ks", a.ks,
                   "--dim", str(a.dim), "--repeats", str(reps)] + (["--parent-root", root] if root else [])
            try:
                p = subprocess.run(cmd, capture_output=True, text=True, timeout=LIMITS.get(N, 480))
            except subprocess.TimeoutExpired:
                lines.append("N=%d %s: time limit" % (N, child))
                status = 124
                break
            out = [ln + ("  [parent commit]" if root else "") for ln in p.stdout.splitlines()]
            lines += out
            print("\n".join(out), flush=True)
            if p.returncode != 0:
                lines.append("N=%d %s: exit status %d\n%s" % (N, child, p.returncode, p.stderr[-2000:]))
                status = p.returncode
                break
        if status:
            break
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        f.write("\n".join(lines) + "\n")
    print("\n".join(lines[-3:]))
    return status


if __name__ == "__main__":
    sys.exit(main() or 0)
