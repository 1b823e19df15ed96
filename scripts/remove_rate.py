"""gpmi_remove against a refit (profiles/r16_remove_rate.txt).

    python scripts/remove_rate.py [--sizes 4096,16384,65536] [--dim 8] [--repeats 3]
                                  [--out profiles/r16_remove_rate.txt] [--parent-root DIR]

One child process per size, each under a time limit of its own; the first that fails or runs out of time ends the run.
Per N and index set -- the first point, a middle one, the last, 16 spread out, 128 spread out (eight sweeps): the wall
time of GPContext.remove (the call ends with its one synchronisation) behind a fit of N points, median of the repeats,
once with the second buffer allocated and freed inside the call (option "remove_keep_spare" 0) and once into a buffer
kept from an earlier removal (option 1; the earlier removal is that of the last point, so this row removes from
N - 1 points); the stage timers summed over the call's sweeps -- GPMI_T_KS what only moves (the 2-D copy, the columns
below J0, the padding), GPMI_T_SOLVE_V the sweeps, GPMI_T_CHOL the tile inverses; the bytes the plan says the sweeps
stream against the sweep time; and gpmi_factorize of the surviving points in the same process.  Then one
slide_window step (remove the oldest, append one; "reserve" 128, spare kept).
--parent-root: a checkout of the parent commit with its library built; gpmi_factorize of the same sizes is then timed
there too (a child per size), which is the refit a caller had to pay before gpmi_remove existed."""
import argparse
import os
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIMITS = {4096: 180, 16384: 240, 65536: 540}          # seconds per child


def _data(N, d):
    rng = np.random.default_rng(N)
    X = rng.uniform(0.0, 4.0, size=(N, d))
    y = np.sin(X.sum(1)) + 0.05 * rng.standard_normal(N)
    return X, y


def _wall(fn):
    t = time.perf_counter()
    fn()
    return (time.perf_counter() - t) * 1e3


def index_sets(N):
    return [("first", [0]), ("middle", [N // 2]), ("last", [N - 1]),
            ("16 spread", [i * N // 16 + 5 for i in range(16)]), ("128 spread", [i * N // 128 + 3 for i in range(128)])]


def stream_bytes(N, idx):
    """what remove_plan (gpmi_remove_plan.h) counts: per sweep the old trailing trapezoid from J0 on, whole 128 x 128 blocks"""
    s, total, n = sorted(idx), 0, N
    end = len(s)
    while end > 0:
        first = max(0, end - 16)
        b0, b1 = s[first] // 128, (n + 127) // 128
        total += (b1 * (b1 + 1) // 2 - b0 * (b0 + 1) // 2) * 128 * 128 * 8
        n -= end - first
        end = first
    return total


def child_factorize(root, N, d, repeats):
    """gpmi_factorize of the surviving points from the tree at `root` (the parent's)"""
    sys.path.insert(0, root)
    from gaussian_process_amd import GPContext
    X, y = _data(N, d)
    with GPContext(0) as ctx:
        for k in (1, 16, 128):
            ctx.set_train(X[:N - k], y[:N - k])
            ctx.factorize(1.2, 1.3 * np.sqrt(d), 1e-2)
            ms = [_wall(lambda: ctx.factorize(1.2, 1.3 * np.sqrt(d), 1e-2)) for _ in range(repeats)]
            print("N=%d k=%d factorize(N-k) median %.3f ms (min %.3f, %d repeats)" % (N, k, float(np.median(ms)), min(ms), repeats),
                  flush=True)


def child_remove(N, d, repeats):
    sys.path.insert(0, ROOT)
    from gaussian_process_amd import GPContext
    from gaussian_process_amd import GP_regression as G
    X, y = _data(N + 8, d)
    sig, ell, noise = 1.2, 1.3 * np.sqrt(d), 1e-2
    with GPContext(0) as ctx:
        for name, idx in index_sets(N):
            for spare in (0, 1):
                ctx.set_option("remove_keep_spare", spare)
                ms, cp, sw, inv = [], [], [], []
                for _ in range(repeats + 1):              # the first is the warm-up
                    ctx.set_train(X[:N], y[:N])
                    ctx.factorize(sig, ell, noise)
                    use = idx
                    if spare:                              # a fit drops the spare: a cheap removal leaves one
                        ctx.remove([N - 1])
                        use = [min(i, N - 2) for i in idx]
                    ms.append(_wall(lambda: ctx.remove(use)))
                    t = ctx.timers()
                    cp.append(t["ks"]); sw.append(t["solve_v"]); inv.append(t["chol"])
                ms, cp, sw, inv = ms[1:], cp[1:], sw[1:], inv[1:]
                s, nsw = float(np.median(sw)), (len(idx) + 15) // 16
                gb = stream_bytes(N - spare, use) / 1e9
                print("N=%d remove %-10s (k=%3d, %d sweep%s) spare %-8s median %.3f ms (min %.3f)  copy %.3f  sweep %.3f  inverses %.3f ms;  "
                      "sweeps read %.2f GB (and write as much): %.0f GB/s read"
                      % (N, name, len(idx), nsw, "" if nsw == 1 else "s", "kept" if spare else "not kept", float(np.median(ms)), min(ms),
                         float(np.median(cp)), s, float(np.median(inv)), gb, gb / (s * 1e-3) if s > 0 else 0.0), flush=True)
        ctx.set_option("remove_keep_spare", 0)
        for k in (1, 16, 128):
            ctx.set_train(X[:N - k], y[:N - k])
            ctx.factorize(sig, ell, noise)
            ref = [_wall(lambda: ctx.factorize(sig, ell, noise)) for _ in range(repeats)]
            print("N=%d k=%d factorize(N-k) median %.3f ms (min %.3f, %d repeats), this build" % (N, k, float(np.median(ref)), min(ref), repeats),
                  flush=True)
        # one sliding-window step: the oldest point out, a new one in; nothing is allocated from the second step on
        ctx.set_option("reserve", 128)
        ctx.set_option("remove_keep_spare", 1)
        ctx.set_train(X[:N], y[:N])
        ctx.factorize(sig, ell, noise)
        G.slide_window(X[N:N + 1], y[N:N + 1], ctx=ctx)
        ms = [_wall(lambda: G.slide_window(X[N + 1 + i:N + 2 + i], y[N + 1 + i:N + 2 + i], ctx=ctx)) for i in range(repeats)]
        print("N=%d slide_window step (remove the oldest, append one; reserve 128, spare kept) median %.3f ms (min %.3f, %d repeats)"
              % (N, float(np.median(ms)), min(ms), repeats), flush=True)
        ctx.set_option("reserve", 0)
        ctx.set_option("remove_keep_spare", 0)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="4096,16384,65536")
    ap.add_argument("--dim", type=int, default=8)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r16_remove_rate.txt"))
    ap.add_argument("--parent-root", default=None)
    ap.add_argument("--child", default=None)
    ap.add_argument("--size", type=int, default=0)
    a = ap.parse_args()
    if a.child == "remove":
        return child_remove(a.size, a.dim, a.repeats)
    if a.child == "factorize":
        return child_factorize(a.parent_root, a.size, a.dim, a.repeats)
    lines = ["gpmi_remove against gpmi_factorize: scripts/remove_rate.py --sizes %s --dim %d --repeats %d%s"
             % (a.sizes, a.dim, a.repeats, " --parent-root <checkout of the parent commit, built>" if a.parent_root else ""),
             "wall ms of the call (one synchronisation inside), median of the repeats; copy / sweep / inverses: the stage timers "
             "GPMI_T_KS, GPMI_T_SOLVE_V, GPMI_T_CHOL summed over the call's sweeps"]
    status = 0
    for N in [int(v) for v in a.sizes.split(",")]:
        jobs = [("remove", None)] + ([("factorize", a.parent_root)] if a.parent_root else [])
        for child, root in jobs:
            cmd = [sys.executable, os.path.abspath(__file__), "--child", child, "--size", str(N), "--dim", str(a.dim),
                   "--repeats", str(a.repeats)] + (["--parent-root", root] if root else [])
            try:
                p = subprocess.run(cmd, capture_output=True, text=True, timeout=LIMITS.get(N, 540))
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
