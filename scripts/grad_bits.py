"""SHA-256 of the bits every entry point that reaches csrc/grad.hip returns, from fixed seeds, on one MI355X: the check that
a change to the gradient kernels is a refactor.  Run it on the parent commit's build and on the new one and diff the two
files -- every digest must be equal, there is no tolerance.

    python scripts/grad_bits.py --out FILE [--root TREE]

--root: the tree whose gaussian_process_amd (and the libgpmi355x.so built beside it) is imported; default: this one.  One
JSON object: case name -> digest of the raw float64 bytes of everything the call returns.  A few hundred points per case;
the grid covers every instantiation of the tile kernels (families 0 .. 3, LDS and global memory, the four ARD widths and
two and three launches, the Laplace weight, tri and rectangular traces with a row0 and a row cut, duplicated points)."""
import argparse
import hashlib
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KINDS = {0: "rbf", 4: "matern12", 5: "matern32", 6: "matern52"}
SIGMA, NOISE = 1.3, 1e-2
CO2_THETA_MD = np.array([1.5, 1.2, 0.8, 2.0, 8.0, 0.7, 0.9, 1.3, 0.3, 0.5, 0.5])    # tests/co2_grad_ref.py
CO2_NOISE = 5e-4


def digest(*vals):
    h = hashlib.sha256()
    for v in vals:
        h.update(np.ascontiguousarray(np.atleast_1d(np.asarray(v, dtype=np.float64))).tobytes())
    return h.hexdigest()


def problem(N, d, seed=0):
    rng = np.random.default_rng(1000 * N + d + seed)
    X = rng.standard_normal((N, d))
    y = np.sin(X.sum(1)) + 0.1 * rng.standard_normal(N)
    r = 0.75 + 0.5 * rng.random(d)                          # relative lengthscales
    return X, y, r, 0.9 * np.sqrt(d)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", required=True)
    ap.add_argument("--root", default=ROOT)
    a = ap.parse_args()
    sys.path.insert(0, os.path.abspath(a.root))
    import torch
    from gaussian_process_amd import GPContext, _lib
    from gaussian_process_amd.dist import HipBlockOps

    print("library:", _lib.LIB_PATH, flush=True)
    res = {}

    def put(name, *vals):
        res[name] = digest(*vals)
        print(name, res[name][:16], flush=True)

    with GPContext(0) as c:
        def regression(kind, X, y, ell, r=None):
            c.set_kernel(KINDS[kind])
            return c.fit(X, y, SIGMA, ell, NOISE, lengthscales=r)

        for kind in KINDS:
            for N, d in ((130, 2), (641, 5), (257, 33)):
                X, y, r, ell = problem(N, d)
                regression(kind, X, y, ell)
                put("lml_grad kind=%d N=%d d=%d" % (kind, N, d), *c.lml_grad())
            for N, d in [(257, d) for d in (1, 4, 5, 13, 20, 32, 33, 70)] + [(641, 5)]:
                X, y, r, ell = problem(N, d)
                regression(kind, X, y, ell, r)
                put("lml_grad_ard kind=%d N=%d d=%d" % (kind, N, d), *c.lml_grad_ard())
            for N, d in ((130, 2), (257, 33)):
                X, y, r, ell = problem(N, d)
                regression(kind, X, y, ell)
                put("loo_grad kind=%d N=%d d=%d" % (kind, N, d), *c.loo_grad())
        # nu = 1/2 with two training rows duplicated: H_1/2 is selected to 0 where sq == 0
        X, y, r, ell = problem(130, 2, seed=7)
        X[7], X[129] = X[3], X[64]
        regression(4, X, y, ell)
        put("lml_grad kind=4 N=130 d=2 duplicated rows", *c.lml_grad())
        regression(4, X, y, ell, r)
        put("lml_grad_ard kind=4 N=130 d=2 duplicated rows", *c.lml_grad_ard())
        c.set_kernel("rbf")

        for d in (2, 13, 33):
            X, y, r, ell = problem(257, d, seed=1)
            c.laplace_fit(X, np.where(y > 0, 1.0, -1.0), SIGMA, ell, tol=1e-13, lengthscales=r)
            put("laplace_grad N=257 d=%d" % d, *c.laplace_grad())
        for d in (5, 33):
            X, y, r, ell = problem(257, d, seed=2)
            labels = np.digitize(y, np.quantile(y, [1 / 3, 2 / 3]))
            c.softmax_fit(X, labels, 3, SIGMA, ell, tol=1e-13, lengthscales=r)
            put("softmax_grad C=3 N=257 d=%d" % d, *c.softmax_grad())

        g = np.load(os.path.join(ROOT, "tests", "golden", "kernels_bo_co2.npz"))
        rng = np.random.default_rng(40)
        Xmd = rng.uniform(0.0, 4.0, size=(257, 40)) / np.sqrt(40)
        ymd = np.sin(Xmd.sum(1)) + 0.05 * rng.standard_normal(257)
        for tag, X, y, th in (("fixture N=360 d=1", g["co2_X"][:360], g["co2_y"][:360], g["co2_theta"]),
                              ("N=257 d=40", Xmd, ymd, CO2_THETA_MD)):
            try:
                c.set_kernel("co2", th)
                c.fit(X, y, 1.0, 1.0, CO2_NOISE, lengthscales=None)
                put("lml_grad_co2 " + tag, *c.lml_grad_co2())
            finally:
                c.set_kernel("rbf")

        for N, d in ((300, 3), (300, 33)):                      # every tile of the rectangle, tri = 0
            X, y, r, ell = problem(N, d, seed=3)
            rng = np.random.default_rng(N + d)
            Kinv = rng.standard_normal((N, N))
            put("grad_trace N=%d d=%d" % (N, d), *c.grad_trace(X, X, SIGMA, ell, rng.standard_normal(N), Kinv + Kinv.T))

    ops = HipBlockOps(0)
    N, d, row0 = 300, 3, 128                                    # a row block of the partitioned path: whole, and cut short
    X, y, r, ell = problem(N, d, seed=4)
    rng = np.random.default_rng(5)
    dev = lambda v: torch.from_numpy(np.ascontiguousarray(v)).to(ops.device)      # noqa: E731
    for nrows in (128, 100):
        out = torch.zeros(2, dtype=torch.float64, device=ops.device)
        part = torch.empty(2 * -(-nrows // 128) * -(-N // 128), dtype=torch.float64, device=ops.device)
        ops.grad_trace(dev(X), N, d, row0, nrows, dev(rng.standard_normal(N)), dev(rng.standard_normal(N)),
                       dev(rng.standard_normal((nrows, N + 10))), -1.0, SIGMA, ell, part, out)
        ops.sync()
        put("HipBlockOps.grad_trace N=300 d=3 row0=128 nrows=%d" % nrows, out.cpu().numpy())

    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1, sort_keys=True)
        f.write("\n")
    print("%d cases -> %s" % (len(res), a.out))


if __name__ == "__main__":
    main()
