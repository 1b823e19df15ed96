"""Write tests/golden/laplace_grad/*.npz: scikit-learn's gradient of the Laplace log marginal likelihood of the binary
classifier, GaussianProcessClassifier(ConstantKernel(sigma**2) * RBF(l * r), optimizer=None, max_iter_predict=200)
.log_marginal_likelihood(theta, eval_gradient=True), the external check of tests/test_laplace_grad_cpu.py and
tests/test_laplace_grad_gpu.py.  A sibling of scripts/make_laplace_golden.py: the first three cases are its inputs.

    python scripts/make_laplace_grad_golden.py

scikit-learn differentiates w.r.t. theta = (log sigma**2, log(l r_1), ..., log(l r_d)); the files hold the gradient
converted to the parameters of gpmi_laplace_grad,

    d/dsigma = (2 / sigma) d/dlog sigma**2,   d/dr_k = (1 / r_k) d/dlog(l r_k),   d/dl = (1 / l) sum_k d/dlog(l r_k),

with X, y (+-1), sigma, l, r and log_marginal_likelihood."""
import os

import numpy as np
from sklearn.gaussian_process import GaussianProcessClassifier
from sklearn.gaussian_process.kernels import RBF, ConstantKernel

from make_laplace_golden import data

OUT = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tests", "golden", "laplace_grad")

# name, data, N, d, points drawn (the first N are kept), sigma, l, r (None: all 1), seed
CASES = [
    ("moons_N50_d2", "moons", 50, 2, 87, 1.0, 0.5, None, 0),
    ("blobs_N300_d1", "blobs", 300, 1, 428, 2.0, 1.0, None, 1),
    ("blobs_N1024_d8", "blobs", 1024, 8, 1224, 1.5, 3.0, None, 2),
    ("moons_N50_d2_ard", "moons", 50, 2, 87, 1.0, 0.5, [0.7, 1.6], 0),
    ("blobs_N1024_d8_ard", "blobs", 1024, 8, 1224, 1.5, 3.0, [0.6, 1.0, 1.7, 0.8, 2.5, 1.2, 0.9, 1.4], 2),
    ("blobs_N257_d8_saturated", "blobs", 257, 8, 257, 12.0, 3.0, [1.3, 0.8, 1.0, 2.0, 0.7, 1.1, 1.6, 0.9], 4),
]


def main():
    os.makedirs(OUT, exist_ok=True)
    for name, kind, N, d, drawn, sigma, l, r, seed in CASES:
        X, y = data(kind, drawn, d, seed)
        X, y = X[:N], y[:N]
        r = np.ones(d) if r is None else np.asarray(r, dtype=np.float64)
        k = ConstantKernel(sigma ** 2) * RBF(l * r)
        gpc = GaussianProcessClassifier(k, optimizer=None, max_iter_predict=200).fit(X, y)
        lml, g = gpc.log_marginal_likelihood(gpc.kernel_.theta, eval_gradient=True)
        d_sigma = 2.0 / sigma * g[0]
        d_r = g[1:] / r
        d_l = float(np.sum(g[1:])) / l
        np.savez_compressed(os.path.join(OUT, name + ".npz"), X=X, y=y, sigma=sigma, l=l, r=r,
                            log_marginal_likelihood=lml, d_r=d_r, d_l=d_l, d_sigma=d_sigma)
        print(name, lml, d_l, d_sigma, "max|f^| %.2f" % np.max(np.abs(gpc.base_estimator_.f_cached)))


if __name__ == "__main__":
    main()
