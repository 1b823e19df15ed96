"""Write tests/golden/laplace/*.npz: scikit-learn's GaussianProcessClassifier (the same GPML Algorithms 3.1 / 3.2, binary
Laplace, fixed kernel ConstantKernel(sigma**2) * RBF(l), no hyper-parameter optimisation) on seeded two-moons and
Gaussian-blob data, the external check of tests/test_laplace_cpu.py and tests/test_laplace_gpu.py.

    python scripts/make_laplace_golden.py

Each file holds X, y (+-1), Xs, sigma, l and sklearn's log_marginal_likelihood_value_, f_cached (its last Newton
iterate), pi_ and W_sr_ of base_estimator_, the latent mean / variance at Xs computed from those as its predict_proba
does (L_ itself is not kept: N x N), and predict_proba[:, 1] (the erf-mixture approximation of the integral).  The fixtures live in a
subdirectory: tests/golden/*.npz are the regression parity cases."""
import os

import numpy as np
from scipy.linalg import solve_triangular
from sklearn.datasets import make_blobs, make_moons
from sklearn.gaussian_process import GaussianProcessClassifier
from sklearn.gaussian_process.kernels import RBF, ConstantKernel

OUT = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tests", "golden", "laplace")

# name, data, N, d, n test points, sigma, l, seed
CASES = [
    ("moons_N50_d2", "moons", 50, 2, 37, 1.0, 0.5, 0),
    ("blobs_N300_d1", "blobs", 300, 1, 128, 2.0, 1.0, 1),
    ("blobs_N1024_d8", "blobs", 1024, 8, 200, 1.5, 3.0, 2),
    ("moons_N2000_d2", "moons", 2000, 2, 257, 3.0, 0.7, 3),
]


def data(kind, n, d, seed):
    if kind == "moons":
        X, y = make_moons(n_samples=n, noise=0.3, random_state=seed)
    else:
        X, y = make_blobs(n_samples=n, n_features=d, centers=2, cluster_std=2.5, random_state=seed)
    return X.astype(np.float64), np.where(y == 1, 1.0, -1.0)


def main():
    os.makedirs(OUT, exist_ok=True)
    for name, kind, N, d, n, sigma, l, seed in CASES:
        X, y = data(kind, N + n, d, seed)
        X, Xs, y = X[:N], X[N:], y[:N]
        k = ConstantKernel(sigma ** 2, "fixed") * RBF(l, "fixed")
        gpc = GaussianProcessClassifier(k, optimizer=None).fit(X, y)
        be = gpc.base_estimator_
        Ks = be.kernel_(be.X_train_, Xs)
        f_mean = Ks.T.dot(be.y_train_ - be.pi_)
        v = solve_triangular(be.L_, be.W_sr_[:, None] * Ks, lower=True)
        f_var = be.kernel_.diag(Xs) - np.einsum("ij,ij->j", v, v)
        np.savez_compressed(os.path.join(OUT, name + ".npz"), X=X, y=y, Xs=Xs, sigma=sigma, l=l,
                            log_marginal_likelihood=be.log_marginal_likelihood_value_, f_cached=be.f_cached,
                            pi=be.pi_, W_sr=be.W_sr_, f_mean=f_mean, f_var=f_var,
                            prob=gpc.predict_proba(Xs)[:, 1])
        print(name, be.log_marginal_likelihood_value_)


if __name__ == "__main__":
    main()
