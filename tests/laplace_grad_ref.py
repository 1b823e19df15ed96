"""NumPy float64 mirror of gpmi_laplace_grad: the gradient of the Laplace approximation log q(y | X, theta) of the
binary classifier (GPML Algorithm 5.1, logistic likelihood) w.r.t. the relative lengthscales r_k, the common
lengthscale l and sigma, on top of tests/laplace_ref.laplace_fit.  Per-dimension lengthscales: X is divided by r.

At the mode f^: pi = expit(f^), W = pi (1 - pi), s = sqrt(W), g = t - pi, a = K^-1 f^ (= g at the mode),
B = I + s s^T o K = L L^T, R = diag(s) B^-1 diag(s), and for every hyper-parameter

    dlog q/dtheta = sum_ik dK_ik/dtheta [ (a_i a_k - R_ik) / 2 + (z_i g_k + z_k g_i) / 2 ]
    s2_i = -(1 - [B^-1]_ii) (1 - 2 pi_i) / 2
    z    = s2 - R (K s2)

(z^T dK g is GPML's implicit term s2^T (I - K R) dK g with the matrix moved onto the left vector.)  Test
infrastructure only."""
import numpy as np
from scipy.linalg import solve_triangular

import laplace_ref as R


def weights(fit, a=None):
    """-> (Wt, parts): the N x N weight matrix in front of dK/dtheta and the vectors it is made of"""
    K, f, g, s, L = fit["K"], fit["f"], fit["grad"], fit["s"], fit["L"]
    a = g if a is None else a
    N = f.shape[0]
    pi = R.expit(f)
    U = solve_triangular(L, np.eye(N), lower=True).T           # L^-T
    Binv = U @ U.T
    kappa = np.einsum("ij,ij->i", U, U)
    Rm = s[:, None] * Binv * s[None, :]
    s2 = -0.5 * (1.0 - kappa) * (1.0 - 2.0 * pi)
    z = s2 - Rm @ (K @ s2)
    Wt = 0.5 * (np.outer(a, a) - Rm) + 0.5 * (np.outer(z, g) + np.outer(g, z))
    return Wt, dict(kappa=kappa, s2=s2, z=z, a=a, pi=pi)


def gradient_from(fit, Z, sigma, l, r):
    """(d_r, d_l, d_sigma) from a fit on Z = X / r"""
    Wt, _ = weights(fit)
    WK = Wt * fit["K"]
    d_r = np.array([np.sum(WK * ((Z[:, k, None] - Z[None, :, k]) ** 2)) / (l * l * r[k]) for k in range(Z.shape[1])])
    d_l = float(np.sum(d_r * r)) / l                           # sum_k D2_k = sq: dK/dl = K sq / l^3
    d_sigma = 2.0 * float(np.sum(WK)) / sigma
    return d_r, d_l, d_sigma


def log_q_and_gradient(X, y, sigma, l, r=None, tol=1e-13, max_iter=100, perturb=None):
    """-> dict(log_q, d_r (d,), d_l, d_sigma, fit).  perturb: an N x N symmetric matrix of relative perturbations
    applied to K before the fit (the rounding experiment of tests/test_laplace_grad_cpu.py)."""
    X = np.asarray(X, dtype=np.float64)
    r = np.ones(X.shape[1]) if r is None else np.asarray(r, dtype=np.float64).reshape(-1)
    Z = X / r
    K = None
    if perturb is not None:
        K = R.rbf(Z, Z, sigma, l) * (1.0 + perturb)
    fit = R.laplace_fit(Z, y, sigma, l, tol=tol, max_iter=max_iter, K=K)
    d_r, d_l, d_sigma = gradient_from(fit, Z, sigma, l, r)
    return dict(log_q=fit["log_q"], d_r=d_r, d_l=d_l, d_sigma=d_sigma, fit=fit)


def flat(res):
    """the d + 2 derivatives as one vector (r..., l, sigma)"""
    return np.concatenate([res["d_r"], [res["d_l"], res["d_sigma"]]])


class MirrorContext:
    """The slice of GPContext the classification tuner uses, served by the mirror (CPU tests of the tuner's loop)."""

    def __init__(self):
        self.r = None
        self.res = None
        self.fits = 0

    def set_lengthscales(self, r):
        self.r = None if r is None else np.asarray(r, dtype=np.float64).reshape(-1)
        self.res = None

    def laplace_fit(self, X, y, sigma, l, *, tol=1e-10, max_iter=100, lengthscales=None):
        self.r = None if lengthscales is None else np.asarray(lengthscales, dtype=np.float64).reshape(-1)
        self.res = log_q_and_gradient(X, y, sigma, l, self.r, tol=tol, max_iter=max_iter)
        self.fits += 1
        fit = self.res["fit"]
        return fit["log_q"], fit["f"], fit["iters"], fit["converged"]

    def laplace_grad(self):
        if self.res is None:
            raise ValueError("gpmi_laplace_grad: no Laplace fit resident (call gpmi_laplace_fit)")
        return self.res["d_r"], self.res["d_l"], self.res["d_sigma"]
