"""NumPy float64 mirror of gpmi_softmax_grad: the gradient of the Laplace approximation log q(y | X, theta) of the
multi-class softmax classifier w.r.t. the relative lengthscales r_k, the common lengthscale l and sigma, on top of
tests/softmax_ref.fit and in softmax_grad.hip's order of operations.  Per-dimension lengthscales: X is divided by r.

At the mode (notation of softmax_ref.fit): P = softmax(F^), G = Y - P, E_c, M M^T = sum_c E_c, one K for all classes.
For every hyper-parameter of K

    dlog q/dtheta = 1/2 sum_ik dK_ik/dtheta Wm_ik
    Wm    = -sum_c E_c + Gamma + sum_c (g_c g_c^T + z_c g_c^T + g_c z_c^T)
    Gamma = sum_c E_c (M M^T)^-1 E_c = sum_c T_c^T T_c,  T_c^T = E_c M^-T
    Sigma_i[c, e] = delta_ce (K_ii - (K E_c K)_ii) + Q_c[i] . Q_e[i],  Q_c = K E_c M^-T   (posterior covariance at point i)
    q_i   = diag(Sigma_i) - 2 Sigma_i pi_i
    s2_ci = -1/2 pi_ci (q_ci - pi_i . q_i)
    v_c   = E_c (K s2_c),  t = M^-T M^-1 sum_c v_c,  z_c = s2_c - v_c + E_c t

(-sum_c E_c + Gamma is minus the sum of the diagonal blocks of R = (K_blk + W^-1)^-1, GPML eq. 3.47; z = s2 - R K_blk s2
carries the dependence of the mode on theta.)  Test infrastructure only."""
import numpy as np
from scipy.linalg import solve_triangular

import softmax_ref as S
from laplace_ref import rbf


def point_covariances(fit, sig2):
    """Sigma (N, C, C): the posterior covariance of the C latent values at every training point, the prediction's path
    (softmax_ref.predict) with R = K and sigma^2 on the diagonal"""
    K, Es, M = fit["K"], fit["Es"], fit["M"]
    C, N = fit["P"].shape
    Bc = [K @ Es[c] for c in range(C)]
    U = [solve_triangular(M, Bc[c].T, lower=True) for c in range(C)]
    Sig = np.zeros((N, C, C))
    for c in range(C):
        for e in range(c + 1):
            Sig[:, c, e] = Sig[:, e, c] = np.sum(U[c] * U[e], axis=0)
        Sig[:, c, c] += sig2 - np.sum(Bc[c] * K, axis=1)
    return Sig


def third_derivative_term(Sig, P):
    """s2 (C, N) from Sigma (N, C, C) and P (C, N): s2_ci = -1/2 sum_pq Sigma_i[p, q] dW_i[p, q]/df_ci"""
    q = np.einsum("icc->ci", Sig) - 2.0 * np.einsum("ice,ei->ci", Sig, P)
    return -0.5 * P * (q - np.sum(P * q, axis=0))


def weights(fit, sig2, flip_s2=False, drop_gamma=False):
    """-> (Wm, parts): the N x N matrix in front of dK/dtheta / 2 and what it is made of.  flip_s2 / drop_gamma are
    the negative controls of tests/test_softmax_grad_cpu.py."""
    K, P, G, Es, M = fit["K"], fit["P"], fit["G"], fit["Es"], fit["M"]
    C, N = P.shape
    Sig = point_covariances(fit, sig2)
    s2 = third_derivative_term(Sig, P)
    if flip_s2:
        s2 = -s2
    Ks2 = s2 @ K
    V = np.stack([Es[c] @ Ks2[c] for c in range(C)])
    t = solve_triangular(M.T, solve_triangular(M, V.sum(axis=0), lower=True), lower=False)
    Z = s2 - V + np.stack([Es[c] @ t for c in range(C)])
    Gamma = np.zeros((N, N))
    for c in range(C):
        T = solve_triangular(M, Es[c], lower=True)                 # T_c = M^-1 E_c
        Gamma += T.T @ T
    Wm = -sum(Es[1:], Es[0])
    if not drop_gamma:
        Wm = Wm + Gamma
    for c in range(C):
        Wm = Wm + np.outer(G[c], G[c]) + np.outer(Z[c], G[c]) + np.outer(G[c], Z[c])
    return Wm, dict(Sigma=Sig, s2=s2, z=Z, Gamma=Gamma, t=t)


def gradient_from(fit, Z, sigma, l, r, **controls):
    """(d_r, d_l, d_sigma) from a fit on Z = X / r"""
    Wm, _ = weights(fit, sigma * sigma, **controls)
    WK = 0.5 * Wm * fit["K"]
    d_r = np.array([np.sum(WK * ((Z[:, k, None] - Z[None, :, k]) ** 2)) / (l * l * r[k]) for k in range(Z.shape[1])])
    d_l = float(np.sum(d_r * r)) / l                           # sum_k D2_k = sq: dK/dl = K sq / l^3
    d_sigma = 2.0 * float(np.sum(WK)) / sigma
    return d_r, d_l, d_sigma


def log_q_and_gradient(X, labels, C, sigma, l, r=None, tol=1e-13, max_iter=100, perturb=None, **controls):
    """-> dict(log_q, d_r (d,), d_l, d_sigma, fit).  perturb: an N x N symmetric matrix of relative perturbations
    applied to K before the fit (the rounding experiment of tests/test_softmax_grad_cpu.py)."""
    X = np.asarray(X, dtype=np.float64)
    r = np.ones(X.shape[1]) if r is None else np.asarray(r, dtype=np.float64).reshape(-1)
    Z = X / r
    K = None
    if perturb is not None:
        K = rbf(Z, Z, sigma, l) * (1.0 + perturb)
    fit = S.fit(Z, labels, C, sigma, l, tol=tol, max_iter=max_iter, K=K)
    d_r, d_l, d_sigma = gradient_from(fit, Z, sigma, l, r, **controls)
    return dict(log_q=fit["log_q"], d_r=d_r, d_l=d_l, d_sigma=d_sigma, fit=fit)


def flat(res):
    """the d + 2 derivatives as one vector (r..., l, sigma)"""
    return np.concatenate([res["d_r"], [res["d_l"], res["d_sigma"]]])


class MirrorContext:
    """The slice of GPContext the multi-class tuner uses, served by the mirror (CPU tests of the tuner's loop)."""

    def __init__(self):
        self.r = None
        self.res = None
        self.fits = 0
        self.n_classes = 0

    def set_lengthscales(self, r):
        self.r = None if r is None else np.asarray(r, dtype=np.float64).reshape(-1)
        self.res = None

    def softmax_fit(self, X, labels, n_classes, sigma, l, *, tol=1e-10, max_iter=100, lengthscales=None):
        self.r = None if lengthscales is None else np.asarray(lengthscales, dtype=np.float64).reshape(-1)
        self.res = log_q_and_gradient(X, labels, n_classes, sigma, l, self.r, tol=tol, max_iter=max_iter)
        self.n_classes = n_classes
        self.fits += 1
        fit = self.res["fit"]
        return fit["log_q"], fit["F"], fit["iters"], fit["converged"]

    def softmax_grad(self):
        if self.res is None:
            raise ValueError("gpmi_softmax_grad: no softmax fit resident (call gpmi_softmax_fit)")
        return self.res["d_r"], self.res["d_l"], self.res["d_sigma"]
