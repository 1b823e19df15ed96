"""Dense NumPy float64 mirror of leave-one-out cross-validation for GP regression (Rasmussen & Williams, GPML, section
5.4.2), on the problems and the kernel of tests/ard_ref.py.  With K_y = K + noise I, alpha = K_y^-1 y, kappa_i = [K_y^-1]_ii:

    mu_i = y_i - alpha_i / kappa_i,   var_i = 1 / kappa_i,   logp_i = -.5 log var_i - (y_i - mu_i)^2 / (2 var_i) - .5 log 2 pi
    dL_LOO/dtheta = sum_i (alpha_i r_i - .5 (1 + alpha_i^2 / kappa_i) s_i) / kappa_i,   Z = K_y^-1 dK_y/dtheta, r = Z alpha,
                                                                                        s_i = [Z K_y^-1]_ii     (eq. 5.13)

(a) closed(): those closed forms from the explicit symmetrised inverse, each derivative with the scale at which its terms
    cancel, sum_i (|alpha_i r_i / kappa_i| + |.5 (1 + alpha_i^2 / kappa_i) s_i / kappa_i|) -- the construction of s_* in ard_ref.py;
(b) brute(): N separate fits, each with one point deleted, predicting the deleted point with the noise variance included.
Test infrastructure: dense N x N matrices (and N of them one after the other in (b)), small N only.
"""
import numpy as np

import ard_ref as R

HALF_LOG_2PI = .5 * np.log(2 * np.pi)


def _logp(y, mu, var):
    return -.5 * np.log(var) - (y - mu) ** 2 / (2 * var) - HALF_LOG_2PI


def from_Ky(Ky, y):
    """the closed forms for any covariance: -> dict mu, var, logp, loo, alpha, kappa, Kinv, cond"""
    y = np.asarray(y, dtype=np.float64).reshape(-1)
    Kinv = np.linalg.inv(Ky)
    Kinv = .5 * (Kinv + Kinv.T)
    alpha = Kinv @ y
    kappa = np.diag(Kinv).copy()
    mu, var = y - alpha / kappa, 1.0 / kappa
    logp = _logp(y, mu, var)
    return {"mu": mu, "var": var, "logp": logp, "loo": float(np.sum(logp)), "alpha": alpha, "kappa": kappa,
            "Kinv": Kinv, "cond": float(np.linalg.cond(Ky))}


def values(X, y, r, sigma, l, noise):
    X = np.asarray(X, dtype=np.float64)
    return from_Ky(R.kernel(X, r, sigma, l) + noise * np.eye(X.shape[0]), y)


def total(X, y, r, sigma, l, noise):
    return values(X, y, r, sigma, l, noise)["loo"]


def closed(X, y, r, sigma, l, noise):
    """values() plus g_l, g_sigma, g_noise and their cancellation scales s_l, s_sigma, s_noise"""
    X = np.asarray(X, dtype=np.float64)
    N = X.shape[0]
    K = R.kernel(X, r, sigma, l)
    out = from_Ky(K + noise * np.eye(N), y)
    Kinv, alpha, kappa = out["Kinv"], out["alpha"], out["kappa"]

    def both(dK):
        Z = Kinv @ dK
        rr = Z @ alpha
        s = np.sum(Z * Kinv, axis=1)                 # [Z K_y^-1]_ii, K_y^-1 symmetric
        a = alpha * rr / kappa
        b = .5 * (1.0 + alpha ** 2 / kappa) * s / kappa
        return float(np.sum(a - b)), float(np.sum(np.abs(a) + np.abs(b)))

    out["g_l"], out["s_l"] = both(K * R.sq_parts(X, r).sum(-1) / l ** 3)
    out["g_sigma"], out["s_sigma"] = both(2 * K / sigma)
    out["g_noise"], out["s_noise"] = both(np.eye(N))
    return out


def brute_from_Ky(Ky, y):
    """N fits with one point deleted each: -> dict mu, var, logp, loo"""
    y = np.asarray(y, dtype=np.float64).reshape(-1)
    N = y.shape[0]
    mu, var = np.empty(N), np.empty(N)
    for i in range(N):
        keep = np.arange(N) != i
        L = np.linalg.cholesky(Ky[np.ix_(keep, keep)])
        k = Ky[keep, i]
        v = np.linalg.solve(L, k)
        mu[i] = v @ np.linalg.solve(L, y[keep])
        var[i] = Ky[i, i] - v @ v                     # K_y's diagonal carries the noise: the variance of y_i, not of f_i
    logp = _logp(y, mu, var)
    return {"mu": mu, "var": var, "logp": logp, "loo": float(np.sum(logp))}


def brute(X, y, r, sigma, l, noise):
    X = np.asarray(X, dtype=np.float64)
    return brute_from_Ky(R.kernel(X, r, sigma, l) + noise * np.eye(X.shape[0]), y)
