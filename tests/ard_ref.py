"""Dense NumPy float64 mirror of the squared-exponential GP with one lengthscale per input dimension (ARD):

    K_ij = sigma^2 exp(-.5 / l^2 * sum_k ((x_ik - x_jk) / r_k)^2),     K_y = K + noise I

the log marginal likelihood as oracle/gp_oracle.py states it, and its d + 3 derivatives from the explicit inverse,

    dLML/dtheta = .5 tr((alpha alpha^T - K_y^-1) dK_y/dtheta),        alpha = K_y^-1 y

each with the scale at which its two terms cancel, .5 |alpha^T D alpha| + .5 |sum K_y^-1 o D| (the construction of
_grad_scale in tests/test_parity_gpu.py).  Test infrastructure: dense N x N matrices, small N only.
"""
import numpy as np


def scaled(X, r):
    """z = X / r, the one division per element the device performs"""
    return np.asarray(X, dtype=np.float64) / np.asarray(r, dtype=np.float64)


def sq_parts(X, r):
    """(N, N, d): ((x_ik - x_jk) / r_k)^2 from the scaled inputs"""
    z = scaled(X, r)
    return (z[:, None, :] - z[None, :, :]) ** 2


def kernel(X, r, sigma, l):
    return sigma ** 2 * np.exp(-.5 / l ** 2 * sq_parts(X, r).sum(-1))


def lml(X, y, r, sigma, l, noise):
    N = X.shape[0]
    L = np.linalg.cholesky(kernel(X, r, sigma, l) + noise * np.eye(N))
    m = np.linalg.solve(L, y)
    return -.5 * (m @ m) - np.sum(np.log(np.diag(L))) - .5 * N * np.log(2 * np.pi)


def lml_and_grad(X, y, r, sigma, l, noise):
    """-> dict: lml, alpha, Kinv, and for 'r' (d,), 'l', 'sigma', 'noise' the derivative g_* and its cancellation
    scale s_*"""
    X = np.asarray(X, dtype=np.float64)
    y = np.asarray(y, dtype=np.float64).reshape(-1)
    r = np.asarray(r, dtype=np.float64).reshape(-1)
    N, d = X.shape
    z = scaled(X, r)
    part = lambda k: (z[:, None, k] - z[None, :, k]) ** 2      # noqa: E731  (one dimension at a time: N^2 memory)
    sq = np.zeros((N, N))
    for k in range(d):
        sq += part(k)
    K = sigma ** 2 * np.exp(-.5 / l ** 2 * sq)
    Ky = K + noise * np.eye(N)
    L = np.linalg.cholesky(Ky)
    Kinv = np.linalg.inv(Ky)
    Kinv = .5 * (Kinv + Kinv.T)
    alpha = Kinv @ y
    m = np.linalg.solve(L, y)
    out = {"lml": -.5 * (m @ m) - np.sum(np.log(np.diag(L))) - .5 * N * np.log(2 * np.pi), "alpha": alpha, "Kinv": Kinv}

    def both(D):
        a, b = .5 * (alpha @ D @ alpha), .5 * np.sum(Kinv * D)
        return a - b, abs(a) + abs(b)

    g_r, s_r = np.empty(d), np.empty(d)
    for k in range(d):
        g_r[k], s_r[k] = both(K * part(k) / (l ** 2 * r[k]))
    out["g_r"], out["s_r"] = g_r, s_r
    out["g_l"], out["s_l"] = both(K * sq / l ** 3)
    out["g_sigma"], out["s_sigma"] = both(2 * K / sigma)
    out["g_noise"], out["s_noise"] = both(np.eye(N))
    return out


def problem(N, d, seed, relevant=None):
    """inputs uniform in [0, 4), a smooth target of the first `relevant` dimensions (default all) plus a little noise"""
    rng = np.random.default_rng(seed)
    X = rng.uniform(0.0, 4.0, size=(N, d))
    k = d if relevant is None else relevant
    y = np.sin(X[:, :k].sum(1)) + 0.05 * rng.standard_normal(N)
    return X, y
