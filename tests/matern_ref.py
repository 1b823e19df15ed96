"""Dense NumPy float64 mirror of the Matern covariance functions nu = 1/2, 3/2, 5/2 (kinds 4, 5, 6 of include/gpmi.h;
Rasmussen & Williams, GPML, section 4.2.1) with one lengthscale per input dimension, on the problems of tests/ard_ref.py:

    K_ij = sigma^2 P(t) exp(-t),   t = a sqrt(sq_ij),   a = sqrt(2 nu) / |l|,   sq_ij = sum_k ((x_ik - x_jk) / r_k)^2
    P = 1,  1 + t,  1 + t + t^2 / 3

kernel() follows the header's evaluation order operation for operation (sq summed over the middle axis of the (N, d, M)
differences as oracle/gp_oracle.py's RBF_kernel does, r = sqrt(sq), t = a * r, P = 1 + t or (1 + t) + (t * t) * c3,
K = sigma^2 * (P * exp(-t))), so that only exp itself can differ from the device.  The log marginal likelihood, its
d + 3 derivatives

    dLML/dtheta = .5 tr((alpha alpha^T - K_y^-1) dK_y/dtheta),   dK/dl = sigma^2 a^2 H(t) sq / l,
    dK/dr_k = sigma^2 a^2 H(t) ((x_ik - x_jk) / r_k)^2 / r_k,    H = e^-t / t,  e^-t,  (1 + t) e^-t / 3

(H(t) sq is 0 where sq == 0: a select, not a division), each with the scale at which its two terms cancel (the
construction of ard_ref.lml_and_grad), and leave-one-out with its gradient (the closed forms of tests/loo_ref.py).
Test infrastructure: dense N x N matrices, small N only.
"""
import numpy as np

import ard_ref as R
import loo_ref as LR

NUS = (0.5, 1.5, 2.5)
KIND = {0.5: "matern12", 1.5: "matern32", 2.5: "matern52"}
C3 = 1.0 / 3.0           # the double nearest 1/3


def duplicate_rows(X, y, pairs):
    """copies of (X, y) in which row i repeats row j exactly for every (i, j): a repeated measurement, its target the
    other's plus 0.03 (targets that contradicted each other would put 1 / noise into alpha and the conditioning of the
    problem into every comparison)"""
    X, y = np.array(X, dtype=np.float64), np.array(y, dtype=np.float64)
    for i, j in pairs:
        X[i] = X[j]
        y[i] = y[j] + 0.03
    return X, y


def a_of(nu, l):
    """sqrt(2 nu) / |l| in double: sqrt(1.0), sqrt(3.0), sqrt(5.0) are correctly rounded"""
    return np.sqrt(np.float64(2.0 * nu)) / abs(np.float64(l))


def sq_cross(A, B):
    """sum_k (a_ik - b_jk)^2 in the order the device reproduces (oracle/gp_oracle.py: RBF_kernel)"""
    A = np.ascontiguousarray(A, dtype=np.float64)
    B = np.ascontiguousarray(B, dtype=np.float64)
    return ((A[:, :, None] - B[:, :, None].T) ** 2).sum(1)


def P_of(nu, t):
    if nu == 0.5:
        return np.ones_like(t)
    if nu == 1.5:
        return 1.0 + t
    if nu == 2.5:
        return (1.0 + t) + (t * t) * C3
    raise ValueError(nu)


def H_of(nu, t, e):
    """-(1/t) d(P e^-t)/dt; the nu = 1/2 singularity at t = 0 is selected to 0 (it only ever multiplies sq = 0)"""
    if nu == 0.5:
        with np.errstate(divide="ignore", invalid="ignore"):
            return np.where(t > 0.0, e / np.where(t > 0.0, t, 1.0), 0.0)
    if nu == 1.5:
        return e
    return (1.0 + t) * e * C3


def kernel_cross(A, B, nu, sigma, l):
    """K(A, B) on inputs that are already scaled, in the header's evaluation order"""
    t = a_of(nu, l) * np.sqrt(sq_cross(A, B))
    return (np.float64(sigma) * np.float64(sigma)) * (P_of(nu, t) * np.exp(-t))


def kernel(X, r, nu, sigma, l):
    z = R.scaled(X, r)
    return kernel_cross(z, z, nu, sigma, l)


def lml(X, y, r, nu, sigma, l, noise):
    N = X.shape[0]
    L = np.linalg.cholesky(kernel(X, r, nu, sigma, l) + noise * np.eye(N))
    m = np.linalg.solve(L, np.asarray(y, dtype=np.float64).reshape(-1))
    return -.5 * (m @ m) - np.sum(np.log(np.diag(L))) - .5 * N * np.log(2 * np.pi)


def lml_long(X, y, r, nu, sigma, l, noise):
    """the same LML with every operation in long double (the central differences of the CPU tests)"""
    ld = np.longdouble
    z = np.asarray(X, dtype=ld) / np.asarray(r, dtype=ld)
    N = z.shape[0]
    sq = ((z[:, None, :] - z[None, :, :]) ** 2).sum(-1)
    t = np.sqrt(ld(2.0 * nu)) / abs(ld(l)) * np.sqrt(sq)
    P = {0.5: ld(1.0) + 0 * t, 1.5: 1 + t, 2.5: 1 + t + t * t / ld(3.0)}[nu]
    Ky = ld(sigma) ** 2 * P * np.exp(-t) + ld(noise) * np.eye(N, dtype=ld)
    L = np.zeros((N, N), dtype=ld)             # np.linalg has no long double: Cholesky-Banachiewicz by rows
    for i in range(N):
        for j in range(i):
            L[i, j] = (Ky[i, j] - L[i, :j] @ L[j, :j]) / L[j, j]
        L[i, i] = np.sqrt(Ky[i, i] - L[i, :i] @ L[i, :i])
    m = np.zeros(N, dtype=ld)
    yy = np.asarray(y, dtype=ld).reshape(-1)
    for i in range(N):
        m[i] = (yy[i] - L[i, :i] @ m[:i]) / L[i, i]
    return -(m @ m) / 2 - np.sum(np.log(np.diag(L))) - ld(N) / 2 * np.log(2 * ld(np.pi))


def _pieces(X, r, nu, sigma, l):
    z = R.scaled(X, r)
    N, d = z.shape
    part = lambda k: (z[:, None, k] - z[None, :, k]) ** 2      # noqa: E731
    sq = sq_cross(z, z)
    a = a_of(nu, l)
    t = a * np.sqrt(sq)
    e = np.exp(-t)
    K = (np.float64(sigma) * np.float64(sigma)) * (P_of(nu, t) * e)
    G = np.float64(sigma) ** 2 * a * a * H_of(nu, t, e)        # dK = G o (squared difference) / (its lengthscale)
    return part, sq, K, G


def lml_and_grad(X, y, r, nu, sigma, l, noise):
    """-> dict: lml, alpha, Kinv, and for 'r' (d,), 'l', 'sigma', 'noise' the derivative g_* and its cancellation
    scale s_* (ard_ref.lml_and_grad for a Matern)"""
    X = np.asarray(X, dtype=np.float64)
    y = np.asarray(y, dtype=np.float64).reshape(-1)
    r = np.asarray(r, dtype=np.float64).reshape(-1)
    N, d = X.shape
    part, sq, K, G = _pieces(X, r, nu, sigma, l)
    Ky = K + noise * np.eye(N)
    L = np.linalg.cholesky(Ky)
    Kinv = np.linalg.inv(Ky)
    Kinv = .5 * (Kinv + Kinv.T)
    alpha = Kinv @ y
    m = np.linalg.solve(L, y)
    out = {"lml": -.5 * (m @ m) - np.sum(np.log(np.diag(L))) - .5 * N * np.log(2 * np.pi), "alpha": alpha, "Kinv": Kinv,
           "cond": float(np.linalg.cond(Ky))}

    def both(D):
        p, q = .5 * (alpha @ D @ alpha), .5 * np.sum(Kinv * D)
        return p - q, abs(p) + abs(q)

    g_r, s_r = np.empty(d), np.empty(d)
    for k in range(d):
        g_r[k], s_r[k] = both(G * part(k) / r[k])
    out["g_r"], out["s_r"] = g_r, s_r
    out["g_l"], out["s_l"] = both(G * sq / l)
    out["g_sigma"], out["s_sigma"] = both(2 * K / sigma)
    out["g_noise"], out["s_noise"] = both(np.eye(N))
    return out


def loo_closed(X, y, r, nu, sigma, l, noise):
    """loo_ref.closed for a Matern: mu, var, logp, loo and g_l, g_sigma, g_noise with their cancellation scales"""
    X = np.asarray(X, dtype=np.float64)
    N = X.shape[0]
    _, sq, K, G = _pieces(X, np.asarray(r, dtype=np.float64).reshape(-1), nu, sigma, l)
    out = LR.from_Ky(K + noise * np.eye(N), y)
    Kinv, alpha, kappa = out["Kinv"], out["alpha"], out["kappa"]

    def both(dK):
        Z = Kinv @ dK
        rr = Z @ alpha
        s = np.sum(Z * Kinv, axis=1)
        p = alpha * rr / kappa
        q = .5 * (1.0 + alpha ** 2 / kappa) * s / kappa
        return float(np.sum(p - q)), float(np.sum(np.abs(p) + np.abs(q)))

    out["g_l"], out["s_l"] = both(G * sq / l)
    out["g_sigma"], out["s_sigma"] = both(2 * K / sigma)
    out["g_noise"], out["s_noise"] = both(np.eye(N))
    return out


def predict(X, y, Xs, r, nu, sigma, l, noise):
    """(mu, sd) at the test points: GP_regression.py:138-148 with the Matern kernel"""
    z, zs = R.scaled(X, r), R.scaled(Xs, r)
    N = z.shape[0]
    L = np.linalg.cholesky(kernel_cross(z, z, nu, sigma, l) + noise * np.eye(N))
    Ks = kernel_cross(z, zs, nu, sigma, l)
    alpha = np.linalg.solve(L.T, np.linalg.solve(L, np.asarray(y, dtype=np.float64).reshape(-1)))
    v = np.linalg.solve(L, Ks)
    var = np.float64(sigma) ** 2 - np.sum(v ** 2, axis=0)
    return Ks.T @ alpha, np.sqrt(var)
