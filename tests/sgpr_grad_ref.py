"""NumPy mirror of the gradient of the collapsed variational bound (VFE) of sparse GP regression, in the notation of
tests/sgpr_ref.py and of gpmi_sparse_grad (include/gpmi.h): s = noise, j = jitter, z = x / r, K0_uu = K_uu without j,

    u = L_B^-T c,  p = L^-T u,  T = L^-T (I - B^-1) L^-1 / s,  beta = (y - K_fu p) / s
    D_fu = K_fu T + beta p^T,  D_uu = -1/2 L^-T (B - 2 I + B^-1 + u u^T) L^-1,  G_fu = D_fu o K_fu,  G_uu = D_uu o K0_uu
    dF/dsigma = (2 / sigma) (sum G_fu + sum G_uu) - N sigma / s
    dF/dl     = (sum G_fu,ij |z_i - z_j|^2 + sum G_uu,jj' |z_j - z_j'|^2) / l^3
    dF/dr_k   = (sum G_fu,ij (z_ik - z_jk)^2 + sum G_uu,jj' (z_jk - z_j'k)^2) / (l^2 r_k)
    dF/ds     = -(N - m + tr B^-1) / (2 s) + 1/2 beta^T beta + sum_i (sigma^2 - q_i) / (2 s^2)
    dF/dZ_jk  = (sum_i G_fu,ij (z_ik - z_jk) + 2 sum_j' G_uu,jj' (z_j'k - z_jk)) / (l^2 r_k)      [the raw Z]

`grad` evaluates them in float64 (LAPACK) or -- dtype=np.longdouble -- with the plain Cholesky and substitution of
sgpr_ref.py, and returns with every component g_* its cancellation scale s_*: the sum of the absolute values of the
terms added (the construction of ard_ref.py).  Test infrastructure: small m and N only.
"""
import numpy as np

import sgpr_ref as S


def grad(X, y, Z, sigma, l, noise, r=None, jitter=S.JITTER, dtype=np.float64):
    """-> dict: value, and g_x / s_x for x in l, sigma, noise (scalars), r (d,), Z (m, d)"""
    X, y, Z = (np.asarray(a, dtype=dtype) for a in (X, y, Z))
    N, d = X.shape
    m = Z.shape[0]
    r = np.ones(d, dtype=dtype) if r is None else np.asarray(r, dtype=dtype)
    sigma, l, s, jitter = (dtype(v) for v in (sigma, l, noise, jitter))
    half, two = dtype(0.5), dtype(2)
    chol, solve_lower = S._ops(dtype)
    x, z = X / r, Z / r
    eye = np.eye(m, dtype=dtype)
    K0uu = S.kernel(z, z, sigma, l)
    Kfu = S.kernel(x, z, sigma, l)
    L = chol(K0uu + jitter * eye)
    A = solve_lower(L, Kfu.T)
    q = np.sum(A * A, axis=0)
    At, yt = A / np.sqrt(s), y / np.sqrt(s)
    LB = chol(eye + At @ At.T)
    c = solve_lower(LB, At @ yt)
    terms = [-half * N * np.log(two * dtype(np.pi)), -np.sum(np.log(np.diag(LB))), -half * N * np.log(s),
             -half * (yt @ yt), half * (c @ c), -np.sum(sigma ** 2 - q) / (two * s)]
    Li, LBi = solve_lower(L, eye), solve_lower(LB, eye)
    u = LBi.T @ c
    p = Li.T @ u
    Binv = LBi.T @ LBi
    B = LB @ LB.T
    T = Li.T @ (eye - Binv) @ Li / s
    beta = (y - Kfu @ p) / s
    Duu = -half * (Li.T @ (B - two * eye + Binv + np.outer(u, u)) @ Li)
    Gfu = (Kfu @ T + np.outer(beta, p)) * Kfu
    Guu = Duu * K0uu
    out = {"value": sum(terms)}

    sg = [np.sum(Gfu), np.sum(Guu), -N * sigma / s]
    out["g_sigma"] = (two / sigma) * (sg[0] + sg[1]) + sg[2]
    out["s_sigma"] = (two / sigma) * (np.sum(np.abs(Gfu)) + np.sum(np.abs(Guu))) + abs(sg[2])

    g_r, s_r = np.empty(d, dtype=dtype), np.empty(d, dtype=dtype)
    g_Z, s_Z = np.empty((m, d), dtype=dtype), np.empty((m, d), dtype=dtype)
    sq_fu, sq_uu = np.zeros((N, m), dtype=dtype), np.zeros((m, m), dtype=dtype)
    for k in range(d):
        dfu = x[:, k][:, None] - z[:, k][None, :]          # z_ik - z_jk
        duu = z[:, k][:, None] - z[:, k][None, :]          # z_j'k - z_jk, rows j'
        sq_fu += dfu * dfu
        sq_uu += duu * duu
        a, b = Gfu * dfu * dfu, Guu * duu * duu
        g_r[k] = (np.sum(a) + np.sum(b)) / (l ** 2 * r[k])
        s_r[k] = (np.sum(np.abs(a)) + np.sum(np.abs(b))) / (l ** 2 * r[k])
        a, b = Gfu * dfu, Guu * duu
        g_Z[:, k] = (np.sum(a, axis=0) + two * np.sum(b, axis=0)) / (l ** 2 * r[k])
        s_Z[:, k] = (np.sum(np.abs(a), axis=0) + two * np.sum(np.abs(b), axis=0)) / (l ** 2 * r[k])
    out["g_r"], out["s_r"], out["g_Z"], out["s_Z"] = g_r, s_r, g_Z, s_Z
    a, b = Gfu * sq_fu, Guu * sq_uu                        # the whole squared distance: sum_k r_k dF/dr_k = l dF/dl
    out["g_l"] = (np.sum(a) + np.sum(b)) / l ** 3
    out["s_l"] = (np.sum(np.abs(a)) + np.sum(np.abs(b))) / l ** 3

    tn = [-(N - m + np.trace(Binv)) / (two * s), half * (beta @ beta), np.sum(sigma ** 2 - q) / (two * s ** 2)]
    out["g_noise"], out["s_noise"] = sum(tn), sum(abs(t) for t in tn)
    return out
