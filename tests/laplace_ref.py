"""NumPy float64 restatement of the GPU Laplace classifier (gpmi_laplace_fit / gpmi_laplace_predict_resident),
line for line: GPML Algorithms 3.1 and 3.2 with the logistic likelihood, labels +-1, the step-halving rule and the
prediction's composite trapezoid rule.  Test infrastructure only."""
import math

import numpy as np
from scipy.linalg import cholesky, solve_triangular


def rbf(a, b, sigma, l, chunk=512):
    """sigma**2 * exp(-.5/l**2 * sqdist) with sqdist from exact differences"""
    a = np.asarray(a, dtype=np.float64)
    b = np.asarray(b, dtype=np.float64)
    out = np.empty((a.shape[0], b.shape[0]))
    for r0 in range(0, a.shape[0], chunk):
        d = a[r0:r0 + chunk, None, :] - b[None, :, :]
        out[r0:r0 + chunk] = sigma ** 2 * np.exp(-.5 / l ** 2 * np.einsum("ijk,ijk->ij", d, d))
    return out


def expit(f):
    out = np.empty_like(f)
    pos = f >= 0
    out[pos] = 1.0 / (1.0 + np.exp(-f[pos]))
    e = np.exp(f[~pos])
    out[~pos] = e / (1.0 + e)
    return out


def log_p(y, f):
    """log p(y|f) = -softplus(-y f), overflow-safe"""
    z = -y * f
    return -(np.maximum(z, 0.0) + np.log1p(np.exp(-np.abs(z))))


def newton_state(y, a, f):
    """step 3: pi, W, s = sqrt(W), grad, b and Psi(a, f) = -a^T f / 2 + sum log p(y|f)"""
    t = (y + 1) / 2
    pi = expit(f)
    W = pi * (1 - pi)
    s = np.sqrt(W)
    grad = t - pi
    b = W * f + grad
    psi = -0.5 * (a @ f) + log_p(y, f).sum()
    return dict(pi=pi, W=W, s=s, grad=grad, b=b, psi=psi)


def laplace_fit(X, y, sigma, l, tol=1e-10, max_iter=100, K=None, max_halvings=20):
    """-> dict(log_q, f, grad, s, L, iters, converged, K, psi, halvings, decisions): halvings[k] is the number of
    halved steps and decisions[k] the list of (d, thr) of every accept / halve decision taken after Newton step k + 1"""
    y = np.asarray(y, dtype=np.float64)
    K = rbf(X, X, sigma, l) if K is None else K                  # 1.
    N = y.shape[0]
    a = np.zeros(N)
    a_prev = f_prev = None
    psi_prev = None
    iters, converged = 0, False
    halved, decisions = [], []
    while True:
        f = K @ a                                                # 2.
        st = newton_state(y, a, f)                               # 3.
        if psi_prev is not None:                                 # 4.
            halvings = 0
            halved.append(0)
            decisions.append([])
            while True:
                d = st["psi"] - psi_prev
                thr = tol * max(1.0, abs(st["psi"]))
                halved[-1] = halvings
                decisions[-1].append((d, thr))
                if abs(d) <= thr:
                    converged = True
                    break
                if d < -thr and halvings < max_halvings:
                    a = (a + a_prev) / 2
                    f = (f + f_prev) / 2
                    st = newton_state(y, a, f)
                    halvings += 1
                    continue
                break
        s = st["s"]
        u = K @ st["b"]                                          # 5.
        B = np.eye(N) + np.outer(s, s) * K
        L = cholesky(B, lower=True)                              # 6.
        m = solve_triangular(L, s * u, lower=True)
        if converged or iters >= max_iter:
            break
        x = solve_triangular(L.T, m, lower=False)                # 7.
        a_prev, f_prev, psi_prev = a, f, st["psi"]
        a = st["b"] - s * x
        iters += 1
    log_q = st["psi"] - np.log(np.diag(L)).sum()
    return dict(log_q=log_q, f=f, grad=st["grad"], s=s, L=L, iters=iters, converged=converged, K=K, psi=st["psi"],
                halvings=halved, decisions=decisions)


QUAD_T = 8.5


def quad_nodes(sig2):
    """the composite trapezoid rule of the prediction (laplace.hip: laplace_quad_nodes) -> (t, w)"""
    step = 0.25
    if sig2 > 0:
        a = 0.9 * math.pi / math.sqrt(sig2)
        if a < 8 * math.pi:
            step = min(0.25, 2 * math.pi * a / (36.0 + 0.5 * a * a))
    M = int(min(math.ceil(2 * QUAD_T / step), 1e8))
    h = 2 * QUAD_T / M
    t = -QUAD_T + np.arange(M + 1) * h
    w = h * 0.39894228040143267794 * np.exp(-0.5 * t * t)
    w[0] *= 0.5
    w[-1] *= 0.5
    return t, w


def expit_gauss(mu, var, sig2):
    """int expit(z) N(z | mu, var) dz for each (mu, var), var <= sig2"""
    t, w = quad_nodes(sig2)
    sd = np.sqrt(np.maximum(np.asarray(var, dtype=np.float64), 0.0))
    z = np.asarray(mu, dtype=np.float64)[:, None] + sd[:, None] * t[None, :]
    return expit(z.ravel()).reshape(z.shape) @ w


def laplace_predict(fit, X, Xs, sigma, l):
    """-> (f_mean, f_var, prob, label)"""
    R = rbf(Xs, X, sigma, l)
    f_mean = R @ fit["grad"]
    v = solve_triangular(fit["L"], (R * fit["s"]).T, lower=True)
    f_var = sigma ** 2 - np.sum(v ** 2, axis=0)
    prob = expit_gauss(f_mean, f_var, sigma ** 2)
    return f_mean, f_var, prob, np.where(f_mean >= 0, 1, -1)
