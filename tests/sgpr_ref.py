"""NumPy mirror of sparse GP regression with m inducing inputs Z (VFE: Titsias 2009; FITC: Snelson & Ghahramani 2006; GPML
chapter 8) in the whitened form the device uses:

    L = chol(K_uu + j I),  A = L^-1 K_uf (m x N),  q_i = |A[:, i]|^2,
    Lambda_i = s (VFE)  or  s + sigma^2 - q_i (FITC),  A~ = A Lambda^-1/2,  y~ = Lambda^-1/2 y,
    B = I + A~ A~^T,  L_B = chol(B),  c = L_B^-1 A~ y~
    value = -N/2 log 2 pi - sum log diag L_B - 1/2 sum log Lambda_i - 1/2 y~^T y~ + 1/2 c^T c
            [VFE only: - sum_i (sigma^2 - q_i) / (2 s)]
    prediction at x*: v1 = L^-1 k_u*, v2 = L_B^-1 v1, mean = v2^T c, var = sigma^2 - |v1|^2 + |v2|^2

`fit` evaluates it in float64 (LAPACK) or -- dtype=np.longdouble -- with the hand-written Cholesky and substitution
below, which run in any NumPy float type.  `dense` states the same quantities from the N x N matrix Q_ff + Lambda, the
definition the whitened form is checked against.  Test infrastructure: small m and N only.
"""
import numpy as np

SIGMA, ELL, JITTER = 1.2, 1.3, 1e-6
# (N, d, m, noise): m below one tile, at exactly one tile, just over one tile; N no multiple of 128
CASES = [(300, 5, 64, 5e-4), (257, 8, 130, 5e-4), (130, 2, 40, 1e-2), (641, 5, 128, 5e-4), (300, 2, 128, 1e-2)]
MID = (1500, 8, 384, 5e-4)       # several tiles


def inducing(X, m, seed=0):
    """a seeded random subset of the rows of X, in their order in X"""
    idx = np.sort(np.random.default_rng(seed).choice(X.shape[0], size=m, replace=False))
    return np.ascontiguousarray(X[idx])


def kernel(A, B, sigma, l):
    """sigma^2 exp(-.5 / l^2 |a - b|^2), the squared distance added one dimension after the other"""
    sq = np.zeros((A.shape[0], B.shape[0]), dtype=A.dtype)
    for k in range(A.shape[1]):
        sq += (A[:, k][:, None] - B[:, k][None, :]) ** 2
    return sigma ** 2 * np.exp(-sq / (2 * l ** 2))


def chol_plain(A):
    """lower Cholesky factor, column by column, in A's dtype"""
    n = A.shape[0]
    L = np.zeros_like(A)
    for j in range(n):
        dj = A[j, j] - L[j, :j] @ L[j, :j]
        if not dj > 0:
            raise np.linalg.LinAlgError("pivot %d is not positive" % (j + 1))
        L[j, j] = np.sqrt(dj)
        if j + 1 < n:
            L[j + 1:, j] = (A[j + 1:, j] - L[j + 1:, :j] @ L[j, :j]) / L[j, j]
    return L


def solve_lower_plain(L, Bm):
    """L^-1 Bm by forward substitution, in L's dtype; Bm a vector or a matrix"""
    X = np.array(Bm, dtype=L.dtype, copy=True)
    for i in range(L.shape[0]):
        if i:
            X[i] -= L[i, :i] @ X[:i]
        X[i] /= L[i, i]
    return X


def _ops(dtype):
    if dtype == np.float64:
        from scipy.linalg import solve_triangular
        return np.linalg.cholesky, lambda L, Bm: solve_triangular(L, Bm, lower=True)
    return chol_plain, solve_lower_plain


def fit(X, y, Z, sigma, l, noise, jitter=JITTER, method="vfe", Xs=None, dtype=np.float64):
    """-> dict: value, terms (the signed terms whose sum it is), scale (the sum of their absolute values), c, q, cond
    (of K_uu + j I, float64), and mean / var at Xs when given"""
    assert method in ("vfe", "fitc")
    X, y, Z = (np.asarray(a, dtype=dtype) for a in (X, y, Z))
    sigma, l, noise, jitter = (dtype(v) for v in (sigma, l, noise, jitter))
    chol, solve_lower = _ops(dtype)
    N, m = X.shape[0], Z.shape[0]
    Kuu = kernel(Z, Z, sigma, l) + jitter * np.eye(m, dtype=dtype)
    L = chol(Kuu)
    A = solve_lower(L, kernel(Z, X, sigma, l))
    q = np.sum(A * A, axis=0)
    lam = (noise + sigma ** 2) - q if method == "fitc" else np.full(N, noise, dtype=dtype)
    if not np.all(lam > 0):
        raise np.linalg.LinAlgError("Lambda is not positive")
    At = A / np.sqrt(lam)
    yt = y / np.sqrt(lam)
    LB = chol(np.eye(m, dtype=dtype) + At @ At.T)
    c = solve_lower(LB, At @ yt)
    half = dtype(0.5)
    terms = [-half * N * np.log(2 * dtype(np.pi)), -np.sum(np.log(np.diag(LB))), -half * np.sum(np.log(lam)),
             -half * (yt @ yt), half * (c @ c)]
    if method == "vfe":
        terms.append(-np.sum(sigma ** 2 - q) / (2 * noise))
    out = {"value": sum(terms), "terms": terms, "scale": sum(abs(t) for t in terms), "c": c, "q": q,
           "cond": float(np.linalg.cond(np.asarray(Kuu, dtype=np.float64)))}
    if Xs is not None:
        v1 = solve_lower(L, kernel(Z, np.asarray(Xs, dtype=dtype), sigma, l))
        v2 = solve_lower(LB, v1)
        out["mean"] = v2.T @ c
        out["var"] = (sigma ** 2 - np.sum(v1 * v1, axis=0)) + np.sum(v2 * v2, axis=0)
    return out


def dense(X, y, Z, sigma, l, noise, jitter=JITTER, method="vfe", Xs=None):
    """The same from the dense definition: Q_ff = K_fu (K_uu + j I)^-1 K_uf, C = Q_ff + Lambda (N x N),
    log N(y | 0, C) (minus the trace term tr(K_ff - Q_ff) / (2 s) for VFE), and the prediction
    mean = Q_*f C^-1 y,  var = sigma^2 - Q_** + Q_** - Q_*f C^-1 Q_f* = sigma^2 - Q_*f C^-1 Q_f*."""
    X, y, Z = (np.asarray(a, dtype=np.float64) for a in (X, y, Z))
    N, m = X.shape[0], Z.shape[0]
    Kuu = kernel(Z, Z, sigma, l) + jitter * np.eye(m)
    Kuf = kernel(Z, X, sigma, l)
    Qff = Kuf.T @ np.linalg.solve(Kuu, Kuf)
    lam = noise + sigma ** 2 - np.diag(Qff) if method == "fitc" else np.full(N, noise)
    Cm = Qff + np.diag(lam)
    Lc = np.linalg.cholesky(Cm)
    a = np.linalg.solve(Lc, y)
    value = -.5 * (a @ a) - np.sum(np.log(np.diag(Lc))) - .5 * N * np.log(2 * np.pi)
    trace = np.sum(sigma ** 2 - np.diag(Qff)) / (2 * noise)
    if method == "vfe":
        value -= trace
    out = {"value": value, "trace": trace}
    if Xs is not None:
        Ksu = kernel(np.asarray(Xs, dtype=np.float64), Z, sigma, l)
        Qsf = Ksu @ np.linalg.solve(Kuu, Kuf)
        W = np.linalg.solve(Lc, Qsf.T)
        out["mean"] = W.T @ a
        out["var"] = sigma ** 2 - np.sum(W * W, axis=0)
    return out
