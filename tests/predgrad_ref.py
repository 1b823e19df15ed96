"""Plain mirror of the gradients of the predictive mean and variance with respect to the test inputs
(include/gpmi.h: gpmi_predict_grad_resident), in a chosen dtype.  With z = x / r, k_j = k(z*, z_j), alpha = K_y^-1 y,
v = L^-1 k and w = L^-T v:

    mu = sum_j alpha_j k_j              dmu/dx*_k  =      sum_j alpha_j D_jk
    var = sigma^2 - v.v                 dvar/dx*_k = -2 * sum_j w_j D_jk
    D_jk = -k_j (z*_k - z_jk) / (l^2 r_k)                     kind 'rbf'
         = -sigma^2 a^2 H(t_j) (z*_k - z_jk) / r_k            the Matern kinds (a, t, H: tests/matern_ref.py)

an element with sq_j == 0 contributing 0.  Every sum cancels: beside the four results the mirror returns the scales

    S_mu[i, k] = sum_j |alpha_j D_jk|        S_var[i, k] = 2 sum_j |w_j D_jk|

and an error is ALWAYS |got - ref| / S, elementwise, maximum over the case (err()): on the problems of the tests
S_var / |dvar| reaches 1e7, so a plain relative error says nothing.

The squared-exponential fit is predict_ref.fit; a Matern fit is the same statements with matern_ref's covariance in the
dtype; the inputs are scaled by ard_ref.scaled (one float64 division per element, what the device forms).  `broken`
breaks the mirror on purpose for the tests' own check: "no_r" drops the 1 / r_k from D, "w_is_v" takes v for w.

Test infrastructure: dense matrices, small N only."""
import numpy as np

import ard_ref as R
import matern_ref as M
import predict_ref as P
import sgpr_ref as S

KINDS = ("rbf", "matern12", "matern32", "matern52")
NU = {"matern12": 0.5, "matern32": 1.5, "matern52": 2.5}


def _kh(kind, sq, sigma, l, dtype):
    """-> (K, G): the covariance and G with D_jk = -G e_k / r_k, both from the squared distance of scaled inputs"""
    sigma, l = dtype(sigma), dtype(l)
    if kind == "rbf":
        K = sigma ** 2 * np.exp(dtype(-.5) / l ** 2 * sq)
        return K, K / l ** 2
    nu = NU[kind]
    a = np.sqrt(dtype(2.0 * nu)) / abs(l)
    t = a * np.sqrt(sq)
    e = np.exp(-t)
    if nu == 0.5:
        Pt = np.ones_like(t)
        with np.errstate(divide="ignore", invalid="ignore"):
            H = np.where(t > 0, e / np.where(t > 0, t, dtype(1)), dtype(0))
    elif nu == 1.5:
        Pt, H = 1 + t, e
    else:
        Pt, H = 1 + t + t * t / dtype(3), (1 + t) * e / dtype(3)
    return sigma ** 2 * (Pt * e), sigma ** 2 * a * a * H


def _sq(za, zb, dtype):
    za, zb = za.astype(dtype), zb.astype(dtype)
    sq = np.zeros((za.shape[0], zb.shape[0]), dtype=dtype)
    for k in range(za.shape[1]):
        sq += (za[:, None, k] - zb[None, :, k]) ** 2
    return sq


def fit(X, y, r, kind, sigma, l, noise, dtype=np.float64):
    """-> dict: L, m, alpha and the inputs a prediction needs (predict_ref.fit for 'rbf', its statements for a Matern)"""
    assert kind in KINDS
    r = np.ones(np.asarray(X).shape[1]) if r is None else np.asarray(r, dtype=np.float64)
    if kind == "rbf":
        f = P.fit(X, y, r, sigma, l, noise, dtype)
    else:
        chol, solve_lower = S._ops(dtype)
        z = R.scaled(X, r)
        N = len(z)
        K, _ = _kh(kind, _sq(z, z, dtype), sigma, l, dtype)
        L = chol(K + dtype(noise) * np.eye(N, dtype=dtype))
        m = solve_lower(L, np.asarray(y, dtype=dtype))
        f = dict(L=L, m=m, alpha=P.solve_upper_t(solve_lower, L, m), z=z, r=r, sigma=sigma, l=l, dtype=dtype)
    f["kind"] = kind
    return f


def mean_var(f, Xs):
    """mu and var alone (the central differences of the CPU test evaluate nothing else)"""
    dtype = f["dtype"]
    _, solve_lower = S._ops(dtype)
    zs = np.asarray(Xs, dtype=dtype) / np.asarray(f["r"], dtype=dtype) if dtype != np.float64 else R.scaled(Xs, f["r"])
    K, _ = _kh(f["kind"], _sq(np.asarray(f["z"]), np.asarray(zs), dtype), f["sigma"], f["l"], dtype)      # N x n
    v = solve_lower(f["L"], K)
    return v.T @ f["m"], dtype(f["sigma"]) ** 2 - np.sum(v * v, axis=0)


def predict_grad(f, Xs, broken=None):
    """-> dict: mu (n,), var (n,), dmu, dvar, S_mu, S_var (n, d) in the fit's dtype"""
    assert broken in (None, "no_r", "w_is_v")
    dtype = f["dtype"]
    _, solve_lower = S._ops(dtype)
    z = np.asarray(f["z"]).astype(dtype)
    zs = R.scaled(Xs, f["r"]).astype(dtype)
    r = np.asarray(f["r"]).astype(dtype)
    K, G = _kh(f["kind"], _sq(z, zs, dtype), f["sigma"], f["l"], dtype)                 # N x n
    v = solve_lower(f["L"], K)
    w = v if broken == "w_is_v" else np.stack([P.solve_upper_t(solve_lower, f["L"], v[:, i]) for i in range(v.shape[1])], 1)
    n, d = zs.shape
    out = dict(mu=v.T @ f["m"], var=dtype(f["sigma"]) ** 2 - np.sum(v * v, axis=0))
    dmu, dvar, S_mu, S_var = (np.zeros((n, d), dtype=dtype) for _ in range(4))
    alpha = f["alpha"]
    for k in range(d):
        rk = dtype(1) if broken == "no_r" else r[k]
        D = -G * (zs[None, :, k] - z[:, None, k]) / rk                                  # N x n: D[j, i]
        dmu[:, k] = alpha @ D
        dvar[:, k] = -2 * np.sum(w * D, axis=0)
        S_mu[:, k] = np.abs(alpha) @ np.abs(D)
        S_var[:, k] = 2 * np.sum(np.abs(w * D), axis=0)
    out.update(dmu=dmu, dvar=dvar, S_mu=S_mu, S_var=S_var)
    return out


def err(got, ref, scale):
    """max over the case of |got - ref| / S, in float64"""
    g, rf, s = (np.asarray(a, dtype=np.longdouble) for a in (got, ref, scale))
    return float(np.max(np.abs(g - rf) / s))


def problem(N, d, n, seed, lengthscales=False, coincide=True):
    """Training inputs uniform in [-2, 2]^d with a smooth target, n test points of which a third lie outside the training
    box (in [2, 2.6]) and -- coincide -- the last one IS a training point; r: relative lengthscales in [0.6, 1.7] or None"""
    rng = np.random.RandomState(seed)
    X = rng.uniform(-2, 2, size=(N, d))
    y = np.sin(X.sum(1)) + 0.3 * np.cos(1.7 * X[:, 0]) + 0.05 * rng.standard_normal(N)
    Xs = rng.uniform(-2, 2, size=(n, d))
    out = np.arange(n) % 3 == 1
    Xs[out] = rng.uniform(2.0, 2.6, size=(int(out.sum()), d))
    if coincide and n >= 1:
        Xs[n - 1] = X[N // 2]
    r = rng.uniform(0.6, 1.7, size=d) if lengthscales else None
    return X, y, Xs, r
