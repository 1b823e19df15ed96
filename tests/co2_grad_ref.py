"""Dense NumPy mirror of GP regression under the CO2 composite kernel (CO2_example.py:9-90, kind 3 of the C-ABI):

    K = theta_1^2 e1 + theta_3^2 q2 + theta_6^2 p3 + theta_9^2 e4 + theta_11^2 I,     K_y = K + noise I
    e1 = exp(-sq / (2 theta_2^2))                  q2 = exp(-sq / (2 theta_4^2) - 2 sin^2(pi r) / theta_5^2)
    p3 = (1 + u)^-theta_8, u = sq / (2 theta_8 theta_7^2)          e4 = exp(-sq / (2 theta_10^2)),   r = sqrt(sq)

the log marginal likelihood as oracle/gp_oracle.py states it, and its twelve derivatives from the explicit inverse,

    dLML/dtheta = .5 tr((alpha alpha^T - K_y^-1) dK_y/dtheta),        alpha = K_y^-1 y

each with the scale at which its two terms cancel, .5 |alpha^T D alpha| + .5 |sum K_y^-1 o D| (the construction of
tests/ard_ref.py::lml_and_grad).  Every function takes the number format: np.float64 (LAPACK's Cholesky and inverse) or
np.longdouble (a hand-rolled Cholesky and inverse, N^3 interpreted-speed work: affordable up to N ~ 360).
Test infrastructure: dense N x N matrices, small N only.
"""
import numpy as np

# theta for inputs of more than one dimension: kernel_2 of the Euclidean norm is a valid covariance for d = 1 only, and
# with theta_5 = 1.1 the composite is indefinite at (N, d) = (1100, 3); theta_5 = 8 keeps it positive definite
THETA_MD = np.array([1.5, 1.2, 0.8, 2.0, 8.0, 0.7, 0.9, 1.3, 0.3, 0.5, 0.5])
NOISE = 5e-4


def _pi(dt):
    return np.pi if dt is np.float64 else 4 * np.arctan(dt(1))


def sqdist(X, dt=np.float64):
    X = np.asarray(X, dtype=dt)
    sq = np.zeros((X.shape[0], X.shape[0]), dtype=dt)
    for k in range(X.shape[1]):                                  # one dimension at a time: N^2 memory
        sq += (X[:, None, k] - X[None, :, k]) ** 2
    return sq


def parts(sq, th, dt=np.float64):
    """the four factors and what their derivatives need, in the reference's evaluation order (CO2_example.py:17-64)"""
    th = np.asarray(th, dtype=dt)
    r = np.sqrt(sq)
    e1 = np.exp(-.5 * sq / (th[1] * th[1]))
    sn = np.sin(_pi(dt) * r) / th[4]
    q2 = np.exp(-.5 * sq / (th[3] * th[3]) + -2 * (sn * sn))
    item = 1 + .5 * sq / (th[7] * (th[6] * th[6]))
    p3 = 1.0 / np.power(item, th[7])
    e4 = np.exp(-.5 * sq / (th[9] * th[9]))
    return e1, q2, p3, e4, item, np.sin(_pi(dt) * r) ** 2


def kernel(X, th, dt=np.float64):
    """covariance_function(X, X, th): square, so kernel_4 adds theta_11^2 on the diagonal (:58-64)"""
    th = np.asarray(th, dtype=dt)
    sq = sqdist(X, dt)
    e1, q2, p3, e4, _, _ = parts(sq, th, dt)
    k4 = (th[8] * th[8]) * e4 + (th[10] * th[10]) * np.eye(sq.shape[0], dtype=dt)
    return (((th[0] * th[0]) * e1 + (th[2] * th[2]) * q2) + (th[5] * th[5]) * p3) + k4


def cholesky(A, dt=np.float64):
    if dt is np.float64:
        return np.linalg.cholesky(A)
    # inner products by np.sum of the products (pairwise summation), not by `@` (one running sum)
    N = A.shape[0]
    L = np.zeros((N, N), dtype=dt)
    for j in range(N):
        v = A[j, j] - np.sum(L[j, :j] * L[j, :j])
        if not v > 0:
            raise np.linalg.LinAlgError("Matrix is not positive definite")
        L[j, j] = np.sqrt(v)
        if j + 1 < N:
            L[j + 1:, j] = (A[j + 1:, j] - np.sum(L[j + 1:, :j] * L[j, :j], axis=1)) / L[j, j]
    return L


def lower_inverse(L, dt=np.float64):
    if dt is np.float64:
        return np.linalg.inv(L)
    N = L.shape[0]
    X = np.zeros((N, N), dtype=dt)
    for i in range(N):
        row = -np.sum(L[i, :i, None] * X[:i, :], axis=0) if i else np.zeros(N, dtype=dt)
        row[i] += 1
        X[i, :] = row / L[i, i]
    return X


def _lml_from(L, m, dt):
    N = L.shape[0]
    return -.5 * (m @ m) - np.sum(np.log(np.diag(L))) - .5 * N * np.log(2 * _pi(dt))


def lml(X, y, th, noise=NOISE, dt=np.float64):
    y = np.asarray(y, dtype=dt).reshape(-1)
    Ky = kernel(X, th, dt) + dt(noise) * np.eye(len(y), dtype=dt)
    L = cholesky(Ky, dt)
    m = lower_inverse(L, dt) @ y if dt is not np.float64 else np.linalg.solve(L, y)
    return _lml_from(L, m, dt)


def lml_and_grad(X, y, th, noise=NOISE, dt=np.float64):
    """-> dict: lml, alpha, g_theta (11,), s_theta (11,), g_noise, s_noise (derivatives and cancellation scales)"""
    th = np.asarray(th, dtype=dt)
    y = np.asarray(y, dtype=dt).reshape(-1)
    N = len(y)
    sq = sqdist(X, dt)
    e1, q2, p3, e4, item, s2 = parts(sq, th, dt)
    eye = np.eye(N, dtype=dt)
    K = (((th[0] * th[0]) * e1 + (th[2] * th[2]) * q2) + (th[5] * th[5]) * p3) + ((th[8] * th[8]) * e4 + (th[10] * th[10]) * eye)
    Ky = K + dt(noise) * eye
    L = cholesky(Ky, dt)
    if dt is np.float64:
        Kinv = np.linalg.inv(Ky)
        m = np.linalg.solve(L, y)
    else:
        Li = lower_inverse(L, dt)
        Kinv = Li.T @ Li
        m = Li @ y
    Kinv = .5 * (Kinv + Kinv.T)
    alpha = Kinv @ y
    u = item - 1
    D = [2 * th[0] * e1,
         th[0] ** 2 * e1 * sq / th[1] ** 3,
         2 * th[2] * q2,
         th[2] ** 2 * q2 * sq / th[3] ** 3,
         4 * th[2] ** 2 * q2 * s2 / th[4] ** 3,
         2 * th[5] * p3,
         th[5] ** 2 * p3 * sq / (th[6] ** 3 * item),
         th[5] ** 2 * p3 * (u / item - np.log(item)),
         2 * th[8] * e4,
         th[8] ** 2 * e4 * sq / th[9] ** 3,
         2 * th[10] * eye,
         eye]
    g, s = np.empty(12, dtype=dt), np.empty(12, dtype=dt)
    for i, Di in enumerate(D):
        a, b = .5 * (alpha @ Di @ alpha), .5 * np.sum(Kinv * Di)
        g[i], s[i] = a - b, abs(a) + abs(b)
    return {"lml": _lml_from(L, m, dt), "alpha": alpha, "g_theta": g[:11], "s_theta": s[:11], "g_noise": g[11],
            "s_noise": s[11]}


def central_differences(X, y, th, noise=NOISE, rel_step=1e-6, dt=np.longdouble):
    """the twelve derivatives by central differences of lml, step rel_step * the parameter"""
    th = np.asarray(th, dtype=dt)
    out = np.empty(12, dtype=dt)
    for i in range(11):
        h = dt(rel_step) * th[i]
        e = np.zeros(11, dtype=dt)
        e[i] = h
        out[i] = (lml(X, y, th + e, noise, dt) - lml(X, y, th - e, noise, dt)) / (2 * h)
    h = dt(rel_step) * dt(noise)
    out[11] = (lml(X, y, th, dt(noise) + h, dt) - lml(X, y, th, dt(noise) - h, dt)) / (2 * h)
    return out


def problem_md(N, d, seed):
    """inputs uniform in [0, 4)^d / sqrt(d), a smooth target plus a little noise: positive definite with THETA_MD"""
    rng = np.random.default_rng(seed)
    X = rng.uniform(0.0, 4.0, size=(N, d)) / np.sqrt(d)
    y = np.sin(X.sum(1)) + 0.05 * rng.standard_normal(N)
    return X, y


def error_over_scale(got_theta, got_noise, ref):
    """(12,) float64: |got - ref| / cancellation scale, the noise component last.  A scale of exactly 0 (N = 1: every
    squared distance is 0, so the derivative matrix is) admits exactly 0 only: 0 there, inf otherwise."""
    g = np.concatenate([np.asarray(ref["g_theta"]), [ref["g_noise"]]])
    s = np.concatenate([np.asarray(ref["s_theta"]), [ref["s_noise"]]])
    got = np.concatenate([np.asarray(got_theta, dtype=g.dtype), [got_noise]])
    diff = np.abs(got - g)
    err = np.where(diff == 0, 0.0, np.inf)
    np.divide(diff, s, out=err, where=s > 0, casting="unsafe")
    return np.asarray(err, dtype=np.float64)


class MirrorContext:
    """What CO2_example's gradient functions ask of a GPContext, answered by the float64 mirror."""

    def __init__(self):
        self.kind, self.th, self.X, self.y, self.fit_at = "rbf", None, None, None, None
        self.factorizations = 0

    def set_kernel(self, kind, p0=0.0, p1=0.0):
        self.kind, self.fit_at = kind, None
        self.th = np.array(p0, dtype=np.float64).reshape(-1) if kind == "co2" else None
        if kind == "co2" and self.th.shape[0] != 11:
            self.kind = "rbf"
            raise ValueError("the CO2 composite kernel takes 11 hyper-parameters")

    def set_train(self, X, y):
        self.X, self.y, self.fit_at = np.asarray(X, dtype=np.float64), np.asarray(y, dtype=np.float64).reshape(-1), None

    def factorize(self, sigma, l, noise_var):
        assert self.kind == "co2"
        self.fit_at = None
        self.factorizations += 1
        value = lml(self.X, self.y, self.th, noise_var)          # LinAlgError where K + sI is not positive definite
        self.fit_at = (self.th.copy(), float(noise_var))
        return float(value)

    def fit(self, X, y, sigma, l, noise_var):
        self.set_train(X, y)
        return self.factorize(sigma, l, noise_var)

    def lml_grad_co2(self):
        if self.fit_at is None or self.kind != "co2":
            raise ValueError("no CO2 factorisation resident")
        ref = lml_and_grad(self.X, self.y, self.fit_at[0], self.fit_at[1])
        return ref["g_theta"].copy(), float(ref["g_noise"])
