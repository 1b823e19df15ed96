"""Plain reference of GP regression's prediction and its posterior-sample factor for the squared-exponential covariance
with per-dimension lengthscales, as oracle/gp_oracle.py::fit_predict_feasible states them from the Cholesky factor:

    K_y = K + noise I = L L^T,   m = L^-1 y,   alpha = L^-T m,   lml = -.5 m.m - sum log diag L - N/2 log 2 pi
    v = L^-1 K(X, X*),   mu = v^T m,   var = sigma^2 - sum_i v_i^2
    Sigma_j = K(X*, X*) + j I - v^T v,   L_ = chol(Sigma_j),   L_ @ Z            for every jitter j

K from the scaled inputs ard_ref.scaled (one float64 division per element, what the device forms), the squared distance
added one dimension after the other.  Three evaluations of the same statements:

    fit / predict with dtype = numpy.float64      LAPACK (numpy.linalg.cholesky, scipy's solve_triangular)
    fit / predict with dtype = numpy.longdouble   the column loops of tests/sgpr_ref.py, every product in long double
    blocked                                       float64 in another summation order: the right-looking factorisation
                                                  in 384-wide blocks of oracle/gp_oracle.py::fit_predict_blocked, with
                                                  the y row and the rows K(X*, X) carried below the triangle (they leave
                                                  as m^T and v^T), v^T v subtracted one block of K after the other, and
                                                  the same blocked factorisation of Sigma_j; other_k: the covariance
                                                  itself rounded otherwise (kernel_other_rounding)

Test infrastructure: dense matrices, small N only."""
import numpy as np
from scipy.linalg import solve_triangular

import ard_ref as R
import sgpr_ref as S

BLOCK = 384
QUANTITIES = ("lml", "alpha", "m", "diag", "mu", "var")
PER_JITTER = ("Sigma", "L_", "LZ")


def kernel(za, zb, sigma, l, dtype):
    """sigma^2 exp(-.5 / l^2 |za - zb|^2) of scaled inputs, in dtype"""
    za, zb = za.astype(dtype), zb.astype(dtype)
    sq = np.zeros((za.shape[0], zb.shape[0]), dtype=dtype)
    for k in range(za.shape[1]):
        sq += (za[:, None, k] - zb[None, :, k]) ** 2
    return dtype(sigma) ** 2 * np.exp(dtype(-.5) / dtype(l) ** 2 * sq)


def kernel_other_rounding(za, zb, sigma, l):
    """the same covariance in float64 with every rounding another one: the squared distance added from the last dimension
    to the first, and (sigma e^(a / 2))^2 for sigma^2 e^a.  The elements are a few ulp from kernel()'s (2e-15 in relative
    terms at the most, where |a| is large): the distance at which an exponential of one's own, such as the device's, stands"""
    sq = np.zeros((za.shape[0], zb.shape[0]))
    for k in reversed(range(za.shape[1])):
        sq += (za[:, None, k] - zb[None, :, k]) ** 2
    return (sigma * np.exp(-.25 / l ** 2 * sq)) ** 2


def solve_upper_t(solve_lower, L, b):
    """L^-T b with a forward substitution: L^T reversed in both directions is lower triangular"""
    return solve_lower(np.ascontiguousarray(L.T[::-1, ::-1]), b[::-1])[::-1]


def lml_of(m, diag, N, dtype):
    return dtype(-.5) * (m @ m) - np.sum(np.log(diag)) - dtype(.5) * N * np.log(2 * dtype(np.pi))


def fit(X, y, r, sigma, l, noise, dtype=np.float64):
    """-> dict: the factor L and what a fit returns (lml, m, diag, alpha), with the inputs a prediction needs"""
    chol, solve_lower = S._ops(dtype)
    z = R.scaled(X, r)
    N = len(z)
    L = chol(kernel(z, z, sigma, l, dtype) + dtype(noise) * np.eye(N, dtype=dtype))
    m = solve_lower(L, np.asarray(y, dtype=dtype))
    diag = np.diag(L).copy()
    return dict(L=L, m=m, diag=diag, alpha=solve_upper_t(solve_lower, L, m), lml=lml_of(m, diag, N, dtype), z=z, r=r,
                sigma=sigma, l=l, dtype=dtype)


def posterior(Kss, vtv, jitters, Z, chol, dtype):
    out = {}
    for j in jitters:
        Sigma = Kss + dtype(j) * np.eye(len(Kss), dtype=dtype) - vtv
        L_ = chol(Sigma)
        out[j] = dict(Sigma=Sigma, L_=L_, LZ=L_ @ np.asarray(Z, dtype=dtype))
    return out


def predict(f, Xs, jitters, Z):
    """-> dict: lml, m, diag, alpha of the fit f, mu and var at Xs, and post[j] = {Sigma, L_, LZ} for every jitter"""
    dtype = f["dtype"]
    chol, solve_lower = S._ops(dtype)
    zs = R.scaled(Xs, f["r"])
    v = solve_lower(f["L"], kernel(f["z"], zs, f["sigma"], f["l"], dtype))
    out = {k: f[k] for k in ("lml", "m", "diag", "alpha")}
    out["mu"] = v.T @ f["m"]
    out["var"] = dtype(f["sigma"]) ** 2 - np.sum(v * v, axis=0)
    out["post"] = posterior(kernel(zs, zs, f["sigma"], f["l"], dtype), v.T @ v, jitters, Z, chol, dtype)
    return out


def chol_blocked(A, ncols, block=BLOCK):
    """in place: the right-looking blocked Cholesky of the leading ncols x ncols block of A (lower triangle); the rows
    below it are carried and leave multiplied by L^-T"""
    for k in range(0, ncols, block):
        e = min(k + block, ncols)
        A[k:e, k:e] = np.linalg.cholesky(A[k:e, k:e])
        A[e:, k:e] = solve_triangular(A[k:e, k:e], A[e:, k:e].T, lower=True).T
        for j in range(e, ncols, block):
            je = min(j + block, ncols)
            A[j:, j:je] -= A[j:, k:e] @ A[j:je, k:e].T
    return A


def blocked(X, y, r, Xs, sigma, l, noise, jitters, Z, block=BLOCK, other_k=False):
    """the dict of predict() from the blocked float64 evaluation; other_k: the covariance with kernel_other_rounding"""
    z, zs = R.scaled(X, r), R.scaled(Xs, r)
    N, n = len(z), len(zs)
    cov = kernel_other_rounding if other_k else lambda a, b, sg, ll: kernel(a, b, sg, ll, np.float64)
    A = np.empty((N + 1 + n, N))
    A[:N] = cov(z, z, sigma, l) + noise * np.eye(N)
    A[N] = y
    A[N + 1:] = cov(zs, z, sigma, l)
    chol_blocked(A, N, block)
    L, m, vt = np.tril(A[:N]), A[N].copy(), A[N + 1:]
    diag = np.diag(L).copy()
    out = dict(lml=lml_of(m, diag, N, np.float64), m=m, diag=diag, alpha=solve_triangular(L, m, lower=True, trans="T"),
               mu=vt @ m, var=sigma ** 2 - np.sum(vt * vt, axis=1))
    Kss = cov(zs, zs, sigma, l)
    out["post"] = {}
    for j in jitters:
        # Sigma as the trailing updates of the augmented factorisation leave it: K_ss + j I less one product per block of
        # K.  One dgemm over all of K would sum every entry in the order the LAPACK evaluation's dgemm does, and the
        # distance of the two evaluations would say nothing about the rounding of that depth-N sum
        Sigma = Kss + j * np.eye(n)
        for k in range(0, N, block):
            Sigma -= vt[:, k:k + block] @ vt[:, k:k + block].T
        L_ = np.tril(chol_blocked(Sigma.copy(), n, block))
        out["post"][j] = dict(Sigma=Sigma, L_=L_, LZ=L_ @ np.asarray(Z, dtype=np.float64))
    return out


def f64(v):
    return np.asarray(v, dtype=np.float64)


def errors(got, ref):
    """-> {quantity: error} of one evaluation (or one device run) against a reference, each in the normalisation its bar is
    stated in: lml relative; alpha, m and diag relative to the largest element (relmax of tests/test_parity_gpu.py); mu
    relative to max(1, max|mu|); var, and per jitter Sigma (got's L_ L_^T, a float64 product by BLAS, against the
    reference's Sigma), L_ and L_ @ Z absolute.  The differences are taken in the reference's dtype.  got["post"][j] needs L_ and LZ only"""
    dt = np.asarray(ref["mu"]).dtype.type
    a = lambda v: np.asarray(v, dtype=dt)          # noqa: E731
    gap = lambda k: float(np.max(np.abs(a(got[k]) - ref[k])))      # noqa: E731
    out = dict(lml=float(abs(a(got["lml"]) - ref["lml"]) / abs(ref["lml"])))
    for k in ("alpha", "m", "diag"):
        if k in got:
            out[k] = gap(k) / float(np.max(np.abs(ref[k])))
    out["mu"] = gap("mu") / max(1.0, float(np.max(np.abs(ref["mu"]))))
    out["var"] = gap("var")
    for j, p in got.get("post", {}).items():
        q = ref["post"][j]
        L_ = f64(p["L_"])
        out["Sigma@%g" % j] = float(np.max(np.abs(a(L_ @ L_.T) - q["Sigma"])))        # the product by BLAS, in float64
        out["L_@%g" % j] = float(np.max(np.abs(a(L_) - q["L_"])))
        out["LZ@%g" % j] = float(np.max(np.abs(a(p["LZ"]) - q["LZ"])))
    return out
