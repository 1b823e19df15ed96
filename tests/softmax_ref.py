"""NumPy float64 restatement of the GPU softmax classifier (gpmi_softmax_fit / gpmi_softmax_predict_resident), line for
line with softmax.hip's driver: GPML Algorithms 3.3 and 3.4 with one shared kernel, labels 0 .. C-1, the step-halving
rule of the binary classifier, the extra log-determinant term of log q, and the clamped C x C Cholesky of the
prediction's sampling.  Test infrastructure only."""
import numpy as np
from scipy.linalg import cholesky, solve_triangular

from laplace_ref import rbf


def blobs(N, d, C, seed, n=50):
    """C Gaussian blobs with overlapping tails -> (X, labels, X_test)"""
    rng = np.random.default_rng(seed)
    cen = rng.standard_normal((C, d)) * 2.0
    lab = rng.integers(0, C, N + n)
    X = cen[lab] + rng.standard_normal((N + n, d)) * 1.2
    return X[:N], lab[:N], X[N:]


def softmax_cols(F):
    """F (C, N) -> (P, logsumexp per column), the maximum subtracted"""
    m = F.max(axis=0)
    e = np.exp(F - m)
    se = e.sum(axis=0)
    return e / se, m + np.log(se)


def newton_state(Y, A, F):
    """P and Psi(A, F) = -1/2 sum(A o F) + sum(Y o F) - sum_i logsumexp_c F_ci"""
    P, lse = softmax_cols(F)
    psi = -0.5 * np.sum(A * F) + (np.sum(Y * F, axis=0) - lse).sum()
    return P, psi


def fit(X, labels, C, sigma, l, tol=1e-10, max_iter=100, K=None, max_halvings=20):
    """-> dict(log_q, F, P, Y, G = Y - P, Es, M, psi, iters, converged, K, halvings, decisions): halvings[k] is the
    number of halved steps and decisions[k] the list of (d, thr) of every accept / halve decision taken after Newton
    step k + 1"""
    K = rbf(X, X, sigma, l) if K is None else K
    labels = np.asarray(labels).astype(np.int64)
    N = labels.shape[0]
    Y = np.zeros((C, N))
    Y[labels, np.arange(N)] = 1
    A = np.zeros((C, N))
    A_prev = F_prev = psi_prev = None
    iters, converged = 0, False
    halved, decisions = [], []
    while True:
        F = A @ K                                                  # 1.
        P, psi = newton_state(Y, A, F)
        if psi_prev is not None:                                   # 2.
            halvings = 0
            halved.append(0)
            decisions.append([])
            while True:
                d = psi - psi_prev
                thr = tol * max(1.0, abs(psi))
                halved[-1] = halvings
                decisions[-1].append((d, thr))
                if abs(d) <= thr:
                    converged = True
                    break
                if d < -thr and halvings < max_halvings:
                    A = (A + A_prev) / 2
                    F = (F + F_prev) / 2
                    P, psi = newton_state(Y, A, F)
                    halvings += 1
                    continue
                break
        last = converged or iters >= max_iter
        S = np.sqrt(P)
        Es, z = [], 0.0                                            # 3.
        for c in range(C):
            L = cholesky(np.eye(N) + np.outer(S[c], S[c]) * K, lower=True)
            V = solve_triangular(L, np.diag(S[c]), lower=True)     # (S_c L_c^-T)^T
            Es.append(V.T @ V)
            z += np.log(np.diag(L)).sum()
        if not last:                                               # 4.
            B = P * F - P * np.sum(P * F, axis=0) + Y - P
            KB = B @ K
            Cc = np.stack([Es[c] @ KB[c] for c in range(C)])
        M = cholesky(sum(Es[1:], Es[0]), lower=True)               # 5.
        if last:
            break
        t = solve_triangular(M.T, solve_triangular(M, Cc.sum(axis=0), lower=True), lower=False)   # 6.
        A_prev, F_prev, psi_prev = A, F, psi
        A = B - Cc + np.stack([Es[c] @ t for c in range(C)])
        iters += 1
    log_q = psi - z - np.log(np.diag(M)).sum()
    return dict(log_q=log_q, F=F, P=P, Y=Y, G=Y - P, Es=Es, M=M, psi=psi, iters=iters, converged=converged, K=K,
                halvings=halved, decisions=decisions)


def predict(ft, X, Xs, sigma, l):
    """-> (mu (n, C), Sigma (n, C, C))"""
    C = ft["F"].shape[0]
    R = rbf(Xs, X, sigma, l)
    mu = R @ ft["G"].T
    Bc = [R @ ft["Es"][c] for c in range(C)]
    U = [solve_triangular(ft["M"], Bc[c].T, lower=True) for c in range(C)]
    Sig = np.zeros((len(Xs), C, C))
    for c in range(C):
        for e in range(c + 1):
            Sig[:, c, e] = Sig[:, e, c] = np.sum(U[c] * U[e], axis=0)
        Sig[:, c, c] += sigma ** 2 - np.sum(Bc[c] * R, axis=1)
    return mu, Sig


def chol_clamped(Sg):
    """lower Cholesky factor of a C x C matrix; a pivot <= 0 is set to 0 and its column to 0"""
    C = Sg.shape[0]
    L = np.zeros((C, C))
    for j in range(C):
        dj = Sg[j, j] - np.sum(L[j, :j] ** 2)
        if not dj > 0.0:
            continue
        L[j, j] = np.sqrt(dj)
        for r in range(j + 1, C):
            L[r, j] = (Sg[r, j] - np.sum(L[r, :j] * L[j, :j])) / L[j, j]
    return L


def proba(mu, Sig, normals):
    """(n, C): mean over the S rows of normals of softmax(mu_i + chol(Sigma_i) z_s)"""
    out = np.empty_like(mu)
    for i in range(mu.shape[0]):
        G = mu[i][:, None] + chol_clamped(Sig[i]) @ normals.T     # (C, S)
        out[i] = softmax_cols(G)[0].mean(axis=1)
    return out
