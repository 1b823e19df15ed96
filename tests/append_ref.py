"""NumPy float64 mirror of gpmi_append (gaussian_process_amd/csrc/append.hip) on the device's 16 x 16-tile recurrences
(tests/panel_ref.py): the resident factor of the first N points, then the border of k more --

    N0 = floor(N / 128) 128,  border = rows [N0, ceil((N + k) / 128) 128)
    W = K(border, X[0:N0]) L0^-T               panel_ref.mirror_trsm through the leading N0 x N0 factor
    S = K_bb + noise I - W W^T                 identity padding beyond N + k
    L_bb = chol(S)                             panel_ref.mirror_potrf
    m_b = (y_b - m_0 W^T) L_bb^-T              the y row, carried

Test infrastructure: dense matrices, small N only.  Nothing here needs a GPU."""
import numpy as np

import panel_ref as R

TILE = 128


def round_up(x):
    return (x + TILE - 1) // TILE * TILE


def padded(Ky, n):
    """Ky (n x n) in the identity-padded square the device factors"""
    npad = round_up(n)
    P = np.eye(npad)
    P[:n, :n] = Ky
    return P


def fit(Ky, y):
    """the resident state of a fit: (G, m) with G the fused-layout factor of the padded matrix, m = L^-1 y padded with
    zeros (the y row rides through the factorisation)"""
    n = Ky.shape[0]
    G, fail = R.mirror_potrf(padded(Ky, n))
    assert fail is None
    yp = np.zeros(G.shape[0])
    yp[:n] = y
    return G, R.mirror_trsm(G, yp[None, :])[0]


def append(G, m, N, Ky1, y1):
    """the resident state (G, m) of N points extended to the N1 points of Ky1 (N1 x N1, its leading N x N block the
    fitted one), y1: -> (G1, m1) as the device leaves them"""
    N1 = Ky1.shape[0]
    N0, Np1 = N // TILE * TILE, round_up(N1)
    P = padded(Ky1, N1)
    yp = np.zeros(Np1)
    yp[:N1] = y1
    G1 = np.zeros((Np1, Np1))
    G1[:N0, :N0] = G[:N0, :N0]
    m1 = np.zeros(Np1)
    m1[:N0] = m[:N0]
    L0 = G[:N0, :N0]
    W = R.mirror_trsm(L0, P[N0:, :N0]) if N0 else np.zeros((Np1 - N0, 0))
    S = P[N0:, N0:] - W @ W.T
    Gb, fail = R.mirror_potrf(S)
    assert fail is None
    G1[N0:, :N0] = W
    G1[N0:, N0:] = Gb
    mb = yp[N0:] - m[:N0] @ W.T
    m1[N0:] = R.mirror_trsm(Gb, mb[None, :])[0]
    return G1, m1


def lml(G, m, n):
    """tune_hyperparms_regression.py:312 from the factor and m"""
    return -.5 * float(m[:n] @ m[:n]) - float(np.sum(np.log(np.diag(G)[:n]))) - .5 * n * np.log(2 * np.pi)
