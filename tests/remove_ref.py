"""NumPy float64 mirror of gpmi_remove (gaussian_process_amd/csrc/remove.hip), in the order the device runs:

    the sorted indices go in DESCENDING groups of at most 16 (the 16 largest first, the smallest group last);
    one group is one left-to-right pass over the old columns c from the group's first index on --
      removed column c     not rotated, not written; its part below the diagonal, the y row's entry m_c included,
                           becomes the next active vector; row c is dropped
      surviving column c   for each active vector i, in index order:
                             r = sqrt(d d + v_i[c]^2),  cs = d / r,  sn = v_i[c] / r,  the diagonal d becomes r,
                             and in every row below, the y row included,
                             t = cs L_rc + sn v_ri;  v_ri = cs v_ri - sn L_rc;  L_rc = t

(the device fuses each of the two updates and d d + v^2 into one rounding less: fma(cs, L, sn v), fma(cs, v, -(sn L)),
fma(d, d, v v).)  Rows are independent of each other, so the mirror works on whole columns.

Test infrastructure: dense matrices, small N only.  Nothing here needs a GPU."""
import numpy as np

REMOVE_MAX = 16


def groups(idx):
    """the sorted indices in the groups the sweeps take, in the order they run"""
    s = sorted(int(i) for i in idx)
    out, end = [], len(s)
    while end > 0:
        first = max(0, end - REMOVE_MAX)
        out.append(s[first:end])
        end = first
    return out


def sweep(G, m, rem):
    """one pass: the factor G (n x n, lower) and m = L^-1 y without the <= 16 ascending indices rem"""
    n = G.shape[0]
    assert 0 < len(rem) <= REMOVE_MAX and len(rem) < n
    L = np.tril(G).astype(np.float64)
    L = np.vstack([L, np.asarray(m, dtype=np.float64)[None, :]])        # the y row is one more row
    gone = set(rem)
    V = []                                                              # active vectors, full height (rows <= c unused)
    for c in range(rem[0], n):
        if c in gone:
            v = L[:, c].copy()
            v[:c + 1] = 0.0
            V.append(v)
            continue
        for v in V:
            d, w = L[c, c], v[c]
            r = np.sqrt(d * d + w * w)
            cs, sn = d / r, w / r
            L[c, c] = r
            col, vv = L[c + 1:, c].copy(), v[c + 1:].copy()
            L[c + 1:, c] = cs * col + sn * vv
            v[c + 1:] = cs * vv - sn * col
    keep = [i for i in range(n) if i not in gone]
    out = L[np.ix_(keep + [n], keep)]
    return np.ascontiguousarray(out[:-1]), np.ascontiguousarray(out[-1])


def remove(G, m, idx):
    """(G, m) of a fit of n points -> (G', m') of the fit without the points idx, the survivors in their order"""
    idx = [int(i) for i in idx]
    n = G.shape[0]
    assert len(set(idx)) == len(idx) and 0 < len(idx) < n and min(idx) >= 0 and max(idx) < n
    G, m = np.tril(G), np.asarray(m, dtype=np.float64)
    for g in groups(idx):
        G, m = sweep(G, m, g)
    return G, m


def fit(Ky, y):
    """the plain float64 factor and m = L^-1 y of K_y"""
    L = np.linalg.cholesky(Ky)
    return L, np.linalg.solve(L, y)


def lml(G, m):
    n = G.shape[0]
    return -.5 * float(m @ m) - float(np.sum(np.log(np.diag(G)))) - .5 * n * np.log(2 * np.pi)
