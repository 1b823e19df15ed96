"""References for the Cholesky panel kernels (panel_mfma.hip, panel.hip, the recursions of driver.hip): seeded test matrices,
a long-double Cholesky that names the first failing pivot, a float64 mirror of the device recurrence on 16 x 16 tiles, and
the componentwise ratios that tests/test_panel_kernels_gpu.py (device) and tests/test_panel_ref_cpu.py (mirror) hold to the
same bars.  NumPy only: nothing here needs a GPU."""
import functools
import math

import numpy as np

U = 2.0 ** -53
LD = np.longdouble
T = 16                       # the tile of the fused leaves (panel_mfma.hip)
SENTINEL = (1 << 63) - 1     # what *info holds while no pivot has failed


def _frozen(a):
    a.setflags(write=False)
    return a


# ---------------------------------------------------------------- matrices, all seeded

@functools.lru_cache(maxsize=None)
def spd(n, cond, seed=7):
    """the _spd of test_block_primitives_gpu.py: random orthogonal basis, eigenvalues log-spaced in [1 / cond, 1]"""
    rng = np.random.default_rng(seed)
    Q, _ = np.linalg.qr(rng.standard_normal((n, n)))
    ev = np.logspace(0, -math.log10(cond), n)
    A = (Q * ev) @ Q.T
    return _frozen((A + A.T) / 2)


@functools.lru_cache(maxsize=None)
def gp(n, ell, noise, seed=3):
    """exp(-|x - x'|^2 / 2 ell^2) + noise I on n uniform points in [0, 4]^2: a smooth kernel with tiny noise"""
    rng = np.random.default_rng(seed)
    X = rng.uniform(0.0, 4.0, (n, 2))
    sq = ((X[:, None, :] - X[None, :, :]) ** 2).sum(2)
    K = np.exp(-sq / (2 * ell * ell))
    K = (K + K.T) / 2
    K[np.arange(n), np.arange(n)] = 1.0 + noise
    return _frozen(K)


@functools.lru_cache(maxsize=None)
def graded_exponents(n, seed=5):
    return _frozen(np.random.default_rng(seed).integers(-40, 41, n))


@functools.lru_cache(maxsize=None)
def graded(n):
    """D spd(n, 1e6) D, D = diag(2^k) with integer k uniform in [-40, 40]: an exact scaling of rows and columns, so the
    entries span 2^160 and only a componentwise bound means anything"""
    d = np.exp2(graded_exponents(n).astype(np.float64))
    return _frozen(spd(n, 1e6) * d[:, None] * d[None, :])


@functools.lru_cache(maxsize=None)
def scaled(n, e):
    """2^e spd(n, 1e2), exactly"""
    return _frozen(np.ldexp(spd(n, 1e2), e))


def ref_cholesky(S, upto=None):
    """Left-looking Cholesky in long double.  Returns (L, fail, pivot): fail is the first column whose pivot is not > 0
    (NaN included) and pivot its value, or (None, None) when all are positive; columns >= fail of L are zero.
    upto: stop after that many columns (the rows of those columns are complete)."""
    n = S.shape[0]
    Sl = S.astype(LD)
    L = np.zeros((n, n), LD)
    for j in range(n if upto is None else upto):
        c = Sl[j:, j] - L[j:, :j] @ L[j, :j]
        if not c[0] > 0:
            return L, j, float(c[0])
        L[j, j] = np.sqrt(c[0])
        L[j + 1:, j] = c[1:] / L[j, j]
    return L, None, None


def planted(S, j, kind):
    """S with pivot j made to fail; nothing but S[j, j] changes, so every leading minor of order <= j is untouched.
    "neg": S[j, j] = l_j . l_j - 1 with l_j row j (columns < j) of the long-double factor: the Schur pivot is -1.
    "nan": S[j, j] = NaN.
    "zero": S is only asked for its size -- the identity with the 2 x 2 block [[1, 1], [1, 1]] at (j - 1, j): pivot j
    is 1 - 1 * 1, exactly 0 in any arithmetic."""
    n = S.shape[0]
    if kind == "zero":
        assert j >= 1
        P = np.eye(n)
        P[j - 1, j] = P[j, j - 1] = 1.0
        return P
    P = np.array(S, dtype=np.float64)
    if kind == "nan":
        P[j, j] = np.nan
    elif kind == "neg":
        L, fail, _ = ref_cholesky(P, upto=j)
        assert fail is None, "pivot %d fails before the planted one" % fail
        row = L[j, :j]                       # complete: columns < j are
        P[j, j] = float(row @ row - 1)
    else:
        raise ValueError(kind)
    return P


# ---------------------------------------------------------------- the device recurrence in float64

def _factor_tile(A):
    """factor16_packed: right-looking sweep of a 16 x 16 tile, columns scaled by 1 / sqrt(pivot); the same sweep on the
    identity gives W = L^-1 (forward substitution).  Returns (L, W, first bad pivot or 16)."""
    v = np.tril(A).astype(np.float64)
    w = np.eye(T)
    bad = T
    for c in range(T):
        p = v[c, c]
        if not p > 0 and bad == T:
            bad = c
        with np.errstate(all="ignore"):
            g = np.sqrt(p) if p > 0 else np.nan
            h = 1.0 / g
        v[c + 1:, c] *= h
        v[c, c] = g
        w[c, :] *= h
        lc = v[c + 1:, c]
        v[c + 1:, c + 1:] -= np.outer(lc, lc)
        w[c + 1:, :] -= np.outer(lc, w[c, :])
    return np.tril(v), np.tril(w), bad


def mirror_potrf(S):
    """potrf128 / trsm128 / the Schur updates as one flat right-looking sweep over 16-column steps, in float64:
       1  factor the diagonal tile;  2  W = L_jj^-1 by forward substitution on the identity;
       3  L_ij = S_ij W^T for the rows below;  4  S_ik -= L_ij L_kj^T.
    Returns (G, fail): G as the device leaves the block -- L on and below the diagonal, W_jj^T in the strict upper
    triangles of the diagonal tiles, the other tiles above the diagonal as they were -- and the first failing pivot."""
    n = S.shape[0]
    assert n % T == 0
    A = np.array(S, dtype=np.float64)
    fail = None
    with np.errstate(all="ignore"):
        for j in range(0, n, T):
            L, W, bad = _factor_tile(A[j:j + T, j:j + T])
            if bad < T and fail is None:
                fail = j + bad
            A[j:j + T, j:j + T] = L + np.triu(W.T, 1)
            if j + T < n:
                Lc = A[j + T:, j:j + T] @ W.T
                A[j + T:, j:j + T] = Lc
                A[j + T:, j + T:] -= Lc @ Lc.T
    G = np.where(upper_tiles(n), np.asarray(S, dtype=np.float64), A)
    return G, fail


def stored_inverse(G, t):
    """W_t of diagonal tile t of a fused factor: the transpose of the tile's strict upper triangle, 1 / diag(L_tt) on
    the diagonal"""
    tile = G[T * t:T * t + T, T * t:T * t + T]
    return np.triu(tile, 1).T + np.diag(1.0 / np.diagonal(tile))


def mirror_trsm(G, X0):
    """trsm128's recurrence in float64 with the stored inverses of G:  X_j <- X_j W_jj^T;  X_k -= X_j L_kj^T, k > j"""
    n = G.shape[0]
    X = np.array(X0, dtype=np.float64)
    L = np.tril(G)
    for t in range(n // T):
        j = T * t
        X[:, j:j + T] = X[:, j:j + T] @ stored_inverse(G, t).T
        if j + T < n:
            X[:, j + T:] -= X[:, j:j + T] @ L[j + T:, j:j + T].T
    return X


def mirror_trsv_lt(G, b):
    """solve.hip's trsv_lt_step128_kernel in float64: back substitution on 16 x 16 tiles with explicit tile inverses,
    for s = last..0:  x_s = W_ss^T r_s;  r_t -= L_st^T x_s (t < s)"""
    n = G.shape[0]
    r = np.array(b, dtype=np.float64)
    L = np.tril(G)
    for t in range(n // T - 1, -1, -1):
        j = T * t
        r[j:j + T] = stored_inverse(G, t).T @ r[j:j + T]
        r[:j] -= L[j:j + T, :j].T @ r[j:j + T]
    return r


# ---------------------------------------------------------------- the ratios the bars are set on

def _ratio(num, den):
    """max num / den over the elements, 0 / 0 counted as 0 and x / 0 as inf"""
    num, den = np.asarray(num, LD), np.asarray(den, LD)
    with np.errstate(all="ignore"):
        q = np.where(num == 0, LD(0), num / den)
    q = np.where(np.isnan(q), LD(np.inf), q)
    return float(q.max()) if q.size else 0.0


def potrf_ratio(S, G):
    """worst |S - L L^T|_ij / (n u (|L| |L^T|)_ij) over i >= j, L = tril(G); the residual in long double, 128 x 128 block
    by block of the lower triangle with the sums cut at the block's last column (the bar is 2)"""
    n = S.shape[0]
    L = np.tril(G)
    Ll, La = L.astype(LD), np.abs(L)
    worst = 0.0
    for r0 in range(0, n, 128):
        r1 = min(n, r0 + 128)
        for c0 in range(0, r1, 128):
            c1 = min(n, c0 + 128)
            R = np.abs(S[r0:r1, c0:c1].astype(LD) - Ll[r0:r1, :c1] @ Ll[c0:c1, :c1].T)
            D = (La[r0:r1, :c1] @ La[c0:c1, :c1].T).astype(LD) * (n * U)
            low = np.arange(r0, r1)[:, None] >= np.arange(c0, c1)[None, :]
            worst = max(worst, _ratio(R[low], D[low]))
    return worst


def inverse_ratio(G):
    """worst |L_tt W_t - I|_ij / (16 u (|L_tt| |W_t|)_ij) over the lower triangles of the diagonal tiles (the bar is 2)"""
    worst = 0.0
    low = np.tril(np.ones((T, T), bool))
    for t in range(G.shape[0] // T):
        Lt = np.tril(G[T * t:T * t + T, T * t:T * t + T])
        W = stored_inverse(G, t)
        R = np.abs(Lt.astype(LD) @ W.astype(LD) - np.eye(T, dtype=LD))
        D = (np.abs(Lt).astype(LD) @ np.abs(W).astype(LD)) * (T * U)
        worst = max(worst, _ratio(R[low], D[low]))
    return worst


def trsm_ratio(G, X0, X, rows=None):
    """worst |X0 - X L^T|_rc / (nb u (|X| |L^T|)_rc), L = tril(G), over the given rows (all by default); the residual
    in long double (the bar is 2)"""
    nb = G.shape[0]
    if rows is not None:
        X0, X = X0[rows], X[rows]
    L = np.tril(G)
    Ll, La = L.astype(LD), np.abs(L)
    worst = 0.0
    for c0 in range(0, nb, 128):
        c1 = min(nb, c0 + 128)              # L is lower triangular: column block c of X L^T needs X[:, :c1] only
        for r0 in range(0, X.shape[0], 1024):
            Xb = X[r0:r0 + 1024, :c1]
            R = np.abs(X0[r0:r0 + 1024, c0:c1].astype(LD) - Xb.astype(LD) @ Ll[c0:c1, :c1].T)
            D = (np.abs(Xb) @ La[c0:c1, :c1].T).astype(LD) * (nb * U)
            worst = max(worst, _ratio(R, D))
    return worst


def kappa16(G):
    """the largest cond_inf of a diagonal 16 x 16 tile of L"""
    return max(np.linalg.norm(Lt, np.inf) * np.linalg.norm(np.linalg.inv(Lt), np.inf)
               for Lt in (np.tril(G[j:j + T, j:j + T]) for j in range(0, G.shape[0], T)))


def trsv_ratio(G, b, x):
    """||b - L^T x||_inf / ((n + 16 kappa16) u || |L^T| |x| ||_inf), the residual in long double (the bar is 4)"""
    n = G.shape[0]
    Ll, xl = np.tril(G).astype(LD), x.astype(LD)
    r = np.abs(b.astype(LD) - Ll.T @ xl)
    s = np.abs(Ll.T) @ np.abs(xl)
    return float(r.max() / ((n + T * kappa16(G)) * U * s.max()))


def upper_tiles(n):
    """mask of the elements in 16 x 16 tiles strictly above the block diagonal"""
    t = np.arange(n) // T
    return t[None, :] > t[:, None]


# ---------------------------------------------------------------- the cases, shared by the device and the mirror tests

MATRICES = {
    "spd1e2": lambda n: spd(n, 1e2),
    "spd1e10": lambda n: spd(n, 1e10),
    "gp1": lambda n: gp(n, 1.0, 1e-6),
    "gp2": lambda n: gp(n, 2.0, 1e-8),
    "graded": graded,
    "scaled+600": lambda n: scaled(n, 600),
    "scaled-600": lambda n: scaled(n, -600),
}

# test 1, fused path: the full cross at nb 128 and 512; spd only at the sizes that add a split or a level; the scalings
POTRF_FUSED = ([(nb, name) for nb in (128, 512) for name in ("spd1e2", "spd1e10", "gp1", "gp2", "graded")] +
               [(nb, name) for nb in (256, 384, 1024) for name in ("spd1e2", "spd1e10")] +
               [(256, "scaled+600"), (256, "scaled-600")])
POTRF_FIRST_GEN = [(nb, name) for nb in (128, 256) for name in ("spd1e10", "graded")]
# test 2
INVERSE = [(128, "spd1e10"), (128, "gp2")]
# test 4, fused path
TRSM_FUSED = [(nb, m, name) for nb in (128, 256, 512) for m in (128, 640) for name in ("spd1e2", "spd1e10", "graded", "gp2")]
# test 8
TRSV = [(n, name) for n in (128, 512) for name in ("spd1e2", "spd1e10")]


def rhs(m, nb, seed=11):
    """standard normal X0 (m x nb)"""
    return np.random.default_rng(seed + m + nb).standard_normal((m, nb))


# test 4, the other paths: 64-wide first-generation leaves on a fused factor (nb = 192: the leading 192 columns of a 256 factor),
# and a first-generation factor under trsm_wave 1 / 0 and, at m = 16512, the lane-per-row kernel by size
TRSM_NB192 = [(192, 128, name) for name in ("spd1e10", "graded")]
TRSM_FIRST_GEN = [(nb, m, name) for nb in (128, 256) for m in (128, 640, 16512) for name in ("spd1e10", "graded")]

# test 6: nb = 256 on spd(256, 1e2)
PIVOTS_FUSED = [(j, "neg") for j in (0, 1, 15, 16, 17, 31, 112, 127, 128, 129, 143, 255)]
PIVOTS_TILE3 = list(range(48, 64))            # every position inside one 16 x 16 tile, run in one sweep
PIVOTS_KINDS = [(j, kind) for kind in ("nan", "zero") for j in (17, 128)]
PIVOT_PAIRS = [(40, 200), (130, 131)]
PIVOTS_FIRST_GEN = [(j, "neg") for j in (0, 63, 64, 65, 127, 200)] + [(64, "nan")]


@functools.lru_cache(maxsize=None)
def planted_case(j, kind, j2=None):
    """planted(spd(256, 1e2), j, kind); with j2 a second "neg" pivot planted at j2 > j first"""
    S = spd(256, 1e2)
    if j2 is not None:
        assert j2 > j
        S = planted(S, j2, "neg")
    return _frozen(planted(S, j, kind))


def sample_rows(m, seed=13):
    """for the tall shapes: 256 rows sampled from all but the last 256, and the last 256"""
    rng = np.random.default_rng(seed + m)
    return np.concatenate([np.sort(rng.choice(m - 256, 256, replace=False)), np.arange(m - 256, m)])
