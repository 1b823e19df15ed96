"""The references of tests/panel_ref.py, without a GPU: the matrix builders do what they say, the long-double Cholesky names
the planted pivot, and the float64 mirror of the device recurrence sits at no more than HALF of every bar that
tests/test_panel_kernels_gpu.py holds the device to -- the bars are conditions, so the inputs must leave room for them."""
import numpy as np
import pytest

import panel_ref as R

POTRF_CASES = sorted(set(R.POTRF_FUSED + R.POTRF_FIRST_GEN))
TRSM_CASES = sorted(set(R.TRSM_FUSED + R.TRSM_NB192 + R.TRSM_FIRST_GEN))
_mirrors = {}


def _mirror(nb, name):
    """the mirror's factor of a case's matrix, computed once; nb = 192 is the leading block of the 256 factor"""
    if nb == 192:
        return _mirror(256, name)[:192, :192]
    if (nb, name) not in _mirrors:
        G, fail = R.mirror_potrf(R.MATRICES[name](nb))
        assert fail is None
        G.setflags(write=False)
        _mirrors[nb, name] = G
    return _mirrors[nb, name]


# ---------------------------------------------------------------- the mirror leaves room under every bar

@pytest.mark.parametrize("nb,name", POTRF_CASES)
def test_mirror_margin_potrf(nb, name):
    """test 1: |S - L L^T| <= 2 n u |L| |L^T| componentwise; the mirror at half of it at most"""
    G = _mirror(nb, name)
    assert np.all(np.isfinite(np.tril(G)))
    ratio = R.potrf_ratio(R.MATRICES[name](nb), G)
    print("mirror potrf nb=%d %s: %.4f of n u" % (nb, name, ratio))
    assert ratio <= 0.5 * 2


@pytest.mark.parametrize("nb,name", R.INVERSE)
def test_mirror_margin_stored_inverses(nb, name):
    """test 2: |L_tt W_t - I| <= 2 * 16 u |L_tt| |W_t|"""
    ratio = R.inverse_ratio(_mirror(nb, name))
    print("mirror inverses nb=%d %s: %.4f of 16 u" % (nb, name, ratio))
    assert ratio <= 0.5 * 2


@pytest.mark.parametrize("nb,m,name", TRSM_CASES)
def test_mirror_margin_trsm(nb, m, name):
    """test 4: |X0 - X L^T| <= 2 nb u |X| |L^T|; the tall shape on the rows the device test samples (rows are independent)"""
    G = _mirror(nb, name)
    X0 = R.rhs(m, nb)
    if m > 640:
        X0 = X0[R.sample_rows(m)]
    ratio = R.trsm_ratio(G, X0, R.mirror_trsm(G, X0))
    print("mirror trsm nb=%d m=%d %s: %.4f of nb u" % (nb, m, name, ratio))
    assert ratio <= 0.5 * 2


@pytest.mark.parametrize("n,name", R.TRSV)
def test_mirror_margin_trsv(n, name):
    """test 8: ||b - L^T x||_inf <= 4 (n + 16 kappa16) u || |L^T| |x| ||_inf, the mirror being plain 16 x 16-tile back
    substitution with explicit tile inverses"""
    G = _mirror(n, name)
    b = R.rhs(1, n)[0]
    ratio = R.trsv_ratio(G, b, R.mirror_trsv_lt(G, b))
    print("mirror trsv n=%d %s: %.3g of (n + 16 kappa16) u, kappa16 = %.3g" % (n, name, ratio, R.kappa16(G)))
    assert ratio <= 0.5 * 4


# ---------------------------------------------------------------- the mirror itself

@pytest.mark.parametrize("name", ["spd1e2", "gp1", "graded"])
def test_mirror_agrees_with_long_double(name):
    """the mirror is a Cholesky: its factor is the long-double one to a componentwise cond-sized distance, it leaves the
    tiles above the block diagonal alone and its stored inverses invert the diagonal tiles"""
    S = R.MATRICES[name](128)
    G = _mirror(128, name)
    Lref, fail, _ = R.ref_cholesky(S)
    assert fail is None
    d = np.sqrt(np.diagonal(S))
    rel = np.abs(np.tril(G) - Lref.astype(np.float64)) / d[:, None]       # |L_ij| <= sqrt(S_ii)
    assert rel.max() <= 1e-7
    up = R.upper_tiles(128)
    assert np.array_equal(G[up], S[up])
    for t in range(8):
        Lt = np.tril(G[16 * t:16 * t + 16, 16 * t:16 * t + 16])
        W = R.stored_inverse(G, t)
        assert np.all(np.abs(Lt @ W - np.eye(16)) <= 1e-10 * (np.abs(Lt) @ np.abs(W)))


def test_mirror_solves():
    """mirror_trsm and mirror_trsv_lt against NumPy's solver on a well-conditioned factor"""
    G = _mirror(128, "spd1e2")
    L = np.tril(G)
    X0 = R.rhs(128, 128)
    assert np.allclose(R.mirror_trsm(G, X0), np.linalg.solve(L, X0.T).T, rtol=0, atol=1e-9 * np.abs(X0).max() * 100)
    b = X0[0]
    assert np.allclose(R.mirror_trsv_lt(G, b), np.linalg.solve(L.T, b), rtol=0, atol=1e-9 * 100)


# ---------------------------------------------------------------- the builders

def test_matrices_are_symmetric_and_seeded():
    for name, make in R.MATRICES.items():
        S = make(128)
        assert np.array_equal(S, S.T), name
        assert not S.flags.writeable
    assert np.array_equal(R.spd(64, 1e2, seed=9), R.spd(64, 1e2, seed=9))
    assert not np.array_equal(R.spd(64, 1e2, seed=9), R.spd(64, 1e2, seed=10))
    ev = np.linalg.eigvalsh(R.spd(128, 1e10))
    assert abs(ev[-1] - 1) <= 1e-12 and abs(ev[0] * 1e10 - 1) <= 1e-4
    K = R.gp(128, 2.0, 1e-8)
    assert np.all(np.diagonal(K) == 1.0 + 1e-8) and np.all(K > 0) and np.all(K[~np.eye(128, dtype=bool)] < 1)


@pytest.mark.parametrize("n", [128, 256, 512])
def test_graded_and_scaled_are_exact_scalings(n):
    k = R.graded_exponents(n)
    assert k.min() >= -40 and k.max() <= 40
    back = np.ldexp(np.ldexp(R.graded(n), -k[:, None]), -k[None, :])
    assert np.array_equal(back, R.spd(n, 1e6))
    for e in (600, -600):
        S = R.scaled(n, e)
        assert np.all(np.isfinite(S)) and np.array_equal(np.ldexp(S, -e), R.spd(n, 1e2))
        assert np.all((S == 0) == (R.spd(n, 1e2) == 0))                     # nothing flushed to zero


ALL_PLANTED = sorted(set(R.PIVOTS_FUSED + [(j, "neg") for j in R.PIVOTS_TILE3] + R.PIVOTS_KINDS + R.PIVOTS_FIRST_GEN +
                         [(70, "neg")]))


@pytest.mark.parametrize("j,kind", ALL_PLANTED)
def test_planted_pivot_fails_exactly_there(j, kind):
    """the long-double reference meets its first pivot that is not > 0 at j -- so every leading minor of order <= j has
    positive pivots -- and the mirror agrees; nothing but S[j, j] differs from the clean matrix"""
    P = R.planted_case(j, kind)
    _, fail, pivot = R.ref_cholesky(P)
    assert fail == j
    assert R.mirror_potrf(P)[1] == j
    if kind == "neg":
        assert abs(pivot + 1) <= 1e-12
    elif kind == "nan":
        assert np.isnan(pivot)
    else:
        assert pivot == 0.0 and not np.signbit(pivot)
        assert R.mirror_potrf(P)[0][j, j] != R.mirror_potrf(P)[0][j, j]      # sqrt / rsq of an exact zero: NaN from there
    if kind != "zero":
        diff = P != R.spd(256, 1e2)
        diff[j, j] = False
        assert not diff.any()
        assert np.array_equal(P[:j, :j], R.spd(256, 1e2)[:j, :j])


@pytest.mark.parametrize("j1,j2", R.PIVOT_PAIRS)
def test_two_planted_pivots(j1, j2):
    """both planted pivots fail where they stand (the second is met once the first is repaired); the reference names the
    first"""
    P = R.planted_case(j1, "neg", j2)
    assert R.ref_cholesky(P)[1] == j1
    Q = np.array(P)
    Q[j1, j1] = R.spd(256, 1e2)[j1, j1]
    assert R.ref_cholesky(Q)[1] == j2
    assert np.array_equal(Q, R.planted_case(j2, "neg"))


def test_sample_rows():
    for m in (16512, 32896):
        rows = R.sample_rows(m)
        assert rows.shape == (512,) and len(set(rows.tolist())) == 512 and rows.max() == m - 1
        assert np.array_equal(rows[256:], np.arange(m - 256, m))
