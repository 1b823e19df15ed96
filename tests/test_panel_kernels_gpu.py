"""The Cholesky panel kernels at every launch form, through the block primitives that chain them (gpmi_dev_potrf_block,
gpmi_dev_trsm_block, gpmi_dev_trsv_lt_fused: include/gpmi.h): potrf128, the one- and two-launch forms of trsm128 and its
persistent slab loop, potf2_64, both forms of trsm_rlt64, and the recursions panel_rec / trsm_rec of driver.hip.  Each is held
to a componentwise bound against a long-double residual (tests/panel_ref.py), on matrices up to cond 1e10, graded over
2^160 and scaled by 2^+-600; the float64 mirror of the same recurrence sits under half of every bar
(tests/test_panel_ref_cpu.py).  Also: where a failing pivot is reported, the stored inverses, what the kernels must not
read, that the launch forms give the same bits, and what the host refuses.

Every test prints its worst ratio (LAB_NOTES.md, "panel kernel bounds")."""
import contextlib

import numpy as np
import pytest

import panel_ref as R
from panel_ref import SENTINEL

pytestmark = pytest.mark.gpu

PAD = -7.0                   # the columns past nb of every buffer hold it before and after each call


@pytest.fixture(scope="module")
def ops():
    from gaussian_process_amd.dist import HipBlockOps
    ops = HipBlockOps(0)
    with _forms(ops):                # whatever ran before in this thread: the defaults from here on
        pass
    return ops


def _dev(ops, a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).to(ops.device)


@contextlib.contextmanager
def _forms(ops, panel_fused=1, trsm_wave=1, concurrent=0):
    """kernel-selection state of this thread for the enclosed calls; the defaults (1, 1, off) are back afterwards whatever
    happens: the state is thread-local and outlives a test"""
    try:
        ops.set_option("panel_fused", panel_fused)
        ops.set_option("trsm_wave", trsm_wave)
        ops.set_concurrent(concurrent)
        yield
    finally:
        ops.set_option("panel_fused", 1)
        ops.set_option("trsm_wave", 1)
        ops.set_concurrent(0)


def _padded(A, pad=6):
    """A in a buffer with a padded, even leading dimension"""
    n, c = A.shape
    B = np.full((n, c + pad), PAD)
    B[:, :c] = A
    return B


def _potrf(ops, S, col_offset=0, info0=SENTINEL, **forms):
    """gpmi_dev_potrf_block on S in a padded buffer: (the nb x nb block as left, *info)"""
    import torch
    nb = S.shape[0]
    Ad = _dev(ops, _padded(S))
    info = torch.full((1,), info0, dtype=torch.int64, device=ops.device)
    with _forms(ops, **forms):
        ops.potrf_block(Ad[:, :nb], col_offset, info)
        ops.sync()
    out = Ad.cpu().numpy()
    assert np.all(out[:, nb:] == PAD), "the padding was written"
    return out[:, :nb].copy(), int(info.item())


def _trsm(ops, G, X0, **forms):
    """gpmi_dev_trsm_block with the factored block G on X0, both in padded buffers: X as left"""
    nb = G.shape[0]
    Ld, Xd = _dev(ops, _padded(G, 10)), _dev(ops, _padded(X0))
    with _forms(ops, **forms):
        ops.trsm_block(Ld[:, :nb], Xd[:, :nb])
        ops.sync()
    out = Xd.cpu().numpy()
    assert np.all(out[:, nb:] == PAD), "the padding was written"
    assert np.array_equal(Ld.cpu().numpy()[:, :nb], G, equal_nan=True), "L was written"
    return out[:, :nb].copy()


_factors = {}


def _factor(ops, nb, name, fused=1):
    """the device's factor of a case's matrix in the given path, computed once and left unchanged; nb = 192 is the leading
    block of the 256 factor (potrf_block takes multiples of 128)"""
    if nb == 192:
        return _factor(ops, 256, name, fused)[:192, :192]
    key = (nb, name, fused)
    if key not in _factors:
        G, info = _potrf(ops, R.MATRICES[name](nb), panel_fused=fused)
        assert info == SENTINEL
        G.setflags(write=False)
        _factors[key] = G
    return _factors[key]


def _lower_tiles(n):
    """everything potrf_block owns: the tiles on and below the block diagonal (stored inverses included)"""
    return ~R.upper_tiles(n)


# ---------------------------------------------------------------- 1  potrf_block, componentwise backward error

def _check_potrf(ops, nb, name, fused):
    S = R.MATRICES[name](nb)
    G = _factor(ops, nb, name, fused)
    assert np.all(np.isfinite(np.tril(G)))
    ratio = R.potrf_ratio(S, G)
    print("potrf_block %s nb=%d %s: worst |S - L L^T| / (n u |L| |L^T|) = %.4f (bar 2)"
          % ("fused" if fused else "first-generation", nb, name, ratio))
    assert ratio <= 2, ratio
    return G


@pytest.mark.parametrize("nb,name", R.POTRF_FUSED)
def test_potrf_block_componentwise(ops, nb, name):
    """|S - L L^T|_ij <= 2 n u (|L| |L^T|)_ij for every i >= j: potrf128 alone (nb 128), with trsm128 and the inner update
    (256), the uneven 128 + 256 split of panel_rec (384), two levels (512), three and a K = 512 update (1024).  The bound is
    scale-free: at 2^+-600 nothing may overflow, underflow or flag a pivot either."""
    G = _check_potrf(ops, nb, name, 1)
    if name.startswith("scaled"):
        e = 600 if name.endswith("+600") else -600
        same = np.array_equal(np.tril(G), np.ldexp(np.tril(_factor(ops, nb, "spd1e2", 1)), e // 2))
        print("potrf_block nb=%d: L(2^%d S) == 2^%d L(S) bit for bit: %s" % (nb, e, e // 2, same))


@pytest.mark.parametrize("nb,name", R.POTRF_FIRST_GEN)
def test_potrf_block_first_generation_componentwise(ops, nb, name):
    """the same bound for potf2_64 + trsm_rlt64 + rank-64 updates (option panel_fused = 0)"""
    _check_potrf(ops, nb, name, 0)


# ---------------------------------------------------------------- 2  the stored inverses

@pytest.mark.parametrize("nb,name", R.INVERSE)
def test_stored_inverses(ops, nb, name):
    """W_t^T sits in the strict upper triangle of diagonal tile t (diag(W_t) = 1 / diag(L_tt) implied) and inverts it:
    |L_tt W_t - I|_ij <= 2 * 16 u (|L_tt| |W_t|)_ij over the lower triangle.  The tiles strictly above the block diagonal
    are not written: a planted value is still there, and the factor does not depend on it."""
    S = np.array(R.MATRICES[name](nb))
    up = R.upper_tiles(nb)
    S[up] = 12345.6789
    G, info = _potrf(ops, S)
    assert info == SENTINEL
    assert np.all(G[up] == 12345.6789)
    assert np.array_equal(G[~up], _factor(ops, nb, name)[~up])
    ratio = R.inverse_ratio(G)
    print("stored inverses nb=%d %s: worst |L_tt W_t - I| / (16 u |L_tt| |W_t|) = %.4f (bar 2)" % (nb, name, ratio))
    assert ratio <= 2, ratio


# ---------------------------------------------------------------- 3  what is not read

@pytest.mark.parametrize("fused,nb,name", [(1, 512, "spd1e10"), (0, 256, "spd1e10")])
def test_potrf_block_does_not_read_above_the_diagonal_tiles(ops, fused, nb, name):
    """the symmetric K build writes only tiles on or below the diagonal; above them sits whatever an earlier fit left, NaN
    after a failed one.  With NaN in every 16 x 16 tile strictly above the diagonal (the diagonal tiles symmetric, as the
    build writes them) the lower triangle -- and on the fused path the stored inverses -- are the clean run's bits."""
    S = np.array(R.MATRICES[name](nb))
    S[R.upper_tiles(nb)] = np.nan
    G, info = _potrf(ops, S, panel_fused=fused)
    assert info == SENTINEL
    clean = _factor(ops, nb, name, fused)
    assert np.array_equal(np.tril(G), np.tril(clean))
    if fused:
        own = _lower_tiles(nb)
        assert np.array_equal(G[own], clean[own])


def test_trsm_block_does_not_read_above_the_diagonal_tiles(ops):
    """trsm_block reads the tiles below the diagonal and the diagonal tiles with their stored inverses, nothing above"""
    nb, m = 256, 640
    clean = _factor(ops, nb, "spd1e10")
    G = np.array(clean)
    G[R.upper_tiles(nb)] = np.nan
    X0 = R.rhs(m, nb)
    assert np.array_equal(_trsm(ops, G, X0), _trsm(ops, clean, X0))


# ---------------------------------------------------------------- 4  trsm_block, componentwise backward error

def _check_trsm(ops, G, X0, X, what, rows=None):
    assert np.all(np.isfinite(X))
    ratio = R.trsm_ratio(G, X0, X, rows)
    print("trsm_block %s: worst |X0 - X L^T| / (nb u |X| |L^T|) = %.4f (bar 2)" % (what, ratio))
    assert ratio <= 2, ratio
    return ratio


@pytest.mark.parametrize("nb,m,name", R.TRSM_FUSED)
def test_trsm_block_componentwise(ops, nb, m, name):
    """|X0 - X L^T|_rc <= 2 nb u (|X| |L^T|)_rc: one-launch trsm128 (nb 128) and trsm_rec with its updates (256, 512), one
    slab pair (m 128) and ten slabs (640)"""
    G = _factor(ops, nb, name)
    X0 = R.rhs(m, nb)
    _check_trsm(ops, G, X0, _trsm(ops, G, X0), "fused nb=%d m=%d %s" % (nb, m, name))


@pytest.mark.parametrize("nb,m,name", R.TRSM_NB192)
def test_trsm_block_64_wide_leaves_on_a_fused_factor(ops, nb, m, name):
    """nb = 192 is no multiple of 128: trsm_rec takes the first-generation 64-column leaves, which read only the lower
    triangle of a factor that carries inverses"""
    G = _factor(ops, nb, name)
    X0 = R.rhs(m, nb)
    _check_trsm(ops, G, X0, _trsm(ops, G, X0), "nb=192 m=%d %s" % (m, name))


@pytest.mark.parametrize("nb,m,name", R.TRSM_FIRST_GEN)
def test_trsm_block_first_generation_componentwise(ops, nb, m, name):
    """panel_fused = 0 on a factor made with panel_fused = 0 (such a factor has no stored inverses).  m 128 / 640: the
    wave-per-row kernel (trsm_wave 1) and the lane-per-row kernel (trsm_wave 0); m = 16512, the smallest multiple of 128
    above 16384: the lane-per-row kernel by size, under the default trsm_wave.  Same bound.

    trsm_wave 0 against 1, bit for bit: asserted.  Read in panel.hip: both kernels compute, per row, for C = 0..63
    xc = x[C] * (1.0 / L[C][C]), then x[c'] = fma(-xc, L[c'][C], x[c']) for every c' > C -- the same operations on the same
    operands in the same order for each element; only the lane that holds an element differs."""
    G = _factor(ops, nb, name, 0)
    X0 = R.rhs(m, nb)
    what = "first-generation nb=%d m=%d %s" % (nb, m, name)
    if m > 16384:
        X = _trsm(ops, G, X0, panel_fused=0)
        _check_trsm(ops, G, X0, X, what + " lane-per-row by size", None if nb == 128 else R.sample_rows(m))
        return
    Xw = _trsm(ops, G, X0, panel_fused=0, trsm_wave=1)
    Xl = _trsm(ops, G, X0, panel_fused=0, trsm_wave=0)
    if m == 640:
        _check_trsm(ops, G, X0, Xw, what + " wave-per-row")
    _check_trsm(ops, G, X0, Xl, what + " lane-per-row")
    if m == 640:
        assert np.array_equal(Xw, Xl)


# ---------------------------------------------------------------- 5  the launch forms give the same bits

@pytest.mark.parametrize("m", [128, 640, 32896])
@pytest.mark.parametrize("nb", [128, 256, 512])
def test_trsm_block_concurrent_forms_same_bits(ops, nb, m):
    """gpmi_dev_set_concurrent(1): trsm128 as two small-LDS launches (columns 0..63 with their updates, then 64..127) and the
    shallow-ring inner updates -- the same bits as the one-launch form.  m = 32896 = 257 * 128 gives 514 slabs of 64 rows,
    the smallest size at which a workgroup of the 512-workgroup grid takes a second slab (the reload branch of the
    persistent loop): there the last 256 rows, which only the wrap reaches, and 256 sampled from the rest are held to the
    bound of test 4 as well."""
    G = _factor(ops, nb, "spd1e10")
    X0 = R.rhs(m, nb)
    one = _trsm(ops, G, X0, concurrent=0)
    two = _trsm(ops, G, X0, concurrent=1)
    assert np.array_equal(one, two)
    rows = R.sample_rows(m) if m > 640 else None
    _check_trsm(ops, G, X0, two, "two-launch nb=%d m=%d spd1e10" % (nb, m), rows)


@pytest.mark.parametrize("nb", [256, 512])
def test_potrf_block_concurrent_forms_same_bits(ops, nb):
    """the factorisation of a block under gpmi_dev_set_concurrent(1) (two-launch trsm128 below every potrf128, shallow-ring
    updates): the whole block has the same bits, the tiles above the block diagonal that the inner updates pass over included"""
    G, info = _potrf(ops, R.MATRICES["spd1e10"](nb), concurrent=1)
    assert info == SENTINEL
    assert np.array_equal(G, _factor(ops, nb, "spd1e10"))


# ---------------------------------------------------------------- 6  the failing pivot

OFF = 1000


def _check_pivot(ops, j, kind, j2=None, fused=1, col_offset=OFF):
    """info == col_offset + the pivot the long-double reference fails at; on the fused path the columns left of the failing
    pivot's tile are the clean factor's (only S[j, j] differs from the clean matrix, so they saw the same inputs)"""
    P = R.planted_case(j, kind, j2)
    expect = R.ref_cholesky(P)[1]
    assert expect == j                                     # tests/test_panel_ref_cpu.py holds the builder to this
    G, info = _potrf(ops, P, col_offset, panel_fused=fused)
    assert info == col_offset + expect, "pivot %d (%s): info - col_offset = %d" % (j, kind, info - col_offset)
    if fused and kind != "zero":
        cols = np.arange(256)[None, :] < 16 * (j // 16)
        own = _lower_tiles(256) & cols
        assert np.array_equal(G[own], _factor(ops, 256, "spd1e2")[own])


@pytest.mark.parametrize("j,kind", R.PIVOTS_FUSED + R.PIVOTS_KINDS)
def test_failing_pivot_is_reported_at_its_column(ops, j, kind):
    """nb = 256, col_offset = 1000: first / last column of a tile, of a 128 block, of the block; inside the second leaf of
    the recursion; a pivot of -1, a NaN pivot and an exact zero (rsq(0) = inf, 0 * inf = NaN)"""
    _check_pivot(ops, j, kind)


def test_failing_pivot_every_position_in_a_tile(ops):
    """all 16 columns of tile 3"""
    for j in R.PIVOTS_TILE3:
        _check_pivot(ops, j, "neg")


@pytest.mark.parametrize("j1,j2", R.PIVOT_PAIRS)
def test_two_failing_pivots_report_the_first(ops, j1, j2):
    """two planted pivots, in different potrf128 launches and in one tile: the atomic min keeps the first"""
    _check_pivot(ops, j1, "neg", j2)


def test_failing_pivot_beyond_2_31(ops):
    """col_offset = 3 * 2^31 + 5: the min is taken on 64 bits"""
    _check_pivot(ops, 70, "neg", col_offset=3 * 2 ** 31 + 5)


def test_failing_pivot_keeps_a_smaller_info(ops):
    """*info already holds an earlier column (another block's): it stays"""
    _, info = _potrf(ops, R.planted_case(70, "neg"), OFF, info0=5)
    assert info == 5
    _, info = _potrf(ops, R.planted_case(70, "neg"), OFF, info0=OFF + 71)
    assert info == OFF + 70


@pytest.mark.parametrize("j,kind", R.PIVOTS_FIRST_GEN)
def test_failing_pivot_first_generation(ops, j, kind):
    """potf2_64: first / last column of a 64 leaf, of the 128-column half, inside the last leaf"""
    _check_pivot(ops, j, kind, fused=0)


# ---------------------------------------------------------------- 7  refusals on the host

def test_misaligned_views_are_refused(ops):
    """a view that starts on an odd column of an even-ld buffer is 8 bytes off the 16-byte loads of potrf128 / trsm128:
    launch_potrf128 / launch_trsm128 test the pointer before any launch (default fused path only -- the first-generation
    launcher has no such test).  The call fails and the buffers are as they were."""
    import torch
    nb = 128
    host = _padded(R.MATRICES["spd1e2"](nb), 8)
    G = _padded(_factor(ops, nb, "spd1e2"), 8)
    Ad, Ld, Xd = _dev(ops, host), _dev(ops, G), _dev(ops, host)
    info = torch.full((1,), SENTINEL, dtype=torch.int64, device=ops.device)
    with pytest.raises((RuntimeError, ValueError)):
        ops.potrf_block(Ad[:, 1:nb + 1], 0, info)
    with pytest.raises((RuntimeError, ValueError)):
        ops.trsm_block(Ld[:, 1:nb + 1], Xd[:, :nb])
    with pytest.raises((RuntimeError, ValueError)):
        ops.trsm_block(Ld[:, :nb], Xd[:, 1:nb + 1])
    ops.sync()
    assert np.array_equal(Ad.cpu().numpy(), host) and np.array_equal(Xd.cpu().numpy(), host)
    assert np.array_equal(Ld.cpu().numpy(), G) and int(info.item()) == SENTINEL


def test_bad_sizes_are_refused(ops):
    """odd ld, nb % 128 != 0 (potrf_block; trsm_block takes multiples of 64) and m % 128 != 0: ValueError, nothing runs"""
    import torch
    host = _padded(R.MATRICES["spd1e2"](256), 6)
    Ad, Xd = _dev(ops, host), _dev(ops, host)
    odd = _dev(ops, _padded(R.MATRICES["spd1e2"](128), 7))
    info = torch.full((1,), SENTINEL, dtype=torch.int64, device=ops.device)
    with pytest.raises(ValueError):
        ops.potrf_block(odd[:, :128], 0, info)                          # odd ld
    with pytest.raises(ValueError):
        ops.potrf_block(Ad[:192, :192], 0, info)                        # nb % 128
    with pytest.raises(ValueError):
        ops.potrf_block(Ad[:64, :64], 0, info)
    with pytest.raises(ValueError):
        ops.trsm_block(odd[:, :128], Xd[:128, :128])                    # odd ldl
    with pytest.raises(ValueError):
        ops.trsm_block(Ad[:128, :128], odd[:, :128])                    # odd ldx
    with pytest.raises(ValueError):
        ops.trsm_block(Ad[:128, :128], Xd[:192, :128])                  # m % 128
    with pytest.raises(ValueError):
        ops.trsm_block(Ad[:96, :96], Xd[:128, :96])                     # nb % 64
    ops.sync()
    assert np.array_equal(Ad.cpu().numpy(), host) and np.array_equal(Xd.cpu().numpy(), host)
    assert int(info.item()) == SENTINEL


# ---------------------------------------------------------------- 8  gpmi_dev_trsv_lt_fused

@pytest.mark.parametrize("n,name", R.TRSV)
def test_trsv_lt_fused_normwise_backward_error(ops, n, name):
    """the regression path's backward solve under trsv_vinv = 0.  solve.hip (trsv_lt_step128_kernel): one launch per 128
    unknowns, and inside a diagonal block 16 x 16 rounds with the tiles' stored inverses -- for s = 7..0:
    x_s = W_ss^T r_s;  r_t -= L_st^T x_s (t < s).  x_s comes from a computed inverse, so the residual grows with the
    condition of a 16 x 16 tile: the bar of test_trsv_lt_vinv_normwise_backward_error with 16 in place of 128,
        ||b - L^T x||_inf <= 4 (n + 16 kappa16) u || |L^T| |x| ||_inf,   kappa16 = max cond_inf of a diagonal tile of L.
    The tiles above the block diagonal are NaN (not read); the factor and its inverses are unchanged; b is scratch."""
    import torch
    from gaussian_process_amd._lib import check
    clean = _factor(ops, n, name)
    G = np.array(clean)
    G[R.upper_tiles(n)] = np.nan
    Ld = _dev(ops, _padded(G, 10))
    b = R.rhs(1, n)[0]
    bd = _dev(ops, b)
    xd = torch.full((n,), np.nan, dtype=torch.float64, device=ops.device)
    check(ops.lib.gpmi_dev_trsv_lt_fused(ops._stream(), ops._p(Ld), Ld.stride(0), ops._p(bd), ops._p(xd), n))
    ops.sync()
    x = xd.cpu().numpy()
    assert np.all(np.isfinite(x))
    ratio = R.trsv_ratio(clean, b, x)
    print("trsv_lt_fused n=%d %s: ||b - L^T x|| / ((n + 16 kappa16) u || |L^T| |x| ||) = %.3g (bar 4), kappa16 = %.3g"
          % (n, name, ratio, R.kappa16(clean)))
    assert ratio <= 4, ratio
    back = Ld.cpu().numpy()
    assert np.array_equal(back[:, :n], G, equal_nan=True) and np.all(back[:, n:] == PAD)
