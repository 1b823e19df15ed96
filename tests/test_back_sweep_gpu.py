"""The backward sweep (back_sweep_kernel of panel_mfma.hip) through gpmi_dev_back_sweep: X <- X L^-1 for a fused factor L,
row i becoming L^-T x_i, one launch per 128 columns from the last block to the first, any number of rows.

L is the device's own fused factor (gpmi_dev_potrf_block) of a well-conditioned random SPD matrix (panel_ref "spd1e2":
condition 1e2); the reference is a long-double triangular solve with its lower triangle.  Bar: 1e-12 of the row's largest
element.  It rests on what float64 itself misses of that reference: scipy's solve_triangular on the same L is off by
1.1e-15 (ncols = 128) to 1.3e-15 (ncols = 1152) of the row's largest element, measured on the CPU with NumPy's factor of the
same matrices and printed again by every case for the device's factor -- the bar leaves nearly three orders of magnitude
over it for another summation order and for products with the stored 16 x 16 inverses in place of divisions.

Also: NaN in every 16 x 16 tile strictly above the diagonal tiles, in the rows of X from `rows` on and in the columns
from ncols on changes nothing and stays bit for bit; two runs give the same bits; what the host refuses; ncols = 0."""
import numpy as np
import pytest
from scipy.linalg import solve_triangular

import panel_ref as R
import predict_ref as P
import sgpr_ref as S
from panel_ref import SENTINEL

pytestmark = pytest.mark.gpu

PAD = -7.0
NCOLS = (128, 256, 640, 1152)        # one block; two; an odd count; more blocks than a 1024-wide outer block
ROWS = (1, 7, 16, 17, 40)            # one row; a partial group; a whole one; one more; two and a half
BAR = 1e-12


@pytest.fixture(scope="module")
def ops():
    from gaussian_process_amd.dist import HipBlockOps
    ops = HipBlockOps(0)
    ops.set_option("panel_fused", 1)
    ops.set_option("trsm_wave", 1)
    ops.set_concurrent(0)
    return ops


def _dev(ops, a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).to(ops.device)


_factors, _refs = {}, {}


def _factor(ops, n):
    """the device's fused factor of spd1e2 (stored inverses above the diagonals of its 16 x 16 diagonal tiles), once"""
    import torch
    if n not in _factors:
        Ad = _dev(ops, np.hstack([R.MATRICES["spd1e2"](n), np.full((n, 6), PAD)]))
        info = torch.full((1,), SENTINEL, dtype=torch.int64, device=ops.device)
        ops.potrf_block(Ad[:, :n], 0, info)
        ops.sync()
        assert int(info.item()) == SENTINEL
        G = Ad.cpu().numpy()[:, :n].copy()
        G.setflags(write=False)
        _factors[n] = G
    return _factors[n]


def _reference(G, ncols):
    """(X0, X0 L^-1 in long double, float64's own miss) for the 40 rows every case takes its rows from, once per ncols"""
    if ncols not in _refs:
        X0 = R.rhs(max(ROWS), ncols)
        L = np.tril(G)
        _, solve_lower = S._ops(np.longdouble)
        ref = P.solve_upper_t(solve_lower, L.astype(np.longdouble), X0.T.astype(np.longdouble)).T
        f64 = solve_triangular(L, X0.T, lower=True, trans="T").T
        _refs[ncols] = (X0, ref, _miss(f64, ref))
    return _refs[ncols]


def _miss(X, ref):
    ref = np.asarray(ref, dtype=np.longdouble)
    return float(np.max(np.max(np.abs(X - ref), axis=1) / np.max(np.abs(ref), axis=1)))


def _sweep(ops, G, X0, poison=False, extra_rows=3, xpad=6):
    """gpmi_dev_back_sweep on X0 inside a buffer with extra rows below and xpad columns beside it (ldx != ncols), filled
    with a sentinel -- or NaN: then the tiles of L strictly above its diagonal tiles are NaN as well.  Returns X after
    checking that nothing outside rows x ncols and nothing of L changed."""
    n = G.shape[0]
    rows = X0.shape[0]
    fill = np.nan if poison else PAD
    buf = np.full((rows + extra_rows, n + xpad), fill)
    buf[:rows, :n] = X0
    Lh = np.hstack([G, np.full((n, 10), fill)])
    if poison:
        Lh[:, :n][R.upper_tiles(n)] = np.nan
    Ld, Xd = _dev(ops, Lh), _dev(ops, buf)
    ops.back_sweep(Ld[:, :n], Xd[:rows, :n])
    ops.sync()
    out = Xd.cpu().numpy()
    assert np.array_equal(out[rows:], buf[rows:], equal_nan=True), "a row outside X was written"
    assert np.array_equal(out[:, n:], buf[:, n:], equal_nan=True), "a column outside X was written"
    assert np.array_equal(Ld.cpu().numpy(), Lh, equal_nan=True), "L was written"
    return out[:rows, :n].copy()


@pytest.mark.parametrize("ncols", NCOLS)
def test_back_sweep_against_long_double(ops, ncols):
    G = _factor(ops, ncols)
    X0, ref, f64_miss = _reference(G, ncols)
    for rows in ROWS:
        X = _sweep(ops, G, X0[:rows])
        assert np.all(np.isfinite(X))
        miss = _miss(X, ref[:rows])
        print("back_sweep ncols=%d rows=%d: |X - ref| / max|row| = %.2e (float64 solve_triangular %.2e, bar %.0e)"
              % (ncols, rows, miss, f64_miss, BAR))
        assert miss <= BAR, miss


@pytest.mark.parametrize("ncols,rows", [(256, 1), (640, 17), (1152, 40)])
def test_back_sweep_reads_and_writes_nothing_else(ops, ncols, rows):
    """NaN above the diagonal tiles of L, below the rows and beside the columns of X: the clean run's result, bit for bit,
    and the NaN where it was"""
    G = _factor(ops, ncols)
    X0 = _reference(G, ncols)[0][:rows]
    clean, dirty = _sweep(ops, G, X0), _sweep(ops, G, X0, poison=True)
    assert np.all(np.isfinite(dirty))
    assert np.array_equal(clean, dirty)


@pytest.mark.parametrize("ncols,rows", [(640, 7), (1152, 40)])
def test_back_sweep_same_bits_every_run(ops, ncols, rows):
    G = _factor(ops, ncols)
    X0 = _reference(G, ncols)[0][:rows]
    assert np.array_equal(_sweep(ops, G, X0), _sweep(ops, G, X0))


def test_back_sweep_leading_columns_only(ops):
    """ncols below the factor's size: the leading block of a larger factor, nothing beyond column ncols read or written"""
    G = _factor(ops, 640)
    X0 = _reference(G, 640)[0][:19]
    n = 384
    Ld = _dev(ops, np.hstack([G, np.full((640, 10), PAD)]))
    buf = np.full((20, 646), PAD)
    buf[:19, :640] = X0
    Xd = _dev(ops, buf)
    ops.back_sweep(Ld[:, :640], Xd[:19, :640], ncols=n)
    ops.sync()
    out = Xd.cpu().numpy()
    assert np.array_equal(out[:19, n:640], X0[:, n:]) and np.all(out[19] == PAD) and np.all(out[:, 640:] == PAD)
    assert np.array_equal(out[:19, :n], _sweep(ops, np.array(G[:n, :n]), X0[:, :n]))


def test_back_sweep_refusals_and_no_columns(ops):
    """rows of 0, an odd leading dimension, a pointer off a 16-byte boundary and ncols that is no multiple of 128 or
    exceeds a leading dimension are refused with nothing launched; ncols = 0 does nothing"""
    G = _factor(ops, 128)
    Ld = _dev(ops, np.hstack([G, np.full((128, 10), PAD)]))
    X0 = np.full((20, 134), 3.0)
    Xd = _dev(ops, X0)
    Lodd = _dev(ops, np.hstack([G, np.full((128, 9), PAD)]))
    Xodd = _dev(ops, np.full((20, 133), 3.0))
    for call in (lambda: ops.back_sweep(Ld[:, :128], Xd[:, :128], rows=0),
                 lambda: ops.back_sweep(Ld[:, :128], Xd[:, :128], rows=-1),
                 lambda: ops.back_sweep(Lodd[:, :128], Xd[:, :128], rows=4),
                 lambda: ops.back_sweep(Ld[:, :128], Xodd[:, :128], rows=4),
                 lambda: ops.back_sweep(Ld[:, 1:129], Xd[:, :128], rows=4, ncols=128),
                 lambda: ops.back_sweep(Ld[:, :128], Xd[:, 1:129], rows=4, ncols=128),
                 lambda: ops.back_sweep(Ld[:, :128], Xd[:, :128], rows=4, ncols=64),
                 lambda: ops.back_sweep(Ld[:, :128], Xd[:, :128], rows=4, ncols=130),
                 lambda: ops.back_sweep(Ld[:, :128], Xd[:, :128], rows=4, ncols=256)):
        with pytest.raises(ValueError):
            call()
    ops.back_sweep(Ld[:, :128], Xd[:, :128], rows=4, ncols=0)
    ops.sync()
    assert np.array_equal(Xd.cpu().numpy(), X0)
