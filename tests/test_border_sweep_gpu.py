"""The forward sweep for at most 16 rows (border_sweep_kernel of panel_mfma.hip) through gpmi_dev_border_sweep: X <- X L^-T
for a fused factor L, one launch per 128 columns.  It runs trsm128's recurrence, so it is held to trsm_block's bar
(tests/panel_ref.py: |X0 - X L^T| <= 2 nb u |X| |L^T| componentwise, the residual in long double) on the matrices and
the factors tests/test_panel_kernels_gpu.py uses -- and in the same test trsm_block itself, on the same rows padded to 128,
is held to it too, so a miss of both points at the input.  Also: the same bits run to run, nothing read or written
outside rows x ncols, nothing read above the diagonal but the diagonal 16 x 16 tiles, and what the host refuses.

Every test prints its worst ratio."""
import numpy as np
import pytest

import panel_ref as R
from panel_ref import SENTINEL

pytestmark = pytest.mark.gpu

PAD = -7.0
NCOLS = (128, 256, 640, 1152)        # one block; two; an odd count; more blocks than a 1024-wide outer block
ROWS = (1, 5, 16)
NAMES = ("spd1e2", "spd1e10", "graded", "gp2")


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


_factors = {}


def _factor(ops, n, name):
    """the device's fused factor of a case's matrix (gpmi_dev_potrf_block, as test_panel_kernels_gpu.py makes them), once"""
    import torch
    key = (n, name)
    if key not in _factors:
        S = R.MATRICES[name](n)
        Ad = _dev(ops, np.hstack([S, np.full((n, 6), PAD)]))
        info = torch.full((1,), SENTINEL, dtype=torch.int64, device=ops.device)
        ops.potrf_block(Ad[:, :n], 0, info)
        ops.sync()
        assert int(info.item()) == SENTINEL
        G = Ad.cpu().numpy()[:, :n].copy()
        G.setflags(write=False)
        _factors[key] = G
    return _factors[key]


def _sweep(ops, G, X0, lpad=10, xpad=6):
    """gpmi_dev_border_sweep on X0 (rows x ncols) inside a buffer with a sentinel row above, two below and xpad sentinel
    columns (ldx != ncols): X as left, after checking that the sentinels and L are untouched"""
    n = G.shape[0]
    rows = X0.shape[0]
    buf = np.full((rows + 3, n + xpad), PAD)
    buf[1:1 + rows, :n] = X0
    Ld = _dev(ops, np.hstack([G, np.full((n, lpad), PAD)]))
    Xd = _dev(ops, buf)
    ops.border_sweep(Ld[:, :n], Xd[1:1 + rows, :n])
    ops.sync()
    out = Xd.cpu().numpy()
    assert np.all(out[0] == PAD) and np.all(out[1 + rows:] == PAD), "a row outside X was written"
    assert np.all(out[:, n:] == PAD), "a column outside X was written"
    assert np.array_equal(Ld.cpu().numpy()[:, :n], G, equal_nan=True), "L was written"
    return out[1:1 + rows, :n].copy()


def _trsm_padded(ops, G, X0):
    """the existing gpmi_dev_trsm_block on the same rows, padded with zero rows to 128"""
    n = G.shape[0]
    Xp = np.zeros((128, n + 6))
    Xp[:X0.shape[0], :n] = X0
    Ld, Xd = _dev(ops, np.hstack([G, np.full((n, 10), PAD)])), _dev(ops, Xp)
    ops.trsm_block(Ld[:, :n], Xd[:, :n])
    ops.sync()
    return Xd.cpu().numpy()[:X0.shape[0], :n].copy()


@pytest.mark.parametrize("ncols,name", [(n, name) for n in NCOLS for name in NAMES])
def test_border_sweep_componentwise(ops, ncols, name):
    """|X0 - X L^T|_rc <= 2 ncols u (|X| |L^T|)_rc for 1, 5 and 16 rows, and for trsm_block on the same rows"""
    G = _factor(ops, ncols, name)
    for rows in ROWS:
        X0 = R.rhs(rows, ncols)
        X = _sweep(ops, G, X0)
        assert np.all(np.isfinite(X))
        ratio = R.trsm_ratio(G, X0, X)
        ref = R.trsm_ratio(G, X0, _trsm_padded(ops, G, X0))
        print("border_sweep ncols=%d rows=%d %s: worst |X0 - X L^T| / (nb u |X| |L^T|) = %.4f, trsm_block %.4f (bar 2)"
              % (ncols, rows, name, ratio, ref))
        assert ref <= 2, "the existing trsm_block misses the bar on this input: %g" % ref
        assert ratio <= 2, ratio


@pytest.mark.parametrize("ncols,rows", [(640, 5), (1152, 16)])
def test_border_sweep_same_bits_every_run(ops, ncols, rows):
    G = _factor(ops, ncols, "spd1e10")
    X0 = R.rhs(rows, ncols)
    a, b = _sweep(ops, G, X0), _sweep(ops, G, X0)
    assert np.array_equal(a, b)


@pytest.mark.parametrize("ncols,rows", [(256, 1), (640, 16)])
def test_border_sweep_reads_no_block_upper_tile(ops, ncols, rows):
    """after a backward solve the block-upper tiles of every 128 x 128 diagonal block hold L_kk^-T, and above the block
    diagonal sits whatever an earlier fit left: with NaN in every 16 x 16 tile strictly above the diagonal the result is
    the clean run's, bit for bit"""
    clean = _factor(ops, ncols, "spd1e10")
    G = np.array(clean)
    G[R.upper_tiles(ncols)] = np.nan
    X0 = R.rhs(rows, ncols)
    assert np.array_equal(_sweep(ops, G, X0), _sweep(ops, clean, X0))


def test_border_sweep_leading_columns_only(ops):
    """ncols below the factor's size: the leading block of a larger factor (what gpmi_append sweeps through), nothing
    beyond column ncols read or written"""
    G = _factor(ops, 640, "spd1e2")
    X0 = R.rhs(3, 640)
    n = 384
    Ld = _dev(ops, np.hstack([G, np.full((640, 10), PAD)]))
    buf = np.full((4, 646), PAD)
    buf[:3, :640] = X0
    Xd = _dev(ops, buf)
    ops.border_sweep(Ld[:, :640], Xd[:3, :640], ncols=n)
    ops.sync()
    out = Xd.cpu().numpy()
    assert np.array_equal(out[:3, n:640], X0[:, n:]) and np.all(out[3] == PAD) and np.all(out[:, 640:] == PAD)
    assert np.array_equal(out[:3, :n], _sweep(ops, np.array(G[:n, :n]), X0[:, :n]))


def test_border_sweep_refusals(ops):
    """rows of 0 or 17, an odd leading dimension and ncols that is no multiple of 128 are refused with nothing launched"""
    G = _factor(ops, 128, "spd1e2")
    Ld = _dev(ops, np.hstack([G, np.full((128, 10), PAD)]))
    X0 = np.full((20, 134), 3.0)
    Xd = _dev(ops, X0)
    Lodd = _dev(ops, np.hstack([G, np.full((128, 9), PAD)]))
    Xodd = _dev(ops, np.full((20, 133), 3.0))
    for call in (lambda: ops.border_sweep(Ld[:, :128], Xd[:, :128], rows=0),
                 lambda: ops.border_sweep(Ld[:, :128], Xd[:, :128], rows=17),
                 lambda: ops.border_sweep(Ld[:, :128], Xd[:, :128], rows=-1),
                 lambda: ops.border_sweep(Lodd[:, :128], Xd[:, :128], rows=4),
                 lambda: ops.border_sweep(Ld[:, :128], Xodd[:, :128], rows=4),
                 lambda: ops.border_sweep(Ld[:, :128], Xd[:, :128], rows=4, ncols=64),
                 lambda: ops.border_sweep(Ld[:, :128], Xd[:, :128], rows=4, ncols=130),
                 lambda: ops.border_sweep(Ld[:, :128], Xd[:, :128], rows=4, ncols=256)):
        with pytest.raises(ValueError):
            call()
    ops.sync()
    assert np.array_equal(Xd.cpu().numpy(), X0)
