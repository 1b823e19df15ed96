"""Every route of the kernel-matrix build (gaussian_process_amd/csrc/rbf.hip) on the GPU, at the cases of
kbuild_route_table.py (tests/test_kbuild_route_cpu.py proves on the CPU that each case reaches the kernel and the
tile forms it claims):

  (a) the device exps against their exact emulation (kbuild_ref.py), bit for bit over the directed argument set;
  (b) placement invariance: an in-domain K[i, j] is a function of (A[i], B[j], parameters) only, bit for bit;
  (c) variants that must not change a bit: sigma, a far row that switches the domain test on, rbf_blocks, symmetric rows;
  (d) every (F, d) route against sig2 P(t) exp(x) in long double, at the bars derived in kbuild_ref.py;
  (e) the 4-tile strip against strip-1 chunks of the same matrix, compared on the device.

Everything in (a) for in-domain arguments and all of (b), (c), (e) is equality of bits.  Worst measured errors of (d)
are printed per route (pytest -s)."""
import contextlib

import numpy as np
import pytest

import kbuild_ref as R
import kbuild_route_table as T
import matern_ref as M
from numpy_block_ops import NumpyBlockOps

pytestmark = pytest.mark.gpu

COV_RTOL = 2e-14        # tests/test_block_primitives_gpu.py: kinds 1-3, sin, pow and several exps per element
CANARY = -7.0
KIND_FAMILY = {k: F for F, k in T.FAMILY_KIND.items()}


@pytest.fixture(scope="module")
def ops():
    from gaussian_process_amd.dist import HipBlockOps
    return HipBlockOps(0)


@pytest.fixture(scope="module")
def kctx():
    """a context of this module's own: rbf_blocks is context state"""
    from gaussian_process_amd import GPContext
    c = GPContext(0)
    yield c
    c.close()


def _dev(ops, a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.float64)).to(ops.device)


@contextlib.contextmanager
def rbf_blocks(kctx, ops, b):
    """rbf_blocks = b for the context's calls and for this thread's block primitives; the default afterwards"""
    try:
        if b is not None:
            kctx.set_option("rbf_blocks", b)
            ops.set_option("rbf_blocks", b)
        yield
    finally:
        kctx.set_option("rbf_blocks", T.RBF_BLOCKS)
        ops.set_option("rbf_blocks", T.RBF_BLOCKS)


def cov(kctx, kind, A, B, sigma, ell):
    name = T.KIND_NAME[kind]
    if name == "co2":
        return kctx.cov("co2", A, B, T.CO2)
    if not T.stationary(kind):
        return kctx.cov(name, A, B, *T.OTHER_PARAMS[kind])
    return kctx.cov(name, A, B, sigma, ell)


def run(case, kctx, ops):
    """the launch of a case -> (what it wrote, A, B): the nA x nB matrix for cov, the nrows x (ncols + 6) buffer for the
    block primitives (filled with a canary first)"""
    import torch
    A, B = T.inputs(case)
    with rbf_blocks(kctx, ops, case.blocks):
        if case.api == "cov":
            return cov(kctx, case.kind, A, B, case.sigma, case.ell), A, B
        out = torch.full((case.nrows, case.ncols + 6), CANARY, dtype=torch.float64, device=ops.device)
        view = out[:, :case.ncols]
        if case.api == "rows":
            if case.kind == 0:
                ops.rbf_rows(_dev(ops, A), case.nA, case.d, case.row0, case.nrows, case.ncols, case.sigma, case.ell, T.NOISE, view)
            else:
                ops.cov_rows(case.kind, T.params(case), _dev(ops, A), case.nA, case.d, case.row0, case.nrows, case.ncols, T.NOISE, view)
        elif case.kind == 0:
            ops.rbf_cross(_dev(ops, A), case.nA, _dev(ops, B), case.nB, case.d, case.nrows, case.ncols, case.sigma, case.ell, view)
        else:
            ops.cov_cross(case.kind, T.params(case), _dev(ops, A), case.nA, _dev(ops, B), case.nB, case.d, 0, False, case.nrows,
                          case.ncols, view)
        ops.sync()
        return out.cpu().numpy(), A, B


def arguments(case, A, B):
    """the exp argument of every real element, from the mirror whose bits the device reproduces (matern_ref.sq_cross)"""
    sq = M.sq_cross(A, B)
    return T.coef(case) * (sq if case.kind == 0 else np.sqrt(sq))


def exp_bar(case):
    """the fast exp of the kernel a case reaches"""
    return R.E_TAB if case.d in T.REG_D else R.E_FAST


def hold_values(got, x, case, what):
    """in-domain elements against the long-double value at (2 E + m) u; waves (one row x one 128-column tile) with a lane
    outside [-700, 0] took the library exp: E_LIB, the suite's atol for subnormal results, exactly 0 from -746 down"""
    F, sig2 = KIND_FAMILY[case.kind], case.sigma * case.sigma
    ref = R.value_ld(F, x, sig2)
    worst = {"fast": 0.0, "lib": 0.0}
    for c0 in range(0, x.shape[1], T.RT):
        xs, g, r = x[:, c0:c0 + T.RT], got[:, c0:c0 + T.RT], ref[:, c0:c0 + T.RT]
        lib = xs.min(axis=1) < -700.0
        for rows, E, key in ((~lib, exp_bar(case), "fast"), (lib, R.E_LIB, "lib")):
            if not rows.any():
                continue
            bar = R.route_bar(E, F, sig2)
            err = np.abs(g[rows].astype(R.LD) - r[rows])
            assert np.all(err <= bar * np.abs(r[rows]) + (R.SUBNORMAL_ATOL if key == "lib" else 0.0)), \
                "%s: %s-exp waves of columns %d..: %.3f u against a bar of %.3f u" % (what, key, c0, R.rel_error_u(g[rows], r[rows]), bar / R.U)
            worst[key] = max(worst[key], R.rel_error_u(g[rows], r[rows]))
            assert np.all(g[rows][xs[rows] <= -746.0] == 0.0)
    return worst


# ------------------------------------------------------------------------------------------ (a) the exp, bit for bit
OUT_OF_DOMAIN = (-700.5, -708.0, -745.0, -746.0, -800.0)


def _exp_columns(parts, with_tile):
    """the directed b of the parts, padded with zeros to whole tiles; with_tile: one more tile of out-of-domain arguments
    (a wave never crosses a tile, so every other tile stays on the fast exp)"""
    D = R.directed()
    b = np.concatenate([D["b_" + p] for p in parts])
    want_tab = np.concatenate([D["tab_" + p] for p in parts])
    want_fast = np.concatenate([D["fast_" + p] for p in parts])
    n = len(b)
    b = np.concatenate([b, np.zeros(T.round_up(n) - n)])
    if with_tile:
        far = [float(np.sqrt(-2.0 * x)) for x in OUT_OF_DOMAIN] + [1e200]          # 1e200^2 overflows: the argument is -inf
        b = np.concatenate([b, np.resize(np.array(far), T.RT)])
    return b, n, want_tab, want_fast


EXP_RUNS = [  # id, d, rows of A, parts of the directed set, out-of-domain tile, emulation
    ("regs_interior_nocheck", 1, 128, ("core",), False, "tab"),
    ("regs_interior_check", 1, 128, ("core", "ext"), True, "tab"),
    ("regs_edge", 1, 1, ("core", "ext"), True, "tab"),
    ("lds", 9, 2, ("core", "ext"), True, "fast"),
    ("naive", 33, 2, ("core", "ext"), True, "fast")]


@pytest.mark.parametrize("sigma", [1.0, 1.3], ids=["unit", "sigma1.3"])
@pytest.mark.parametrize("name,d,rows,parts,with_tile,emu", EXP_RUNS, ids=[r[0] for r in EXP_RUNS])
def test_device_exp_equals_its_emulation_bit_for_bit(kctx, name, d, rows, parts, with_tile, emu, sigma):
    """a = 0, l = 1: the argument of column j is -0.5 fl(b_j^2) in every kernel (zero coordinates add exactly)"""
    b, n, want_tab, want_fast = _exp_columns(parts, with_tile)
    B = np.zeros((len(b), d))
    B[:, 0] = b
    A = np.zeros((rows, d))
    with np.errstate(over="ignore"):
        x = R.arg_of(b)
        box = T.box_max_sq(A, B)
    # what makes the launch take the nocheck form or not (gpmi_kroute.h: rbf_route)
    assert (box >= 0.0 and -0.5 * box * 1.000001 >= -690.0) == (name == "regs_interior_nocheck")
    got = kctx.rbf(A, B, sigma, 1.0)
    sig2 = sigma * sigma
    want = sig2 * (want_tab if emu == "tab" else want_fast)
    for r in range(rows):
        differ = np.flatnonzero(got[r, :n] != want)
        assert len(differ) == 0, "%s row %d: %d of %d arguments differ from the emulation, first x = %r: device %r, emulation %r" % (
            name, r, len(differ), n, float(x[differ[0]]), float(got[r, differ[0]]), float(want[differ[0]]))
    assert np.all(got[:, n:T.round_up(n)] == sig2)                       # the zero padding: exp(-0) == 1
    if with_tile:
        c0 = T.round_up(n)
        case = T.Case("cov", 0, d, rows, len(b), sigma=sigma, ell=1.0)
        worst = hold_values(got[:, c0:], np.broadcast_to(x[c0:], (rows, T.RT)), case, name)
        print("%s sigma %.1f: out-of-domain tile %.3f u of the long-double value" % (name, sigma, worst["lib"]))
        assert worst["fast"] == 0.0                                      # every wave of that tile took the library exp


# --------------------------------------------------------------------- (b) placement invariance, (c) sigma, bit for bit
WINDOWS = [(5, 135, 1, 258), (129, 300, 127, 512), (0, 1, 0, 1), (255, 258, 383, 386), (64, 300, 2, 131)]


@pytest.mark.parametrize("F,d", sorted(T.STATIONARY), ids=["F%d-d%d" % k for k in sorted(T.STATIONARY)])
def test_placement_and_sigma_do_not_change_a_bit(kctx, F, d):
    """windows that move every element across lane, column-pair parity, row group and tile class (interior, edge, the
    odd last column), and K(sigma) == fl(sigma^2 K(1))"""
    case = T.STATIONARY[(F, d)][0].case
    A, B = T.inputs(case)
    assert arguments(case, A, B).min() >= -700.0
    K1 = cov(kctx, case.kind, A, B, 1.0, case.ell)
    Ks = cov(kctx, case.kind, A, B, 1.3, case.ell)
    assert np.array_equal(Ks, (1.3 * 1.3) * K1)
    for i, (r0, r1, c0, c1) in enumerate(WINDOWS):
        K, sigma = (K1, 1.0) if i % 2 else (Ks, 1.3)
        sub = cov(kctx, case.kind, A[r0:r1], B[c0:c1], sigma, case.ell)
        assert np.array_equal(sub, K[r0:r1, c0:c1]), (r0, r1, c0, c1)


# ------------------------------------------------------------------------------------------------ (c) a far row
@pytest.mark.parametrize("c", T.FAR, ids=[c.kernel for c in T.FAR])
def test_a_far_row_switches_the_domain_test_on_and_changes_no_other_bit(kctx, ops, c):
    got, A, B = run(c.case, kctx, ops)
    near = cov(kctx, c.case.kind, A[:-1], B, c.case.sigma, c.case.ell)
    assert np.array_equal(got[:-1], near)
    x = arguments(c.case, A[-1:], B)
    assert x.min() < -700.0 and x.min() > -746.0 and T.max_sq(c.case) > 0
    if c.case.kind != 0:            # the Matern far rows: every wave on the library exp, every result normal
        assert x.max() < -700.0 and x.min() > -708.0
    worst = hold_values(got[-1:], x, c.case, c.kernel)
    print("%s: far row %.3f u (library exp), %.3f u (waves inside the domain)" % (c.kernel, worst["lib"], worst["fast"]))


# ------------------------------------------------------------------------------------------------ (c) rbf_blocks
@pytest.mark.parametrize("c", T.BLOCKS, ids=["%s-%s-blocks%d" % (c.kernel, c.case.api, c.case.blocks) for c in T.BLOCKS])
def test_fewer_blocks_than_work_items_give_the_same_bits(kctx, ops, c):
    got, _, _ = run(c.case, kctx, ops)
    want, _, _ = run(c.case._replace(blocks=None), kctx, ops)
    assert np.array_equal(got, want)
    assert np.any(got != CANARY) and np.all(np.isfinite(got))


# ------------------------------------------------------------------------------------------------ symmetric rows
def hold_rows_layout(got, case, K):
    """got: the nrows x (ncols + 6) buffer of a symmetric-rows launch; K: cov(X, X) of the same parameters.  Tiles
    strictly above the diagonal and the columns past ncols keep the canary; the padding is the identity, exactly; the
    real diagonal is fl(K_ii + s); everything else has the bits of K."""
    N = case.nA
    r = np.arange(case.row0, case.row0 + case.nrows)[:, None]
    c = np.arange(got.shape[1])[None, :]
    dead = (c >= case.ncols) | ((c // T.RT) > (r // T.RT))
    assert np.all(got[np.broadcast_to(dead, got.shape)] == CANARY)
    pad = ~dead & ((r >= N) | (c >= N))
    assert np.array_equal(got[pad], np.broadcast_to(r == c, got.shape)[pad].astype(float))
    real = ~dead & ~pad
    want = np.zeros(got.shape)
    rows = r[:, 0][r[:, 0] < N]
    want[:len(rows), :N] = K[rows]
    want[np.broadcast_to(r == c, got.shape) & real] += T.NOISE
    assert np.array_equal(got[real], want[real])


ROWS = [T.STATIONARY[(F, d)][1] for F, d in [(0, 3), (1, 1), (2, 8), (3, 16), (3, 12), (1, 33)]] + T.SHAPES[:5]


@pytest.mark.parametrize("c", ROWS, ids=["%s-row0_%d" % (c.kernel, c.case.row0) for c in ROWS])
def test_symmetric_rows_have_the_bits_of_the_rectangular_build(kctx, ops, c):
    got, X, _ = run(c.case, kctx, ops)
    K = cov(kctx, c.case.kind, X, X, c.case.sigma, c.case.ell)
    sig2 = c.case.sigma * c.case.sigma
    assert np.all(np.diag(K) == sig2)                    # every factor is exactly 1 at sq == 0
    hold_rows_layout(got, c.case, K)
    i = np.arange(c.case.row0, min(c.case.nA, c.case.row0 + c.case.nrows))
    assert np.all(got[i - c.case.row0, i] == sig2 + T.NOISE)


# --------------------------------------------------------------------- (d) every route against the long-double value
VALUE_CLAIMS = [c for v in T.STATIONARY.values() for c in v] + [c for c in T.SHAPES if T.stationary(c.case.kind)] + T.THRESHOLD


def _id(c):
    k = c.case
    return "%s-%s-d%d-%dx%d-row0_%d-sigma%.1f%s" % (c.kernel.replace(" ", ""), k.api, k.d, k.nrows, k.ncols, k.row0, k.sigma,
                                                     "-nocheck" if c.nocheck else "")


@pytest.mark.parametrize("c", VALUE_CLAIMS, ids=[_id(c) for c in VALUE_CLAIMS])
def test_route_against_the_long_double_value(kctx, ops, c):
    case = c.case
    got, A, B = run(case, kctx, ops)
    if case.api == "cov":
        x = arguments(case, A, B)
    else:
        rows = np.arange(case.row0, min(case.nA, case.row0 + case.nrows))
        x = arguments(case, A[rows], B)
        full = got
        got = full[:len(rows), :case.nB].copy()
        if case.api == "rows":
            # the launch wrote the lower tiles only, and added the noise to the real diagonal
            sig2 = case.sigma * case.sigma
            assert np.all(full[rows - case.row0, rows] == sig2 + T.NOISE)
            got[rows - case.row0, rows] = sig2
            dead = (np.arange(case.nB)[None, :] // T.RT) > (rows[:, None] // T.RT)
            assert np.all(got[dead] == CANARY)
            F = KIND_FAMILY[case.kind]
            got[dead] = R.value_ld(F, x, sig2)[dead].astype(np.float64)      # not part of the comparison
        else:
            assert np.all(full[:, case.ncols:] == CANARY) and np.all(full[len(rows):, :case.ncols] == 0.0)
            assert np.all(full[:, case.nB:case.ncols] == 0.0)
    assert x.min() >= -700.0
    worst = hold_values(got, x, case, _id(c))
    print("%s: %.3f u of the long-double value (bar %.3f u)" % (_id(c), worst["fast"],
                                                                R.route_bar(exp_bar(case), KIND_FAMILY[case.kind], case.sigma ** 2) / R.U))


OTHER_CLAIMS = [c for v in T.OTHER.values() for c in v] + [c for c in T.SHAPES if not T.stationary(c.case.kind)]


@pytest.mark.parametrize("c", OTHER_CLAIMS, ids=["%s-%s-d%d-%s-row0_%d" % (T.KIND_NAME[c.case.kind], c.kernel, c.case.d, c.case.api,
                                                                            c.case.row0) for c in OTHER_CLAIMS])
def test_other_kinds_against_the_numpy_mirror(kctx, ops, c):
    """kinds 1-3 on the LDS tile kernel and on cov_other_kernel, at the suite's COV_RTOL against NumpyBlockOps"""
    import torch
    case = c.case
    got, A, B = run(case, kctx, ops)
    if case.api == "cov":
        ref = NumpyBlockOps._cov(case.kind, T.params(case), A, B)
    else:
        assert np.all(got[:, case.ncols:] == CANARY)
        got = got[:, :case.ncols]
        ref = torch.zeros((case.nrows, case.ncols), dtype=torch.float64)
        NumpyBlockOps().cov_rows(case.kind, T.params(case), torch.from_numpy(A), case.nA, case.d, case.row0, case.nrows, case.ncols,
                                 T.NOISE, ref)
        ref = ref.numpy()
        assert np.all(got[np.isnan(ref)] == CANARY)
        r = np.arange(case.row0, case.row0 + case.nrows)[:, None]
        col = np.arange(case.ncols)[None, :]
        pad = ((r >= case.nA) | (col >= case.nA)) & ~np.isnan(ref)
        assert np.array_equal(got[pad], np.broadcast_to(r == col, got.shape)[pad].astype(float))
    ok = np.isnan(ref) | np.isclose(got, ref, rtol=COV_RTOL, atol=COV_RTOL * np.nanmax(np.abs(ref)))
    assert ok.all(), "%d elements differ, first at %s" % ((~ok).sum(), tuple(np.argwhere(~ok)[0]))


# ------------------------------------------------------------------------------- (e) the 4-tile strip, on the device
@pytest.mark.parametrize("blocks", [None, 64], ids=["default", "blocks64"])
def test_strip_of_four_row_tiles_symmetric(ops, kctx, blocks):
    """the lower triangle of 91 x 91 tiles in one launch (4186 tiles: strip 4) against 1024-row launches (strip 1)"""
    import torch
    N, Np, chunk, d = T.STRIP_SYM_N, T.STRIP_SYM_NP, T.STRIP_SYM_CHUNK, 8
    case = T.STRIP[0].case
    X = _dev(ops, np.random.default_rng(5).uniform(0.0, 4.0, (N, d)))
    one = torch.full((Np, Np), CANARY, dtype=torch.float64, device=ops.device)
    parts = torch.full((Np, Np), CANARY, dtype=torch.float64, device=ops.device)
    with rbf_blocks(kctx, ops, blocks):
        ops.rbf_rows(X, N, d, 0, Np, Np, case.sigma, case.ell, T.NOISE, one)
        for r0 in range(0, Np, chunk):
            rows = min(chunk, Np - r0)
            ops.rbf_rows(X, N, d, r0, rows, Np, case.sigma, case.ell, T.NOISE, parts[r0:r0 + rows])
        ops.sync()
    assert torch.equal(one, parts)
    assert float(one[0, 0]) == case.sigma * case.sigma + T.NOISE and float(one[0, T.RT]) == CANARY and float(one[Np - 1, Np - 1]) == 1.0


def test_strip_of_four_row_tiles_rectangular(ops):
    """18 x 256 tiles in one launch (the last strip holds two row tiles) against 512-row launches"""
    import torch
    n, nrows, ncols_real, ncols, chunk = T.STRIP_RECT
    d = 8
    case = T.STRIP[-3].case
    assert (case.nA, case.nB) == (n, ncols_real)
    rng = np.random.default_rng(6)
    Xs, Xc = _dev(ops, rng.uniform(0.0, 4.0, (n, d))), _dev(ops, rng.uniform(0.0, 4.0, (ncols_real, d)))
    one = torch.full((nrows, ncols), CANARY, dtype=torch.float64, device=ops.device)
    parts = torch.full((nrows, ncols), CANARY, dtype=torch.float64, device=ops.device)
    ops.rbf_cross(Xs, n, Xc, ncols_real, d, nrows, ncols, case.sigma, case.ell, one)
    for r0 in range(0, nrows, chunk):
        rows = min(chunk, nrows - r0)
        ops.rbf_cross(Xs[r0:], min(rows, n - r0), Xc, ncols_real, d, rows, ncols, case.sigma, case.ell, parts[r0:r0 + rows])
    ops.sync()
    assert torch.equal(one, parts)
    assert float(one[n, 0]) == 0.0 and float(one[0, ncols_real]) == 0.0 and 0.0 < float(one[n - 1, ncols_real - 1]) <= case.sigma ** 2
