"""The device block primitives that dist.HipBlockOps chains (gpmi_dev_*: include/gpmi.h) and that the suite otherwise
reaches only through whole DistGP fits, each against a plain high-precision reference at its documented edges:
trsv_lt, trsv_lt_vinv, logdiag_sumsq, row_dots, grad_trace, rbf_rows / rbf_cross, cov_rows / cov_cross."""
import math

import numpy as np
import pytest

from numpy_block_ops import NumpyBlockOps

pytestmark = pytest.mark.gpu

U = 2.0 ** -53
LD = np.longdouble
K_RTOL = 7e-16          # as test_parity_gpu.py: identical exp argument, exp itself < 1 ulp on both sides
COV_RTOL = 2e-14        # kinds 1-3: sin, pow and several exps per element, each within ~1 ulp of NumPy's (CO2_K_RTOL)


@pytest.fixture(scope="module")
def ops():
    from gaussian_process_amd.dist import HipBlockOps
    return HipBlockOps(0)


def _dev(ops, a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).to(ops.device)


def _spd(n, cond, seed):
    rng = np.random.default_rng(seed)
    Q, _ = np.linalg.qr(rng.standard_normal((n, n)))
    ev = np.logspace(0, -math.log10(cond), n)
    A = (Q * ev) @ Q.T
    return (A + A.T) / 2


def _factor(ops, n, cond, seed, ld):
    """L as gpmi_dev_potrf_block leaves it, in an (n x ld) buffer"""
    import torch
    A = np.zeros((n, ld))
    A[:, :n] = _spd(n, cond, seed)
    Ad = _dev(ops, A)
    info = torch.full((1,), (1 << 63) - 1, dtype=torch.int64, device=ops.device)
    ops.potrf_block(Ad[:, :n], 0, info)
    ops.sync()
    assert int(info.item()) == (1 << 63) - 1
    return Ad


# ---------------------------------------------------------------- backward substitution  L^T x = b

def _residual(L, x, b):
    """b - L^T x and |L^T| |x|, in long double"""
    Ll, xl = np.tril(L).astype(LD), x.astype(LD)
    return b.astype(LD) - Ll.T @ xl, np.abs(Ll.T) @ np.abs(xl)


@pytest.mark.parametrize("cond", [1e2, 1e10])
@pytest.mark.parametrize("n", [448, 512])
def test_trsv_lt_componentwise_backward_error(ops, n, cond):
    """gpmi_dev_trsv_lt (n % 64): |b - L^T x| <= 2 n u |L^T| |x| componentwise (a backward-stable substitution); the
    strict upper triangle is NaN, so a read of it would show"""
    ld = 512 + 6
    Ad = _factor(ops, 512, cond, n, ld)
    Ld = Ad[:n, :n]
    L = np.tril(Ld.cpu().numpy())
    iu = np.triu_indices(n, 1)
    Lnan = Ld.cpu().numpy().copy()
    Lnan[iu] = np.nan
    Ld.copy_(_dev(ops, Lnan))
    b = np.random.default_rng(n).standard_normal(n)
    bd = _dev(ops, b)
    # through the C-ABI: HipBlockOps.trsv_lt takes the vinv form when n % 128 == 0
    from gaussian_process_amd._lib import check
    check(ops.lib.gpmi_dev_trsv_lt(ops._stream(), ops._p(Ld), Ld.stride(0), ops._p(bd), n))
    ops.sync()
    x = bd.cpu().numpy()
    assert np.all(np.isfinite(x))
    r, s = _residual(L, x, b)
    assert np.all(np.abs(r) <= 2 * n * U * s), "worst ratio %g" % np.max(np.abs(r) / (n * U * s))


@pytest.mark.parametrize("cond", [1e2, 1e10])
def test_trsv_lt_vinv_normwise_backward_error(ops, cond):
    """gpmi_dev_trsv_lt_vinv: invert=1 writes the inverses of the 128 x 128 diagonal blocks, invert=0 reuses them for a
    second right-hand side.  x_k = V_kk^T (b_k - s_k) with V_kk the computed inverse, so the residual grows with
    cond(L_kk):  ||b - L^T x||_inf <= 4 (n + 128 cond_inf(L_kk)) u || |L^T| |x| ||_inf.  Outside the diagonal blocks
    the upper triangle is NaN."""
    import torch
    n, ld = 512, 512 + 10
    Ad = _factor(ops, n, cond, 7, ld)
    Ld = Ad[:, :n]
    F = Ld.cpu().numpy().copy()
    L = np.tril(F)
    keep = np.zeros((n, n), bool)
    for k in range(0, n, 128):
        keep[k:k + 128, k:k + 128] = True
    F[np.triu(~keep, 1)] = np.nan
    Ld.copy_(_dev(ops, F))
    kappa = max(np.linalg.norm(L[k:k + 128, k:k + 128], np.inf) * np.linalg.norm(np.linalg.inv(L[k:k + 128, k:k + 128]), np.inf)
                for k in range(0, n, 128))
    rng = np.random.default_rng(11)
    for invert in (1, 0):
        b = rng.standard_normal(n)
        bd = _dev(ops, b)
        xd = torch.empty_like(bd)
        from gaussian_process_amd._lib import check
        check(ops.lib.gpmi_dev_trsv_lt_vinv(ops._stream(), ops._p(Ld), Ld.stride(0), ops._p(bd), ops._p(xd), n, invert))
        ops.sync()
        x = xd.cpu().numpy()
        assert np.all(np.isfinite(x))
        r, s = _residual(L, x, b)
        tol = 4 * (n + 128 * kappa) * U * np.max(s)
        assert np.max(np.abs(r)) <= tol, "invert=%d: %g > %g" % (invert, np.max(np.abs(r)), tol)
        # the lower triangle (the factor) is untouched
        assert np.array_equal(np.tril(Ld.cpu().numpy()), L)


# ---------------------------------------------------------------- LML pieces: sum log L_ii, x^T x

@pytest.mark.parametrize("what", ["A", "x", "both", "ones"])
@pytest.mark.parametrize("n", [1, 63, 1024, 1025, 4097])
def test_logdiag_sumsq(ops, n, what):
    import torch
    rng = np.random.default_rng(n)
    ld = n + 3
    A = rng.standard_normal((n, ld))
    A[np.arange(n), np.arange(n)] = 1.0 if what == "ones" else np.exp(rng.uniform(-30, 30, n))
    x = rng.standard_normal(n) * np.exp2(rng.integers(-20, 21, n))
    Ad, xd = _dev(ops, A), _dev(ops, x)
    out = torch.full((2,), np.nan, dtype=torch.float64, device=ops.device)
    useA, usex = what in ("A", "both", "ones"), what in ("x", "both", "ones")
    ops.logdiag_sumsq(Ad[:, :n] if useA else None, n, xd if usex else None, n, out)
    ops.sync()
    got = out.cpu().numpy()
    logs = [math.log(v) for v in np.diagonal(A)[:n]]
    if not useA:
        assert got[0] == 0.0
    elif what == "ones":
        assert got[0] == 0.0                         # log 1 == 0 exactly, whatever the order
    else:
        assert abs(got[0] - math.fsum(logs)) <= (n + 2) * U * math.fsum(abs(v) for v in logs)
    if not usex:
        assert got[1] == 0.0
    else:
        ref = math.fsum(float(v) * float(v) for v in x)
        assert abs(got[1] - ref) <= (n + 1) * U * ref


# ---------------------------------------------------------------- row_dots: V m and the row sums of squares

@pytest.mark.parametrize("pad", [0, 6])
@pytest.mark.parametrize("ncols", [0, 2, 130, 4098])
@pytest.mark.parametrize("nrows", [1, 129, 1000])
def test_row_dots(ops, nrows, ncols, pad):
    import torch
    ld = ncols + pad
    rng = np.random.default_rng(nrows * 7 + ncols + pad)
    for exact in (True, False):
        if exact:
            V = rng.integers(-8, 9, size=(nrows, max(ld, 2))) / 4.0
            m = rng.integers(-8, 9, size=max(ncols, 2)) / 4.0
        else:
            V = rng.standard_normal((nrows, max(ld, 2))) * np.exp2(rng.integers(-20, 21, (nrows, 1)))
            m = rng.standard_normal(max(ncols, 2))
        V[:, ncols:] = np.nan                             # columns past ncols are never read
        Vd, md = _dev(ops, V), _dev(ops, m)
        Vv = Vd[:, :ld] if ld else Vd[:, :2]
        dots = {}
        for want in ("dot", "sq"):
            dot = torch.full((nrows,), np.nan, dtype=torch.float64, device=ops.device)
            sq = torch.full((nrows,), np.nan, dtype=torch.float64, device=ops.device)
            from gaussian_process_amd._lib import check
            check(ops.lib.gpmi_dev_row_dots(ops._stream(), ops._p(Vv), Vv.stride(0), nrows, ncols, ops._p(md),
                                            ops._p(dot) if want == "dot" else None, ops._p(sq) if want == "sq" else None))
            ops.sync()
            # the other output is not written
            assert np.all(np.isnan((sq if want == "dot" else dot).cpu().numpy()))
            dots[want] = (dot if want == "dot" else sq).cpu().numpy()
        Vr = V[:, :ncols]
        ref_dot = (Vr.astype(LD) @ m[:ncols].astype(LD)).astype(np.float64)
        ref_sq = (Vr.astype(LD) ** 2).sum(1).astype(np.float64)
        if exact:
            assert np.array_equal(dots["dot"], ref_dot) and np.array_equal(dots["sq"], ref_sq)
        else:
            g = (ncols + 1) * U
            assert np.all(np.abs(dots["dot"] - ref_dot) <= g * (np.abs(Vr) @ np.abs(m[:ncols])))
            assert np.all(np.abs(dots["sq"] - ref_sq) <= g * ref_sq)


# ---------------------------------------------------------------- grad_trace: one row chunk of the gradient trace

def _grad_ref(X, row0, nrows, alpha_r, alpha_c, Kinv, kinv_sign, sigma, ell):
    """tune_hyperparms_regression.py:43-57 (gp_oracle.lml_gradient_terms' arithmetic), in long double:
    (sum W dK/dl, sum W dK/dsigma) and the sums of the terms' magnitudes"""
    Xl = X.astype(LD)
    N = X.shape[0]
    sq = ((Xl[row0:row0 + nrows, :, None] - Xl[:, :, None].T) ** 2).sum(1)
    e = np.exp(-LD(.5) * sq / LD(ell) ** 2)
    Dl = LD(sigma) ** 2 * e * (sq / LD(ell) ** 3)
    Ds = 2 * LD(sigma) * e
    W = np.outer(alpha_r.astype(LD)[row0:row0 + nrows], alpha_c.astype(LD)[:N]) - LD(kinv_sign) * Kinv[:nrows, :N].astype(LD)
    return (float((W * Dl).sum()), float((W * Ds).sum()), float(np.abs(W * Dl).sum()), float(np.abs(W * Ds).sum()))


def _grad_dev(ops, X, N, d, row0, nrows, ar, ac, Kd, sign, sigma, ell, out):
    import torch
    part = torch.empty(2 * -(-nrows // 128) * -(-N // 128), dtype=torch.float64, device=ops.device)
    ops.grad_trace(X, N, d, row0, nrows, ar, ac, Kd, sign, sigma, ell, part, out)


GRAD = [(row0, nrows, N) for N in (130, 1000) for row0 in (0, 128, 300) for nrows in (1, 128, 200) if row0 + nrows <= N]


@pytest.mark.parametrize("sign", [1.0, -1.0])
@pytest.mark.parametrize("d", [1, 3, 8])
@pytest.mark.parametrize("row0,nrows,N", GRAD)
def test_grad_trace(ops, row0, nrows, N, d, sign):
    rng = np.random.default_rng(N + 10 * d + row0 + nrows)
    sigma, ell = 1.3, 0.7 * math.sqrt(d)
    X = rng.standard_normal((N, d))
    ar, ac = rng.standard_normal(N), rng.standard_normal(N)
    ld = N + 10
    Kinv = rng.standard_normal((nrows, ld))
    Kinv[:, N:] = np.nan                                   # past N: never read
    seed = np.array([0.375, -2.5])
    out = _dev(ops, seed.copy())
    Xd, ard, acd, Kd = _dev(ops, X), _dev(ops, ar), _dev(ops, ac), _dev(ops, Kinv)
    _grad_dev(ops, Xd, N, d, row0, nrows, ard, acd, Kd, sign, sigma, ell, out)
    ops.sync()
    got = out.cpu().numpy() - seed                         # out2 is accumulated onto
    gl, gs, al, as_ = _grad_ref(X, row0, nrows, ar, ac, Kinv, sign, sigma, ell)
    n = nrows * N
    tol_l = (n + 16) * U * al + 4 * U * (abs(seed[0]) + abs(gl))
    tol_s = (n + 16) * U * as_ + 4 * U * (abs(seed[1]) + abs(gs))
    assert abs(got[0] - gl) <= tol_l, (got[0], gl, tol_l)
    assert abs(got[1] - gs) <= tol_s, (got[1], gs, tol_s)


def test_grad_trace_row_chunks_add_up(ops):
    """the multi-rank driver calls it once per row block and adds the chunks: a partition of the rows sums to the
    whole within rounding"""
    import torch
    rng = np.random.default_rng(3)
    N, d, sigma, ell = 1000, 3, 0.9, 1.1
    X = rng.standard_normal((N, d))
    ar, ac = rng.standard_normal(N), rng.standard_normal(N)
    Kfull = rng.standard_normal((N, N))
    Xd, ard, acd = _dev(ops, X), _dev(ops, ar), _dev(ops, ac)
    whole = torch.zeros(2, dtype=torch.float64, device=ops.device)
    _grad_dev(ops, Xd, N, d, 0, N, ard, acd, _dev(ops, Kfull), 1.0, sigma, ell, whole)
    chunks = torch.zeros(2, dtype=torch.float64, device=ops.device)
    for r0, r1 in ((0, 128), (128, 300), (300, 301), (301, 1000)):
        _grad_dev(ops, Xd, N, d, r0, r1 - r0, ard, acd, _dev(ops, Kfull[r0:r1]), 1.0, sigma, ell, chunks)
    ops.sync()
    _, _, al, as_ = _grad_ref(X, 0, N, ar, ac, Kfull, 1.0, sigma, ell)
    w, c = whole.cpu().numpy(), chunks.cpu().numpy()
    assert abs(w[0] - c[0]) <= 2 * (N * N + 16) * U * al
    assert abs(w[1] - c[1]) <= 2 * (N * N + 16) * U * as_


# ---------------------------------------------------------------- covariance rows and cross blocks

CO2 = [1.1, 0.9, 0.6, 1.7, 1.3, 0.4, 0.8, 1.5, 0.3, 0.2, 0.05]
PARAMS = {0: [1.3, 0.8], 1: [0.25], 2: [1.7, 0.9], 3: CO2}


def _allclose(got, ref, rtol, what):
    ok = np.isnan(ref) | np.isclose(got, ref, rtol=rtol, atol=2e-323 if rtol == K_RTOL else rtol * np.nanmax(np.abs(ref)))
    assert ok.all(), "%s: %d elements differ, first at %s" % (what, (~ok).sum(), tuple(np.argwhere(~ok)[0]))


@pytest.mark.parametrize("kind", [None, 0, 1, 2, 3])
@pytest.mark.parametrize("N,row0,nrows,ncols", [(300, 0, 384, 384), (300, 128, 256, 384), (1000, 768, 256, 1024),
                                                (200, 128, 128, 512)])
def test_rows(ops, kind, N, row0, nrows, ncols):
    """rbf_rows (kind None) and cov_rows: rows row0 .. of K(X, X) + s I in the tiles that meet the lower triangle,
    noise on the real diagonal only, identity padding; the columns past ncols of the output are not written"""
    import torch
    d = 1 if kind == 2 else 3
    rng = np.random.default_rng(N + row0 + (kind or 0))
    X = rng.uniform(-2, 2, (N, d))
    s = 0.0625
    ld = ncols + 6
    Xd = _dev(ops, X)
    out = torch.full((nrows, ld), -7.0, dtype=torch.float64, device=ops.device)
    ref = torch.full((nrows, ncols), 0.0, dtype=torch.float64)
    npo = NumpyBlockOps()
    if kind is None:
        ops.rbf_rows(Xd, N, d, row0, nrows, ncols, 1.3, 0.8, s, out[:, :ncols])
        npo.rbf_rows(torch.from_numpy(X), N, d, row0, nrows, ncols, 1.3, 0.8, s, ref)
    else:
        ops.cov_rows(kind, PARAMS[kind], Xd, N, d, row0, nrows, ncols, s, out[:, :ncols])
        npo.cov_rows(kind, PARAMS[kind], torch.from_numpy(X), N, d, row0, nrows, ncols, s, ref)
    ops.sync()
    got = out.cpu().numpy()
    assert np.all(got[:, ncols:] == -7.0)
    got, ref = got[:, :ncols], ref.numpy()
    _allclose(got, ref, K_RTOL if kind in (None, 0) else COV_RTOL, "kind %s" % kind)
    # padding: rows >= N and columns >= N are the identity, exactly
    r = np.arange(row0, row0 + nrows)[:, None]
    c = np.arange(ncols)[None, :]
    pad = ((r >= N) | (c >= N)) & ~np.isnan(ref)
    assert np.array_equal(got[pad], np.broadcast_to(r == c, got.shape)[pad].astype(float))
    # the noise sits on the real diagonal only: the reference adds it there, and s is far outside the tolerance
    assert s > 1e3 * COV_RTOL * np.nanmax(np.abs(ref))


# rbf_cross (kind None) has no window and no delta term: col0 = 0, not square
CROSS = [(kind, square, *shape) for kind in (None, 0, 1, 2, 3) for square in (False, True)
         for shape in ((200, 256, 300, 0, 384), (300, 384, 170, 128, 256), (90, 128, 513, 40, 640))
         if kind is not None or (not square and shape[3] == 0)]


@pytest.mark.parametrize("kind,square,n,nrows,ncols_real,col0,ncols", CROSS)
def test_cross(ops, kind, square, n, nrows, ncols_real, col0, ncols):
    """rbf_cross / cov_cross: out[i][j] = k(Xs[i], Xcols[j]), zero in rows >= n and columns >= ncols_real; for kind 3 on a
    square matrix the delta term on row == col0 + col"""
    import torch
    d = 1 if kind == 2 else 2
    rng = np.random.default_rng(n + ncols_real + col0 + (kind or 0))
    Xs = rng.uniform(-2, 2, (n, d))
    Xc = rng.uniform(-2, 2, (ncols_real, d))
    ld = ncols + 4
    out = torch.full((nrows, ld), -7.0, dtype=torch.float64, device=ops.device)
    ref = torch.zeros((nrows, ncols), dtype=torch.float64)
    npo = NumpyBlockOps()
    Xsd, Xcd = _dev(ops, Xs), _dev(ops, Xc)
    if kind is None:
        ops.rbf_cross(Xsd, n, Xcd, ncols_real, d, nrows, ncols, 1.3, 0.8, out[:, :ncols])
        npo.rbf_cross(torch.from_numpy(Xs), n, torch.from_numpy(Xc), ncols_real, d, nrows, ncols, 1.3, 0.8, ref)
    else:
        ops.cov_cross(kind, PARAMS[kind], Xsd, n, Xcd, ncols_real, d, col0, square, nrows, ncols, out[:, :ncols])
        npo.cov_cross(kind, PARAMS[kind], torch.from_numpy(Xs), n, torch.from_numpy(Xc), ncols_real, d, col0, square,
                      nrows, ncols, ref)
    ops.sync()
    got = out.cpu().numpy()
    assert np.all(got[:, ncols:] == -7.0)
    got, ref = got[:, :ncols], ref.numpy()
    _allclose(got, ref, K_RTOL if kind in (None, 0) else COV_RTOL, "kind %s" % kind)
    assert np.all(got[n:] == 0.0) and np.all(got[:, ncols_real:] == 0.0)
    if kind == 3:
        # with the delta term removed from the reference the elements on row == col0 + col differ by theta_11^2
        i = np.arange(min(n, nrows))
        j = i - col0
        on = (j >= 0) & (j < min(ncols_real, ncols))
        bump = got[i[on], j[on]] - NumpyBlockOps._cov(3, CO2, Xs[i[on]], Xc[j[on]])[np.arange(on.sum()), np.arange(on.sum())]
        want = CO2[10] ** 2 if square else 0.0
        assert np.allclose(bump, want, rtol=0, atol=1e-13)
