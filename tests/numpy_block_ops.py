"""NumPy stand-ins for the gpmi_dev_* block primitives -- TEST INFRASTRUCTURE.

Lets the CPU tests (gloo, world_size 2) run gaussian_process_amd.dist.DistGP's
schedule (ownership, collectives, message shapes, row maps) without a GPU.  Each
method mirrors the contract of the C-ABI primitive of the same name (include/gpmi.h)
using the oracle's arithmetic.
"""
import numpy as np
import scipy.linalg as sla
import torch

import gp_oracle as O


class NumpyBlockOps:
    def __init__(self):
        self.device = torch.device("cpu")

    @staticmethod
    def _a(t):
        return t.numpy()          # shares memory with the (possibly strided) CPU tensor

    def rbf_rows(self, X, N, d, row0, nrows, ncols, sigma, ell, noise_var, out):
        Xn = self._a(X)
        o = self._a(out)
        rows = np.arange(row0, row0 + nrows)
        blk = np.zeros((nrows, ncols))
        rr = rows[rows < N]
        cc = min(N, ncols)
        if len(rr) and cc > 0:
            blk[:len(rr), :cc] = O.RBF_kernel(Xn[rr], Xn[:cc], sigma, ell)
        for i, r in enumerate(rows):          # + s on the diagonal, identity padding
            if r < ncols:
                blk[i, r] = blk[i, r] + noise_var if r < N else 1.0
        # only the tiles that intersect the lower triangle are defined by the HIP kernel;
        # poison the rest so the driver cannot rely on it
        for i in range(0, nrows, 128):
            first_dead = (row0 + i) // 128 * 128 + 128
            if first_dead < ncols:
                blk[i:i + 128, first_dead:] = np.nan
        o[:nrows, :ncols] = blk

    def rbf_cross(self, Xs, n, Xcols, ncols_real, d, nrows, ncols, sigma, ell, out):
        o = self._a(out)
        blk = np.zeros((nrows, ncols))
        cc = max(min(ncols_real, ncols), 0)
        if cc > 0:
            blk[:n, :cc] = O.RBF_kernel(self._a(Xs)[:n], self._a(Xcols)[:cc], sigma, ell)
        o[:nrows, :ncols] = blk

    @staticmethod
    def _cov(kind, params, a, b, square_delta_col0=None):
        """the oracle's covariance functions; kind 3's delta term (CO2_example.py:58-62) on row == col + col0 when asked"""
        if kind == 0:
            return O.RBF_kernel(a, b, params[0], params[1])
        if kind == 1:
            return O.lin_kernel(a, b, params[0])
        if kind == 2:
            return O.per_kernel(a, b, (params[0], params[1]))
        sq = ((a[:, None, :] - b[None, :, :]) ** 2).sum(axis=2) if a.shape[1] > 1 else ((a[:, :, None] - b[:, :, None].T) ** 2).sum(1)
        t = params
        r = np.sqrt(sq)
        k1 = (t[0] ** 2) * np.exp(-.5 * sq / t[1] ** 2)
        k2 = t[2] ** 2 * np.exp(-.5 * sq / t[3] ** 2 + (-2 * ((np.sin(np.pi * r)) / t[4]) ** 2))
        k3 = t[5] ** 2 * (1.0 / np.power(1 + .5 * sq / (t[7] * t[6] ** 2), t[7]))
        delta = np.zeros_like(sq)
        if square_delta_col0 is not None:
            for i in range(sq.shape[0]):
                j = i - square_delta_col0
                if 0 <= j < sq.shape[1]:
                    delta[i, j] = 1.0
        k4 = t[8] ** 2 * np.exp(-.5 * sq / t[9] ** 2) + t[10] ** 2 * delta
        return k1 + k2 + k3 + k4

    def cov_rows(self, kind, params, X, N, d, row0, nrows, ncols, noise_var, out):
        Xn = self._a(X)
        o = self._a(out)
        rows = np.arange(row0, row0 + nrows)
        blk = np.zeros((nrows, ncols))
        rr = rows[rows < N]
        cc = min(N, ncols)
        if len(rr) and cc > 0:
            # the symmetric build is square: kernel_4's delta sits on global row == global column
            blk[:len(rr), :cc] = self._cov(kind, params, Xn[rr], Xn[:cc], square_delta_col0=-int(row0) if kind == 3 else None)
        for i, r in enumerate(rows):
            if r < ncols:
                blk[i, r] = blk[i, r] + noise_var if r < N else 1.0
        for i in range(0, nrows, 128):
            first_dead = (row0 + i) // 128 * 128 + 128
            if first_dead < ncols:
                blk[i:i + 128, first_dead:] = np.nan
        o[:nrows, :ncols] = blk

    def cov_cross(self, kind, params, Xs, n, Xcols, ncols_real, d, col0, square, nrows, ncols, out):
        o = self._a(out)
        blk = np.zeros((nrows, ncols))
        cc = max(min(ncols_real, ncols), 0)
        if cc > 0:
            blk[:n, :cc] = self._cov(kind, params, self._a(Xs)[:n], self._a(Xcols)[:cc],
                                     square_delta_col0=int(col0) if (kind == 3 and square) else None)
        o[:nrows, :ncols] = blk

    def potrf_block(self, A, col_offset, info):
        a = self._a(A)
        low = np.tril(a)
        full = low + np.tril(low, -1).T
        try:
            L = np.linalg.cholesky(full)
        except np.linalg.LinAlgError:
            # first non-PD leading minor, as the HIP kernel reports it
            k = next(i for i in range(1, len(full) + 1) if np.linalg.eigvalsh(full[:i, :i]).min() <= 0)
            info[0] = min(int(info[0]), col_offset + k - 1)
            L = np.full_like(full, np.nan)
        iu = np.triu_indices(len(a), 1)
        keep = a[iu].copy()
        a[:] = L
        a[iu] = keep                 # the upper triangle is left untouched

    def trsm_block(self, L, X):
        x = self._a(X)
        x[:] = sla.solve_triangular(np.tril(self._a(L)), x.T, lower=True, check_finite=False).T   # NaN after a failed pivot must flow through

    def gemm_nt(self, Cm, A, B):
        c = self._a(Cm)
        c -= self._a(A) @ self._a(B).T

    def gemm_nt_rowmap(self, Cm, A, B, row_ncols, row_block_rows, row_ncols_host=None):
        c, a, b = self._a(Cm), self._a(A), self._a(B)
        nc = row_ncols.numpy()
        for q in range(-(-c.shape[0] // row_block_rows)):          # the last band may be partial
            rs = slice(q * row_block_rows, (q + 1) * row_block_rows)
            w = int(nc[q])
            w_t = min((w + 127) // 128 * 128, c.shape[1])     # the kernel works on whole 128-col tiles
            c[rs, :w_t] -= a[rs] @ b[:w_t].T

    def gemm_nt_blocks(self, Cm, A, Bflat, ldb, boff, brows, row_ncols=None, row_block_rows=128, row_ncols_host=None):
        c, a = self._a(Cm), self._a(A)
        flat, K = self._a(Bflat), a.shape[1]
        nblk = -(-c.shape[1] // brows)              # the last block may reach past N
        b = np.vstack([flat[int(o):int(o) + brows * ldb].reshape(brows, ldb)[:, :K] for o in boff.numpy()[:nblk]])
        b = b[:c.shape[1]]
        if row_ncols is None:
            c -= a @ b.T
            return
        nc = row_ncols.numpy()
        for q in range(-(-c.shape[0] // row_block_rows)):
            rs = slice(q * row_block_rows, (q + 1) * row_block_rows)
            w_t = min((int(nc[q]) + 127) // 128 * 128, c.shape[1])
            c[rs, :w_t] -= a[rs] @ b[:w_t].T

    def grad_trace(self, X, N, d, row0, nrows, alpha_r, alpha_c, Kinv, kinv_sign, sigma, ell, partial, out2):
        Xn = self._a(X)[:N]
        rows = slice(row0, row0 + nrows)
        sq = ((Xn[rows][:, :, None] - Xn[:, :, None].T) ** 2).sum(1)                 # tune_hyperparms_regression.py:43
        e = np.exp(-.5 * sq / ell ** 2)
        Dl, Ds = sigma ** 2 * e * (sq / ell ** 3), 2 * sigma * e                     # :54, :48
        W = np.outer(self._a(alpha_r)[rows], self._a(alpha_c)[:N]) - kinv_sign * self._a(Kinv)[:nrows, :N]
        o = self._a(out2)
        o[0] += float(np.sum(W * Dl))
        o[1] += float(np.sum(W * Ds))

    def logdiag_sumsq(self, A, n, x, nx, out2):
        o = self._a(out2)
        o[0] = np.log(np.diagonal(self._a(A))[:n]).sum() if A is not None else 0.0
        o[1] = float(np.dot(self._a(x)[:nx], self._a(x)[:nx])) if x is not None else 0.0

    def row_dots(self, V, ncols, m, dot, sq):
        v = self._a(V)[:, :ncols]
        self._a(dot)[:] = v @ self._a(m)[:ncols]
        self._a(sq)[:] = (v * v).sum(1)

    def gemv_t(self, A, x, y, scratch):
        self._a(y)[:] = self._a(A).T @ self._a(x) if A is not None else 0.0

    def trsv_lt(self, L, b, inverted=False):
        bb = self._a(b)
        bb[:] = sla.solve_triangular(np.tril(self._a(L)), bb, lower=True, trans='T', check_finite=False)

    def sum_fixed(self, inp, count, stride, n, out, base=None, scale=1.0):
        flat = self._a(inp).reshape(-1)
        acc = np.zeros(n)
        for q in range(int(count)):                 # index order, as the kernel adds them
            acc = acc + flat[q * stride:q * stride + n]
        self._a(out)[:n] = (self._a(base)[:n] + scale * acc) if base is not None else scale * acc

    def axpy2d(self, Y, X, a):
        y = self._a(Y)
        y += a * self._a(X)

    def sync(self):
        pass
