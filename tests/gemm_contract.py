"""The contract of the update GEMM  C -= A * B^T  (gpmi_dev_gemm_nt, _rowmap, _rowmap_host, _blocks: include/gpmi.h)
as a checker against an independent reference -- TEST INFRASTRUCTURE.

It runs one launch through a block-ops object (dist.HipBlockOps on the GPU, numpy_block_ops.NumpyBlockOps on the
CPU) with every operand a view inside a guard-banded buffer, and holds the result to one of two oracles:

  exact      small dyadic operands (k / 4, |k| <= 8) and C0 on a dyadic grid: every product and every partial sum is
             exact in fp64, whatever the order of summation, so the reference C0 - A B^T is exact too;
  bound      full-mantissa operands with row scales over 2^-20 .. 2^20: |got - ref| <= 2 gamma_{K+1} (|C0| + |A| |B|^T)
             elementwise, ref in fp64 BLAS (both sides are within gamma_{K+1} of the exact value).  Accumulation
             in less than fp64 anywhere misses this by orders of magnitude.

Where the result is required: the live region is {col <= row + diag_off} (lower mode) and {col < reach of the row's
band} (row map).  Inside it the reference must be met; every element of a 128 x 128 tile that does not meet the live
region, and every guard element of C, must hold C0 bit for bit; the rest of a live tile may hold either (a route
computes whole tiles of 64 or of 128).  A and B guards are NaN, so a read outside the operands shows up in C.
"""
import ctypes as C
from dataclasses import dataclass
from typing import Optional, Tuple

import numpy as np
import torch

G = 64              # guard rows and columns on every side; each view starts G columns into its buffer
TILE = 128
U = 2.0 ** -53


@dataclass(frozen=True)
class Case:
    M: int
    N: int
    K: int
    lower: int = 0
    diag_off: int = 0
    # row map: reach of band q = reach[q] columns; bands of rbr rows (the last band may be partial)
    reach: Optional[Tuple[int, ...]] = None
    rbr: int = TILE
    host_map: bool = True           # row map: pass the host copy too (gemm_nt_rowmap_host)
    brows: int = 0                  # > 0: B as a table of row blocks of brows rows (gemm_nt_blocks)

    def __str__(self):
        s = "%dx%dxK%d" % (self.M, self.N, self.K)
        if self.lower:
            s += "-lower%+d" % self.diag_off
        if self.reach is not None:
            s += "-map%d%s" % (self.rbr, "host" if self.host_map else "dev")
        if self.brows:
            s += "-blocks%d" % self.brows
        return s


def dyadic(rng, shape, lim=8):
    return rng.integers(-lim, lim + 1, size=shape) / 4.0


def full_mantissa(rng, shape):
    return rng.standard_normal(shape) * np.exp2(rng.integers(-20, 21, size=(shape[0], 1)))


def live_masks(case):
    """(element-wise live region, elements of 128 x 128 tiles that meet it), both M x N"""
    M, N = case.M, case.N
    r = np.arange(M)[:, None]
    c = np.arange(N)[None, :]
    live = np.ones((M, N), bool)
    tile = np.ones((M, N), bool)
    r0 = r // TILE * TILE                                    # first row / column of the element's tile
    c0 = c // TILE * TILE
    if case.lower:
        live &= c <= r + case.diag_off
        tile &= c0 <= r0 + TILE - 1 + case.diag_off
    if case.reach is not None:
        reach = np.asarray(case.reach)[r // case.rbr]
        live &= c < reach
        tile &= c0 < reach
    return live, tile


class Buffers:
    """C, A, B (or B's block table) as views inside guard-banded buffers on ops.device"""

    def __init__(self, ops, case, C0, A, B, rng):
        M, N, K = case.M, case.N, case.K
        dev = ops.device
        self.case = case
        self.C0full = np.asarray(rng.integers(-64, 65, size=(M + 2 * G, N + 3 * G)) / 16.0)
        self.C0full[G:G + M, G:G + N] = C0
        self.Cbuf = torch.from_numpy(self.C0full.copy()).to(dev)
        self.Cv = self.Cbuf[G:G + M, G:G + N]
        Abuf = np.full((M + 2 * G, K + 3 * G), np.nan)
        Abuf[G:G + M, G:G + K] = A
        self.Abuf = torch.from_numpy(Abuf).to(dev)
        self.Av = self.Abuf[G:G + M, G:G + K]
        if case.brows:
            # the all-gather's receive buffer: the blocks in a scrambled order, NaN gaps between them, each block's
            # rows ldb apart and G columns into its slot
            nblk = -(-N // case.brows)
            self.ldb = K + 2 * G
            slot = case.brows * self.ldb
            perm = rng.permutation(nblk + 2)[:nblk]
            flat = np.full((nblk + 2) * slot + 2 * G, np.nan)
            Bp = np.zeros((nblk * case.brows, K))
            Bp[:N] = B
            for i, q in enumerate(perm):
                blk = flat[q * slot:(q + 1) * slot].reshape(case.brows, self.ldb)
                blk[:, G:G + K] = Bp[i * case.brows:(i + 1) * case.brows]
            self.Bflat = torch.from_numpy(flat).to(dev)
            self.boff = torch.from_numpy((perm * slot + G).astype(np.int64)).to(dev)
        else:
            Bbuf = np.full((N + 2 * G, K + 3 * G), np.nan)
            Bbuf[G:G + N, G:G + K] = B
            self.Bbuf = torch.from_numpy(Bbuf).to(dev)
            self.Bv = self.Bbuf[G:G + N, G:G + K]
        if case.reach is not None:
            self.reach_host = np.ascontiguousarray(case.reach, dtype=np.int32)
            self.reach_dev = torch.from_numpy(self.reach_host.copy()).to(dev)

    def launch(self, ops):
        case = self.case
        if case.brows:
            m = case.reach is not None
            ops.gemm_nt_blocks(self.Cv, self.Av, self.Bflat, self.ldb, self.boff, case.brows,
                               self.reach_dev if m else None, case.rbr, self.reach_host if m else None)
        elif case.reach is not None:
            ops.gemm_nt_rowmap(self.Cv, self.Av, self.Bv, self.reach_dev, case.rbr,
                               self.reach_host if case.host_map else None)
        elif case.lower:
            # HipBlockOps.gemm_nt always passes lower = 0: lower mode through the C-ABI itself
            from gaussian_process_amd._lib import check
            check(ops.lib.gpmi_dev_gemm_nt(ops._stream(), C.c_void_p(self.Cv.data_ptr()), self.Cv.stride(0),
                                           C.c_void_p(self.Av.data_ptr()), self.Av.stride(0),
                                           C.c_void_p(self.Bv.data_ptr()), self.Bv.stride(0),
                                           case.M, case.N, case.K, 1, case.diag_off))
        else:
            ops.gemm_nt(self.Cv, self.Av, self.Bv)
        ops.sync()
        return self.Cbuf.cpu().numpy()


def operands(case, rng, exact):
    gen = dyadic if exact else full_mantissa
    A = gen(rng, (case.M, case.K))
    B = gen(rng, (case.N, case.K))
    C0 = rng.integers(-64, 65, size=(case.M, case.N)) / 16.0 if exact else full_mantissa(rng, (case.M, case.N))
    return C0, A, B


def run(ops, case, seed, exact):
    """one launch -> (whole C buffer after it, C0 buffer, A, B)"""
    rng = np.random.default_rng(seed)
    C0, A, B = operands(case, rng, exact)
    buf = Buffers(ops, case, C0, A, B, rng)
    return buf.launch(ops), buf.C0full, A, B


def _where(mask):
    i = np.argwhere(mask)
    return "%d elements, first at (row, col) %s" % (len(i), tuple(i[0]))


def check_guards(out, C0full, case):
    M, N = case.M, case.N
    g = np.ones(out.shape, bool)
    g[G:G + M, G:G + N] = False
    bad = g & ~(out == C0full)
    assert not bad.any(), "%s: guard of C written: %s" % (case, _where(bad))


def check_exact(ops, case, seed=0):
    out, C0full, A, B = run(ops, case, seed, exact=True)
    check_guards(out, C0full, case)
    M, N = case.M, case.N
    C0 = C0full[G:G + M, G:G + N]
    got = out[G:G + M, G:G + N]
    want = C0 - A @ B.T
    live, tile = live_masks(case)
    bad = live & ~(got == want)
    assert not bad.any(), "%s: live element differs from C0 - A B^T: %s" % (case, _where(bad))
    bad = ~tile & ~(got == C0)
    assert not bad.any(), "%s: element of a dead tile written: %s" % (case, _where(bad))
    bad = ~live & ~((got == C0) | (got == want))
    assert not bad.any(), "%s: element outside the live region neither C0 nor C0 - A B^T: %s" % (case, _where(bad))
    return got


def check_bound(ops, case, seed=1):
    out, C0full, A, B = run(ops, case, seed, exact=False)
    check_guards(out, C0full, case)
    M, N, K = case.M, case.N, case.K
    C0 = C0full[G:G + M, G:G + N]
    got = out[G:G + M, G:G + N]
    ref = C0 - A @ B.T
    gam = (K + 1) * U / (1 - (K + 1) * U)
    tol = 2 * gam * (np.abs(C0) + np.abs(A) @ np.abs(B).T)
    ok = np.abs(got - ref) <= tol
    live, tile = live_masks(case)
    bad = live & ~ok
    assert not bad.any(), "%s: live element off by more than 2 gamma_(K+1) (|C0| + |A||B|^T): %s, worst ratio %g" % (
        case, _where(bad), np.max(np.abs(got - ref)[bad] / tol[bad]))
    bad = ~tile & ~(got == C0)
    assert not bad.any(), "%s: element of a dead tile written: %s" % (case, _where(bad))
    bad = ~live & ~((got == C0) | ok)
    assert not bad.any(), "%s: element outside the live region neither C0 nor within the bound: %s" % (case, _where(bad))
    return got
