"""The 256 x 128 form of the LDS-DMA GEMM (option gemm_tall) against the 128 x 128 form, bit for bit: same MFMAs per
accumulator in the same order, and exactly the same bytes of C written -- the whole buffer is compared, guard rows and
columns around the block included."""
import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.gpu


def _ops():
    from gaussian_process_amd.dist import HipBlockOps
    return HipBlockOps(0)


def _run(ops, form, launch, C0):
    """launch(Cview) under gemm_tall = form (per-tile launches: the resident forms off), -> the whole C buffer"""
    import torch
    ops.set_option("gemm_persist", 0)
    ops.set_option("gemm_tall", form)
    ops.set_option("tall_min_tiles", 0)
    try:
        Cd = torch.from_numpy(C0).to(ops.device)
        launch(Cd)
        torch.cuda.synchronize()
        return Cd.cpu().numpy()
    finally:
        ops.set_option("gemm_tall", 1)
        ops.set_option("tall_min_tiles", 12288)
        ops.set_option("gemm_persist", 1)


def _both(ops, launch, C0):
    tall = _run(ops, 1, launch, C0)
    ref = _run(ops, 0, launch, C0)
    assert np.all(np.isfinite(ref))
    assert np.array_equal(tall, ref), "max |diff| %g" % np.max(np.abs(tall - ref))
    return ref


def _operands(rng, M, N, K, G=128):
    """A (M x K), B (N x K), and C as a view at (G, G) of a buffer with G guard rows / columns on every side"""
    A = rng.standard_normal((M, K))
    B = rng.standard_normal((N, K))
    C0 = rng.standard_normal((M + 2 * G, N + 2 * G + 32))
    return A, B, C0


def _gemm(ops, A, B, M, N, K, lower, diag_off, G=128):
    import torch
    Ad, Bd = torch.from_numpy(A).to(ops.device), torch.from_numpy(B).to(ops.device)

    def launch(Cd):
        v = Cd[G:G + M, G:G + N]
        rc = ops.lib.gpmi_dev_gemm_nt(ops._stream(), C.c_void_p(v.data_ptr()), Cd.stride(0), ops._p(Ad), K,
                                      ops._p(Bd), K, M, N, K, lower, diag_off)
        assert rc == 0
    return launch


@pytest.mark.parametrize("T,K,diag_off", [(33, 32, 0), (33, 48, 0), (32, 512, 0), (37, 2048, 0),
                                          (35, 512, 256), (34, 512, -384), (31, 512, 1024)])
def test_tall_lower_bitwise(T, K, diag_off):
    """lower launches (odd and even tile counts, diagonal offsets): the tiles above the diagonal stay untouched"""
    ops = _ops()
    rng = np.random.default_rng(T * 1000 + K)
    M = N = 128 * T
    A, B, C0 = _operands(rng, M, N, K)
    ref = _both(ops, _gemm(ops, A, B, M, N, K, 1, diag_off), C0)
    # a tile entirely above {col <= row + diag_off} is untouched
    G = 128
    assert np.array_equal(ref[G:G + 128, G + N - 128:G + N], C0[G:G + 128, G + N - 128:G + N]) or diag_off >= N - 128


@pytest.mark.parametrize("Tm,Tn,K", [(23, 17, 512), (17, 31, 32), (40, 24, 2048)])
def test_tall_rectangle_bitwise(Tm, Tn, K):
    ops = _ops()
    rng = np.random.default_rng(Tm * Tn + K)
    M, N = 128 * Tm, 128 * Tn
    A, B, C0 = _operands(rng, M, N, K)
    ref = _both(ops, _gemm(ops, A, B, M, N, K, 0, 0), C0)
    G = 128
    want = C0[G:G + M, G:G + N] - A @ B.T
    assert np.allclose(ref[G:G + M, G:G + N], want, rtol=0, atol=1e-10 * np.abs(want).max())
    assert np.array_equal(ref[:G], C0[:G]) and np.array_equal(ref[G + M:], C0[G + M:])


@pytest.mark.parametrize("K", [48, 512])
def test_tall_rows_below_the_square_bitwise(K):
    """lower launch whose rows run on below the square (the test rows and the y row of the one-pass form ride there)"""
    ops = _ops()
    rng = np.random.default_rng(K + 7)
    M, N = 128 * 45, 128 * 28
    A, B, C0 = _operands(rng, M, N, K)
    _both(ops, _gemm(ops, A, B, M, N, K, 1, 0), C0)


@pytest.mark.parametrize("rbt", [1, 2, 3])
def test_tall_row_map_bitwise(rbt):
    """staircase (row map with its host copy, and without it); bands of an odd number of tiles split pairs"""
    import torch
    ops = _ops()
    rng = np.random.default_rng(rbt)
    M, N, K = 128 * 33, 128 * 40, 512
    bands = -(-(M // 128) // rbt)
    reach = np.minimum(N, 300 + 128 * 2 * rbt * np.arange(bands)).astype(np.int32)
    reach[-1] = N
    A, B, C0 = _operands(rng, M, N, K, G=0)
    Ad, Bd = torch.from_numpy(A).to(ops.device), torch.from_numpy(B).to(ops.device)
    rm = torch.from_numpy(reach).to(ops.device)
    for host in (reach, None):
        def launch(Cd, host=host):
            ops.gemm_nt_rowmap(Cd[:, :N], Ad, Bd, rm, 128 * rbt, host)
        _both(ops, launch, C0)


def test_tall_block_table_bitwise():
    """B read through a table of row blocks (b_block_off), with a row map"""
    import torch
    ops = _ops()
    rng = np.random.default_rng(99)
    M, N, K, brows = 128 * 27, 128 * 24, 512, 256
    nblk = N // brows
    A, B, C0 = _operands(rng, M, N, K, G=0)
    perm = rng.permutation(nblk + 2)[:nblk]
    flat = np.full(((nblk + 2) * brows, K), np.nan)
    for i, q in enumerate(perm):
        flat[q * brows:(q + 1) * brows] = B[i * brows:(i + 1) * brows]
    boff = torch.from_numpy((perm * brows * K).astype(np.int64)).to(ops.device)
    reach = np.minimum(N, 256 + 3 * 128 * np.arange(M // 128)).astype(np.int32)
    reach[-1] = N
    rm = torch.from_numpy(reach).to(ops.device)
    Ad, Fd = torch.from_numpy(A).to(ops.device), torch.from_numpy(flat.reshape(-1)).to(ops.device)
    for m in (rm, None):
        def launch(Cd, m=m):
            ops.gemm_nt_blocks(Cd[:, :N], Ad, Fd, K, boff, brows, m, 128, reach if m is not None else None)
        _both(ops, launch, C0)


def test_tall_fit_predict_N16384_bitwise():
    """one fit + predict at N = 16384 with the tall form off and on: identical LML, mean, variance and alpha"""
    import sys
    import os
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "oracle"))
    import gp_oracle as O
    from gaussian_process_amd import GPContext
    X, y, Xs = O.synthetic_problem(16384, 8, 1024)
    res = []
    with GPContext(0) as ctx:
        for form in (0, 1):
            ctx.set_option("gemm_tall", form)
            ctx.set_option("tall_min_tiles", 0)
            lml, mu, var = ctx.fit_predict(X, y, Xs, 1.0, 2.0, 5e-4, want_sd=False)
            res.append((lml, mu, var, ctx.alpha()))
    (l0, m0, v0, a0), (l1, m1, v1, a1) = res
    assert l0 == l1
    assert np.array_equal(m0, m1) and np.array_equal(v0, v1) and np.array_equal(a0, a1)
