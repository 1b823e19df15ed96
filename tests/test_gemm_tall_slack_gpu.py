"""The 256 x 128 form where only Sharing::panel_slack reaches it -- launches between tall_min_tiles_slack (1024) and
tall_min_tiles (12288) live tiles, every option at its default -- against the 128 x 128 form (gemm_tall 0), bit for bit
and over the whole C buffer, guard rows and columns included.  The state is the one a Cholesky of 49152 columns and
more runs its update launches in (csrc/driver.hip); the block primitives enter it with gpmi_dev_set_concurrent(2).
Which kernel each shape reaches in and out of the state: tests/test_gemm_route_slack_cpu.py."""
import numpy as np
import pytest

import test_gemm_tall_gpu as TG

pytestmark = pytest.mark.gpu


def _run(ops, form, launch, C0):
    """launch(Cview) in the slack state under gemm_tall = form, the bars at their defaults -> the whole C buffer"""
    import torch
    ops.set_option("gemm_tall", form)
    assert ops.lib.gpmi_dev_set_concurrent(2) == 0
    try:
        Cd = torch.from_numpy(C0).to(ops.device)
        launch(Cd)
        torch.cuda.synchronize()
        return Cd.cpu().numpy()
    finally:
        assert ops.lib.gpmi_dev_set_concurrent(0) == 0
        ops.set_option("gemm_tall", 1)


def _both(ops, launch, C0):
    tall = _run(ops, 1, launch, C0)
    ref = _run(ops, 0, launch, C0)
    assert np.all(np.isfinite(ref))
    assert np.array_equal(tall, ref), "max |diff| %g" % np.max(np.abs(tall - ref))
    return ref


@pytest.mark.parametrize("Tm", [72, 73])
def test_next_block_column_shape_bitwise(Tm):
    """part (a) of a step at the headline size: lower, 2048 columns, diag_off 0, K = 2048; 72 and 73 tile rows hold
    1032 and 1048 live tiles (an odd count of tile rows splits the last pair)"""
    ops = TG._ops()
    rng = np.random.default_rng(4000 + Tm)
    M, N, K = 128 * Tm, 2048, 2048
    A, B, C0 = TG._operands(rng, M, N, K)
    ref = _both(ops, TG._gemm(ops, A, B, M, N, K, 1, 0), C0)
    G = 128
    assert np.array_equal(ref[G:G + 128, G + 128:G + N], C0[G:G + 128, G + 128:G + N])      # above the diagonal: untouched
    want = np.tril(C0[G:G + N, G:G + N] - A[:N] @ B.T)
    assert np.allclose(np.tril(ref[G:G + N, G:G + N]), want, rtol=0, atol=1e-10 * np.abs(want).max())


@pytest.mark.parametrize("Tm", [132, 133])
def test_panel_internal_shape_bitwise(Tm):
    """the top-level update inside a 2048-column panel (panel_rec): M x 1024, K = 1024, lower with diag_off 0 (the
    updated columns start on the 128 grid, so r0 == c0); 132 tile rows are the first with 1024 live tiles"""
    ops = TG._ops()
    rng = np.random.default_rng(5000 + Tm)
    M, N, K = 128 * Tm, 1024, 1024
    A, B, C0 = TG._operands(rng, M, N, K)
    _both(ops, TG._gemm(ops, A, B, M, N, K, 1, 0), C0)


@pytest.mark.parametrize("rbt", [1, 3])
def test_row_map_in_the_state_bitwise(rbt):
    """the block primitives reach the state with a row map (33 x 40 tiles: 1320 in the rectangle), with its host copy
    and without"""
    import torch
    ops = TG._ops()
    rng = np.random.default_rng(6000 + rbt)
    M, N, K = 128 * 33, 128 * 40, 512
    bands = -(-(M // 128) // rbt)
    reach = np.minimum(N, 3000 + 128 * rbt * np.arange(bands)).astype(np.int32)
    reach[-1] = N
    A, B, C0 = TG._operands(rng, M, N, K, G=0)
    Ad, Bd = torch.from_numpy(A).to(ops.device), torch.from_numpy(B).to(ops.device)
    rm = torch.from_numpy(reach).to(ops.device)
    for host in (reach, None):
        def launch(Cd, host=host):
            ops.gemm_nt_rowmap(Cd[:, :N], Ad, Bd, rm, 128 * rbt, host)
        _both(ops, launch, C0)
