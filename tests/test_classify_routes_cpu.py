"""Why tests/test_classify_routes_gpu.py has no case for gemm_tall, gemm_persist and gemm_ticket: asked for the
largest GEMM launches of its problems (Np = 768 and 1152: at most 9 x 9 tiles of 128 x 128), the library's route function
(csrc/gpmi_route.h: gemm_route, through tests/sanitize/gemm_route_check.cpp) answers the 64 x 64 ring under every value
of the three options, alone on the chip and beside a lookahead panel; gemm_small_tiles and gemm_small_dma are what
change the kernel at these shapes.  No GPU."""
import pytest

import gemm_route_table as T
from test_gemm_route_cpu import MI355X_GROUPS, query, route_check       # noqa: F401 (route_check is a fixture)

C = T.Case
# Np = 1152 and 768.  softmax_fit's E_c = V V^T, last and first row block (M = nb, N = r0 + nb, K = Np - r0, lower,
# diag_off = r0); softmax_predict's B_c = R E_c with 300 -> 384 test rows; a whole-matrix update as an upper bound of
# every trailing update inside cholesky_inplace and solve_sweep
LAUNCHES = [C(128, 1152, 128, lower=1, diag_off=1024), C(512, 512, 1152, lower=1), C(512, 1024, 640, lower=1, diag_off=512),
            C(384, 1152, 1152), C(1152, 1152, 512), C(1152, 1152, 512, lower=1),
            C(256, 768, 256, lower=1, diag_off=512), C(384, 768, 768), C(768, 768, 512, lower=1)]
SMALL8, SMALL3 = "gemm_nt_small_kernel<8>", "gemm_nt_small_kernel<3>"
LDS_DMA_OPTIONS = [dict(gemm_tall=1, tall_min_tiles=0), dict(gemm_tall=0), dict(gemm_persist=0), dict(gemm_persist=1),
                   dict(gemm_ticket=1), dict(gemm_ticket=2)]


def test_the_lds_dma_options_cannot_reach_a_classification_launch(route_check):
    asked, want = [], []
    for case in LAUNCHES:
        assert (case.M // 128) * (case.N // 128) < 128
        for more in LDS_DMA_OPTIONS:
            for sharing, kernel in (((0, 0), SMALL8), ((0, 1), SMALL8), ((1, 1), SMALL3)):
                asked.append(query(MI355X_GROUPS, "small_dma8", case, sharing=sharing, **more))
                want.append(kernel)
    got = route_check(asked)
    wrong = ["%s: want %s, gemm_route %s" % (q, w, g) for q, w, g in zip(asked, want, got) if g != w]
    assert not wrong, "\n".join(wrong)


def test_the_small_tile_options_can(route_check):
    asked = [query(MI355X_GROUPS, "small_dma8", case, **more) for case in LAUNCHES
             for more in (dict(gemm_small_tiles=0), dict(gemm_small_dma=0))]
    got = route_check(asked)
    assert set(got[0::2]) == {"gemm_nt_kernel<4, 4, false>"} and set(got[1::2]) == {"gemm_nt_kernel<2, 2, false>"}
