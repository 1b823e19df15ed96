"""Every kernel form of the update GEMM (gemm_nt.hip: launch_gemm_nt, gemm_dma.hip: launch_gemm_nt_dma) against an
exact result and against an error bound (gemm_contract.py), not only against another form.

ROUTES is derived from the two launchers: the options (gpmi_dev_set_option, thread-local) and the shapes that select
each form.  The kernel each route should reach is named next to it; a kernel trace of this file shows them all.
Options are restored in `finally`, so a failing case leaves the defaults to the rest of the suite."""
import contextlib

import numpy as np
import pytest

import gemm_contract as GC
from gemm_contract import Case

pytestmark = pytest.mark.gpu

DEFAULTS = dict(gemm_dma=1, gemm_small_tiles=1, gemm_small_dma=1, gemm_persist=1, gemm_ticket=0, gemm_dma_waves=8,
                gemm_tall=1, tall_min_tiles=12288)


def _lowers(M, N, K):
    # diag_off: on the diagonal, panel_rec's -64, above it, well below it, everything live, nothing live
    return [Case(M, N, K, lower=1, diag_off=o) for o in (0, -64, 128, -384, N, -M)]


# fewer than 128 tiles of 128 x 128
SMALL = [Case(640, 640, 16), Case(640, 640, 48), Case(640, 640, 256), Case(640, 640, 1040),
         Case(384, 1088, 48), Case(1280, 704, 48),
         *_lowers(1024, 1024, 48), Case(640, 640, 1040, lower=1, diag_off=-64), Case(1280, 768, 48, lower=1)]
# row maps: reaches off the 128 grid, an empty band, bands of three tiles, a partial last band
SMALL_MAPS = [Case(640, 768, 48, reach=(300, 0, 768, 129, 700)),
              Case(640, 768, 48, reach=(300, 0, 768, 129, 700), host_map=False),
              Case(896, 640, 32, reach=(200, 640, 520), rbr=384),
              Case(896, 640, 1040, reach=(200, 640, 520), rbr=384, host_map=False)]
# N % 128 == 64
ODD64 = [Case(640, 704, 48), Case(384, 1088, 1040), Case(640, 704, 16), *_lowers(1024, 1088, 48),
         Case(640, 832, 48, reach=(100, 832, 0, 577, 64)), Case(896, 832, 48, reach=(300, 700, 832), rbr=384, host_map=False),
         Case(1536, 1600, 48)]
# 128 tiles and more (an odd number of tile rows splits the tall form's pairs)
BIG = [Case(1664, 1664, 32), Case(1664, 1664, 48), Case(1664, 1664, 256), Case(1664, 1664, 1040), Case(1664, 1664, 16),
       Case(1408, 1920, 48), Case(1920, 1152, 256),
       *_lowers(1664, 1664, 48), Case(1664, 1664, 1040, lower=1, diag_off=-64), Case(1920, 1152, 48, lower=1)]
BIG_MAPS = [Case(1920, 1920, 48, reach=tuple(min(1920, 300 + 131 * q) for q in range(14)) + (0,)),
            Case(1920, 1920, 48, reach=tuple(min(1920, 300 + 131 * q) for q in range(14)) + (0,), host_map=False),
            Case(1920, 1920, 272, reach=(129, 1920, 700, 1000, 1), rbr=384),
            Case(1920, 1920, 48, reach=(700, 1920, 1300, 1025), rbr=512),
            Case(1920, 1920, 48, reach=(700, 1920, 1300, 1025), rbr=512, host_map=False)]
BLOCKS = [Case(1536, 1920, 48, brows=256),
          Case(1536, 1920, 48, reach=tuple(min(1920, 100 + 250 * q) for q in range(12)), brows=256),
          Case(1536, 1920, 1040, reach=(1920, 640, 1500, 129), rbr=384, brows=384)]
# at least two rounds of 256 blocks with K >= 256 (persistent), at least one round (ticket)
# (a staircase with its host copy launches only its live supertiles: 30 bands, so that they still make two rounds)
STAIRS = tuple(2944 - 29 * q for q in range(30))
PERSIST = [Case(2944, 2944, 256), Case(2944, 2944, 272),
           Case(3840, 2944, 256, reach=STAIRS),
           Case(3840, 2944, 256, reach=STAIRS, host_map=False),
           Case(3840, 2944, 256, reach=STAIRS, brows=256)]
TICKET = [Case(2304, 2304, 48), Case(2304, 2304, 1040),
          Case(2304, 2304, 48, reach=tuple(2304 - 37 * q for q in range(18))),
          Case(2304, 2304, 48, reach=tuple(2304 - 37 * q for q in range(18)), host_map=False),
          Case(2304, 2304, 48, reach=tuple(2304 - 37 * q for q in range(18)), brows=256)]

# name: (options, under gpmi_dev_set_concurrent(1), kernel, cases)
ROUTES = {
    "small_dma8": ({}, False, "gemm_nt_small_kernel<8>", SMALL),
    "small_dma3": ({}, True, "gemm_nt_small_kernel<3>", SMALL),
    "reg64": ({"gemm_small_dma": 0}, False, "gemm_nt_kernel<2, 2, false>", SMALL + SMALL_MAPS),
    "reg128": ({"gemm_dma": 0, "gemm_small_tiles": 0}, False, "gemm_nt_kernel<4, 4, false>",
               [c for c in SMALL if c.N % 128 == 0] + SMALL_MAPS + [Case(1664, 1664, 1040, lower=1, diag_off=-64)]),
    "reg128x64": ({"gemm_small_tiles": 0}, False, "gemm_nt_kernel<4, 2, false>", ODD64),
    "dma8": ({"gemm_persist": 0, "gemm_tall": 0}, False, "gemm_nt_dma_kernel<2, false>", BIG + BIG_MAPS + BLOCKS),
    "dma4": ({"gemm_persist": 0, "gemm_tall": 0, "gemm_dma_waves": 4}, False, "gemm_nt_dma_kernel<4, false>",
             BIG + BIG_MAPS + BLOCKS),
    "tall": ({"gemm_persist": 0, "gemm_tall": 1, "tall_min_tiles": 0}, False, "gemm_nt_dma_tall_kernel<false>",
             BIG + BIG_MAPS + BLOCKS),
    "persist": ({}, False, "gemm_nt_dma_persist_kernel", PERSIST),
    "ticket": ({"gemm_ticket": 2}, False, "gemm_nt_dma_ticket_kernel", TICKET),
}


@pytest.fixture(scope="module")
def ops():
    from gaussian_process_amd.dist import HipBlockOps
    return HipBlockOps(0)


@contextlib.contextmanager
def route(ops, name):
    opts, concurrent = ROUTES[name][:2]
    try:
        for k, v in opts.items():
            ops.set_option(k, v)
        if concurrent:
            ops.set_concurrent(1)
        yield
    finally:
        if concurrent:
            ops.set_concurrent(0)
        for k in opts:
            ops.set_option(k, DEFAULTS[k])


def _ids(name):
    return [(name, c) for c in ROUTES[name][3]]


ALL = [rc for name in ROUTES for rc in _ids(name)]


@pytest.mark.parametrize("name,case", ALL, ids=["%s-%s" % (n, c) for n, c in ALL])
def test_route_exact(ops, name, case):
    with route(ops, name):
        GC.check_exact(ops, case)


# full-mantissa operands on every route: a plain launch, lower mode on an odd offset, a row map
BOUND = {
    "small_dma8": [Case(640, 640, 1040), Case(1024, 1024, 48, lower=1, diag_off=-64)],
    "small_dma3": [Case(640, 640, 1040), Case(1024, 1024, 48, lower=1, diag_off=-64)],
    "reg64": [Case(640, 640, 1040), Case(1024, 1024, 48, lower=1, diag_off=-64), SMALL_MAPS[2]],
    "reg128": [Case(640, 640, 1040), Case(1024, 1024, 48, lower=1, diag_off=-64), SMALL_MAPS[2]],
    "reg128x64": [Case(384, 1088, 1040), Case(1024, 1088, 48, lower=1, diag_off=-64), ODD64[-2]],
    "dma8": [Case(1664, 1664, 1040), Case(1664, 1664, 48, lower=1, diag_off=-64), BIG_MAPS[2], BLOCKS[2]],
    "dma4": [Case(1664, 1664, 1040), Case(1664, 1664, 48, lower=1, diag_off=-64), BIG_MAPS[2], BLOCKS[2]],
    "tall": [Case(1664, 1664, 1040), Case(1664, 1664, 48, lower=1, diag_off=-64), BIG_MAPS[2], BLOCKS[2]],
    "persist": [PERSIST[1], PERSIST[2]],
    "ticket": [TICKET[1], TICKET[2]],
}
ALL_BOUND = [(n, c) for n in BOUND for c in BOUND[n]]


@pytest.mark.parametrize("name,case", ALL_BOUND, ids=["%s-%s" % (n, c) for n, c in ALL_BOUND])
def test_route_error_bound(ops, name, case):
    with route(ops, name):
        GC.check_bound(ops, case)


def _bits(ops, name, case, seed=5):
    with route(ops, name):
        out, _, _, _ = GC.run(ops, case, seed, exact=False)
    return out


@pytest.mark.parametrize("case", [PERSIST[1], PERSIST[2], PERSIST[4]], ids=str)
def test_dma_forms_same_bits(ops, case):
    """the per-tile 8-wave kernel, the tall form, the persistent and the ticket form run the same MFMAs per
    accumulator in the same order: the same bits, full-mantissa operands"""
    ref = _bits(ops, "dma8", case)
    assert np.all(np.isfinite(ref))
    for name in ("tall", "persist", "ticket"):
        got = _bits(ops, name, case)
        assert np.array_equal(got, ref), "%s: %s differs from dma8, max |diff| %g" % (case, name, np.max(np.abs(got - ref)))


@pytest.mark.parametrize("case", [Case(640, 640, 1040, lower=1, diag_off=-64), Case(384, 1088, 48), Case(1024, 1024, 16)],
                         ids=str)
def test_small_ring_depth_same_bits(ops, case):
    """gpmi_dev_set_concurrent(1) switches the small LDS-DMA kernel to its 3-stage ring: "same results" (gpmi.h)"""
    ref = _bits(ops, "small_dma8", case)
    got = _bits(ops, "small_dma3", case)
    assert np.all(np.isfinite(ref))
    assert np.array_equal(got, ref), "max |diff| %g" % np.max(np.abs(got - ref))

