"""Every kernel form of the update GEMM against an exact result and against an error bound (gemm_contract.py), not only
against another form.

The routes -- the options (gpmi_dev_set_option, thread-local) and the shapes that select each form, with the kernel each
(route, case) reaches -- are the table of gemm_route_table.py.  The kernel is decided by one function, csrc/gpmi_route.h:
gemm_route, and tests/test_gemm_route_cpu.py holds the table against it, so the names there are checked facts; a
kernel trace of this file shows them all.
Options are restored in `finally`, so a failing case leaves the defaults to the rest of the suite."""
import contextlib

import numpy as np
import pytest

import gemm_contract as GC
from gemm_contract import Case
from gemm_route_table import BOUND, DEFAULTS, PERSIST, ROUTES

pytestmark = pytest.mark.gpu


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

