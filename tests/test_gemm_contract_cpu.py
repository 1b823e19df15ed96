"""The update GEMM's contract checker (gemm_contract.py) run against the NumPy stand-in the gloo tests use in place of
the HIP kernels: proves the checker without a GPU, and holds the stand-in to the same contract as the kernels
(test_gemm_routes_gpu.py).  Lower mode is a C-ABI-only launch and has no stand-in."""
import numpy as np
import pytest

import gemm_contract as GC
from gemm_contract import Case
from numpy_block_ops import NumpyBlockOps

CASES = [
    Case(384, 640, 48),
    Case(256, 192, 16),
    Case(640, 384, 272),
    # row maps: reaches off the 128 grid, an empty band, bands of three tiles, a partial last band
    Case(640, 768, 48, reach=(300, 0, 768, 129, 700)),
    Case(640, 768, 48, reach=(300, 0, 768, 129, 700), host_map=False),
    Case(896, 640, 32, reach=(200, 640, 520), rbr=384),
    # B as a table of row blocks, the last block reaching past N; with and without a row map
    Case(512, 640, 48, brows=256),
    Case(512, 640, 48, reach=(1, 255, 640, 400), brows=256),
]


@pytest.mark.parametrize("case", CASES, ids=str)
def test_numpy_block_ops_meets_the_gemm_contract(case):
    ops = NumpyBlockOps()
    GC.check_exact(ops, case)
    GC.check_bound(ops, case)


def test_contract_checker_bites():
    """the checker rejects an update that is off in one element, one that writes a dead tile, one that rounds through fp32"""
    class Off(NumpyBlockOps):
        def __init__(self, how):
            super().__init__()
            self.how = how

        def gemm_nt(self, Cm, A, B):
            if self.how == "fp32":
                self._a(Cm)[:] -= (self._a(A).astype(np.float32) @ self._a(B).T.astype(np.float32)).astype(np.float64)
            else:
                super().gemm_nt(Cm, A, B)
                self._a(Cm)[5, 7] += 0.25

        def gemm_nt_rowmap(self, Cm, A, B, row_ncols, row_block_rows, row_ncols_host=None):
            super().gemm_nt_rowmap(Cm, A, B, row_ncols, row_block_rows, row_ncols_host)
            self._a(Cm)[-1, -1] -= 1.0          # band 2 reaches 128 columns: the last tile of the row is dead

    for how, case, check in (("skip", Case(384, 512, 48), GC.check_exact),
                             ("dead", Case(384, 512, 48, reach=(200, 300, 128)), GC.check_exact),
                             ("fp32", Case(384, 512, 48), GC.check_bound)):
        with pytest.raises(AssertionError):
            check(Off(how), case)
