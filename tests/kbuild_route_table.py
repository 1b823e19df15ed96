"""The route table of the kernel-matrix build: which covariance kind, d, shapes and options reach which kernel of
csrc/rbf.hip in which form -- TEST INFRASTRUCTURE shared by tests/test_kbuild_routes_gpu.py, which runs the cases on
the GPU, and tests/test_kbuild_route_cpu.py, which asks the library's one route function (csrc/gpmi_kroute.h:
rbf_route) for every case and asserts what is written here.

A case is one launch as one of three entry points makes it:
    cov    GPContext.cov(kind, A, B, ...): rectangular, row0 = 0, the bounding boxes of A and B bound the exp argument
    rows   HipBlockOps.rbf_rows / cov_rows: symmetric rows row0 .. of K(X, X) + s I (triangular enumeration when
           row0 == 0 and the launch is square), no bounding box
    cross  HipBlockOps.rbf_cross / cov_cross: rectangular, no bounding box
A claim names the kernel a case reaches, the launch geometry, and the tile forms its tiles take:
    interior   a tile fully inside the matrix and off the diagonal (the register kernel: one of four specialisations,
               check / nocheck by the bounding box, unit / non-unit by sigma^2)
    edge       a tile that crosses the last real row or column
    diag       symmetric builds: a tile that holds global row == column
    skipped    symmetric builds of the register kernel: a work item without a live tile
"""
from collections import namedtuple

import numpy as np

RT = 128
RBF_BLOCKS = 16384                       # Tuning::rbf_blocks
FAMILY_KIND = {0: 0, 1: 4, 2: 5, 3: 6}   # compile-time family F -> kind of include/gpmi.h
KIND_NAME = {0: "rbf", 1: "lin", 2: "per", 3: "co2", 4: "matern12", 5: "matern32", 6: "matern52"}
TWO_NU = {4: 1.0, 5: 3.0, 6: 5.0}
REG_D = (1, 2, 3, 4, 5, 6, 7, 8, 16)
LDS_D = (9, 12, 32)
NAIVE_D = (33, 129)                      # 129: the recursive-halving sum above 128 terms
CO2 = [1.1, 0.9, 0.6, 1.7, 1.3, 0.4, 0.8, 1.5, 0.3, 0.2, 0.05]
OTHER_PARAMS = {1: [0.25], 2: [1.7, 0.9], 3: CO2}
NOISE = 0.0625

_Case = namedtuple("Case", "api kind d nA nB row0 nrows ncols sigma ell width far blocks")


def round_up(n, m=RT):
    return (n + m - 1) // m * m


def Case(api, kind, d, nA, nB, row0=0, nrows=None, ncols=None, sigma=1.3, ell=None, width=4.0, far=False, blocks=None):
    """nA / nB: real rows / columns (rows: nA == nB == N); width: inputs are uniform in [0, width]^d; far: one more row of
    A far from everything else, so that the bounding box no longer proves the exp domain; blocks: rbf_blocks (None: the
    default); ell None: 1.1 sqrt(d)"""
    if api == "rows":
        assert nA == nB and nrows is not None and ncols is not None
    else:
        assert row0 == 0 and nrows is None and ncols is None
        nrows, ncols = round_up(nA + int(far)), round_up(nB)
    return _Case(api, kind, d, nA, nB, row0, nrows, ncols, sigma, 1.1 * float(np.sqrt(d)) if ell is None else ell, width, far,
                 blocks)


def stationary(kind):
    return kind in (0, 4, 5, 6)


def coef(case):
    """gpmi_internal.h: cov_coef"""
    if case.kind == 0:
        return -.5 * (1 / (case.ell * case.ell))
    if case.kind in TWO_NU:
        return -(float(np.sqrt(TWO_NU[case.kind])) / abs(case.ell))
    return 0.0


def params(case):
    """the parameter list of cov_rows / cov_cross (and p0, p1 of GPContext.cov)"""
    return [case.sigma, case.ell] if stationary(case.kind) else OTHER_PARAMS[case.kind]


def far_coordinate(case):
    """first coordinate of the far row.  Squared exponential: its worst exp argument against [0, width] is about -720, so
    that its waves are some inside the domain, some outside with normal, subnormal and no zero results.  Matern: about
    -706, every wave outside the domain and every result normal (P(t) would multiply the absolute error of a subnormal
    exp, and no relative bar would hold)."""
    return float(np.sqrt(2 * 720.0)) * case.ell if case.kind == 0 else 706.0 / -coef(case)


def inputs(case):
    """A (rows) and B (columns) of the case, the same on every call.  The corners 0 and width are planted in both, so
    that the bounding boxes are [0, width]^d exactly and the worst argument of the box is one an element takes."""
    rng = np.random.default_rng(1000 * case.kind + 10 * case.d + case.nA + case.nB)
    A = rng.uniform(0.0, case.width, (case.nA, case.d))
    B = A if case.api == "rows" else rng.uniform(0.0, case.width, (case.nB, case.d))
    if case.api == "cov" and case.d == 1:
        A[0], A[1] = 0.0, case.width
        B[0], B[1] = case.width, 0.0
    if case.far:
        row = rng.uniform(0.0, case.width, (1, case.d))
        row[0, 0] = far_coordinate(case)
        A = np.vstack([A, row])
    return A, B


def box_max_sq(A, B):
    """gpmi_ctx.h: box_max_sq of the two bounding boxes"""
    s = 0.0
    for k in range(A.shape[1]):
        w = max(A[:, k].max() - B[:, k].min(), B[:, k].max() - A[:, k].min())
        s += w * w
    return float(s) if np.isfinite(s) else -1.0


def max_sq(case):
    if case.api != "cov" or not stationary(case.kind):
        return -1.0
    return box_max_sq(*inputs(case))


Claim = namedtuple("Claim", "case kernel tri strip nocheck forms")


def claim(case, kernel, forms, tri=0, strip=1, nocheck=0):
    return Claim(case, kernel, tri, strip, nocheck, frozenset(forms.split()))


def interior_form(c):
    """the specialisation of the register kernel's interior loop a claim reaches"""
    return "%s_%s" % ("nocheck" if c.nocheck else "check", "unit" if c.case.sigma * c.case.sigma == 1.0 else "sigma")


def regs_name(D, F):
    return "rbf_regs_kernel<%d, %d>" % (D, F)


def stationary_name(d, F):
    return regs_name(d, F) if d in REG_D else "rbf_kernel<0, %d>" % F if d <= 32 else "rbf_naive_kernel<%d>" % F


# 300 x 512 through cov (row tiles 0, 1 inside, 2 across the last row; boxes [0, 4]^d: nocheck) and the 512 x 512 lower
# triangle of N = 450 through rows (tiles (1,0) (2,0) (2,1) interior, row 3 edge, four diagonal tiles; no box: check);
# sigma alternates with d so that each family meets all four interior specialisations
def _stationary_claims(F, d):
    kind = FAMILY_KIND[F]
    s_cov, s_rows = (1.0, 1.3) if d % 2 else (1.3, 1.0)
    name = stationary_name(d, F)
    return [claim(Case("cov", kind, d, 300, 512, sigma=s_cov), name, "interior edge", nocheck=1),
            claim(Case("rows", kind, d, 450, 450, 0, 512, 512, sigma=s_rows), name,
                  "interior edge diag" + (" skipped" if d in REG_D else ""), tri=1)]


STATIONARY = {(F, d): _stationary_claims(F, d) for F in range(4) for d in REG_D + LDS_D + NAIVE_D}


def _other_name(d):
    return "rbf_kernel<0, 0>" if d <= 32 else "cov_other_kernel"


OTHER = {(kind, d): [claim(Case("cov", kind, d, 300, 512), _other_name(d), "interior edge"),
                     claim(Case("rows", kind, d, 450, 450, 0, 512, 512), _other_name(d), "interior edge diag", tri=1)]
         for kind, d in [(1, 3), (1, 32), (1, 33), (3, 3), (3, 32), (3, 33), (3, 129), (2, 1)]}

# the three launch shapes beside the two above: symmetric rows below the top (rectangular enumeration with the
# symmetric skip), and a rectangular launch without a box
SHAPES = [claim(Case("rows", 0, 3, 450, 450, 128, 256, 512), regs_name(3, 0), "interior diag skipped"),
          claim(Case("rows", 0, 3, 450, 450, 256, 256, 512), regs_name(3, 0), "interior edge diag skipped"),
          claim(Case("rows", 5, 8, 450, 450, 256, 256, 512), regs_name(8, 2), "interior edge diag skipped"),
          claim(Case("rows", 6, 12, 450, 450, 128, 256, 512), "rbf_kernel<0, 3>", "interior diag"),
          claim(Case("rows", 4, 33, 450, 450, 256, 256, 512), "rbf_naive_kernel<1>", "interior edge diag"),
          claim(Case("rows", 3, 33, 450, 450, 128, 256, 512), "cov_other_kernel", "interior diag"),
          claim(Case("cross", 0, 5, 300, 500), regs_name(5, 0), "interior edge"),
          claim(Case("cross", 6, 16, 300, 500), regs_name(16, 3), "interior edge")]

# one far row appended to A: the box no longer proves the domain, the same tiles take the check form
FAR = [claim(Case("cov", FAMILY_KIND[F], d, 300, 512, sigma=sigma, far=True), stationary_name(d, F), "interior edge")
       for F, d, sigma in [(0, 1, 1.3), (1, 5, 1.0), (2, 16, 1.3), (3, 2, 1.0), (0, 9, 1.3), (2, 33, 1.3)]]

# persistent blocks: fewer blocks than work items (12 items of the 3 x 4 tiles; 16 items of the triangle, 6 of them skipped)
BLOCKS = [claim(Case(api, kind, d, *shape, blocks=b), regs_name(d, F), forms, tri=tri, nocheck=nocheck)
          for b in (1, 3, 7)
          for api, kind, d, F, shape, forms, tri, nocheck in [
              ("cov", 0, 3, 0, (300, 512), "interior edge", 0, 1),
              ("cov", 6, 6, 3, (300, 512), "interior edge", 0, 1),
              ("rows", 0, 3, 0, (450, 450, 0, 512, 512), "interior edge diag skipped", 1, 0),
              ("rows", 5, 8, 2, (450, 450, 0, 512, 512), "interior edge diag skipped", 1, 0)]]

# the nocheck decision from both sides of max_arg * 1.000001 >= -690: 256 x 256 (four interior tiles), d = 1, inputs
# in [0, w] with both corners planted, so that the worst argument of the box is taken and every argument is >= -700
W_RBF = {1: float(np.sqrt(2 * 689.9)), 0: float(np.sqrt(2 * 690.1))}        # ell = 1: the argument is -w^2 / 2
W_M12 = {1: 689.9, 0: 690.1}                                                # nu = 1/2, ell = 1: the argument is -w
THRESHOLD = [claim(Case("cov", kind, 1, 256, 256, sigma=sigma, ell=1.0, width=w[nc]), regs_name(1, F), "interior", nocheck=nc)
             for kind, F, w in [(0, 0, W_RBF), (4, 1, W_M12)] for nc in (1, 0) for sigma in (1.0, 1.3)]

# 4 row tiles per work item from 4096 tiles up (tests/test_kbuild_routes_gpu.py compares them with strip-1 chunks on the
# device): the lower triangle of 91 x 91 tiles (4186), 18 x 256 tiles (the last strip holds two row tiles)
STRIP_SYM_N, STRIP_SYM_NP, STRIP_SYM_CHUNK = 11600, 11648, 1024
STRIP_RECT = (2300, 2304, 32700, 32768, 512)                                # n, nrows, ncols_real, ncols, chunk rows
STRIP = [claim(Case("rows", 0, 8, STRIP_SYM_N, STRIP_SYM_N, 0, STRIP_SYM_NP, STRIP_SYM_NP, blocks=b), regs_name(8, 0),
               "interior edge diag skipped", tri=1, strip=4) for b in (None, 64)]
STRIP += [claim(Case("rows", 0, 8, STRIP_SYM_N, STRIP_SYM_N, r0, min(STRIP_SYM_CHUNK, STRIP_SYM_NP - r0), STRIP_SYM_NP),
                regs_name(8, 0), "interior diag skipped" + (" edge" if r0 + STRIP_SYM_CHUNK > STRIP_SYM_N else ""))
          for r0 in range(0, STRIP_SYM_NP, STRIP_SYM_CHUNK)]
STRIP += [claim(Case("cross", 0, 8, STRIP_RECT[0], STRIP_RECT[2]), regs_name(8, 0), "interior edge", strip=4),
          claim(Case("cross", 0, 8, STRIP_RECT[4], STRIP_RECT[2]), regs_name(8, 0), "interior edge"),
          claim(Case("cross", 0, 8, STRIP_RECT[0] % STRIP_RECT[4], STRIP_RECT[2]), regs_name(8, 0), "interior edge")]


def all_claims():
    out = [c for v in STATIONARY.values() for c in v] + [c for v in OTHER.values() for c in v]
    return out + SHAPES + FAR + BLOCKS + THRESHOLD + STRIP


# every (kernel, D, F) launch_rbf can instantiate
INSTANTIATIONS = ([regs_name(D, F) for F in range(4) for D in REG_D] + ["rbf_kernel<0, %d>" % F for F in range(4)] +
                  ["rbf_naive_kernel<%d>" % F for F in range(4)] + ["cov_other_kernel"])
