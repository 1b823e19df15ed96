"""References of the kernel-matrix build (gaussian_process_amd/csrc/rbf.hip) -- TEST INFRASTRUCTURE shared by
tests/test_kbuild_ref_cpu.py and tests/test_kbuild_routes_gpu.py:

  * an exact emulation of the two device exps, exp_neg_tab (rbf.hip; the register kernel) and exp_neg_fast (exp_dev.h;
    the LDS and global-memory kernels), operation for operation, with every fused multiply-add as ONE exact rounding
    (through fractions.Fraction).  The table is built the way rbf.hip's exp_table_ready builds it: exp2 in long double
    (this machine's libm, as the library's host code calls it), rounded to double;
  * the directed argument set: the arguments at which such an exp goes wrong first -- every tie between two table
    entries, every binade boundary, both ends of the domain -- as 1-D inputs b with a = 0, l = 1, so that the device
    computes the argument -0.5 fl(b^2) exactly as NumPy does;
  * the value sig2 P(t) exp(x) of every family in long double from the double argument x, and the bars of the issue
    that introduced this file, in units of u = 2^-53 relative.
"""
import functools
import math
from fractions import Fraction

import mpmath
import numpy as np

U = 2.0 ** -53
LD = np.longdouble
EXP_TAB = 4096
LOG2E = 1.4426950408889634074
LN2_HI = 6.93147180369123816490e-01
LN2_LO = 1.90821492927058770002e-10
MAGIC = 6755399441055744.0                      # 1.5 * 2^52
MAGIC_TAB = MAGIC / EXP_TAB
FAST_C = [float.fromhex(h) for h in (           # c11 .. c2 of exp_neg_fast
    "0x1.ad7f3c1cdbf13p-26", "0x1.28ad9b87c947cp-22", "0x1.71df25b4b9501p-19", "0x1.a01999e260c97p-16",
    "0x1.a01a012a0e822p-13", "0x1.6c16c18438b14p-10", "0x1.1111111127d10p-7", "0x1.555555555083ep-5",
    "0x1.55555555554f9p-3", "0x1.000000000000ap-1")]
C3 = 0.33333333333333331                        # cov_poly: the double nearest 1/3

# The bars, in ulp of the true value (one ulp of v lies in (u |v|, 2 u |v|]).
# E_TAB: 0.501 (table entry) + 0.5 (final fused multiply-add) + (ln2 / 8192)^4 / 24 relative <= 0.02 (the cubic's
# truncation); the result never leaves the table entry's binade.  E_FAST: exp_dev.h's stated bound.
# E_LIB: the device library's double exp, which a wave takes when one of its lanes leaves [-700, 0].  A ROCm
# installation carries no accuracy table of its own; the bound is the one of the HIP documentation's table of
# double-precision device functions ("HIP math API": exp, maximum ULP difference 1).
E_TAB = 1.03
E_FAST = 1.0
E_LIB = 1.0
SUBNORMAL_ATOL = 2e-323                         # the suite's bar for the last bits of subnormal results
M_FAMILY = {0: 0, 1: 0, 2: 2, 3: 5}             # further single roundings, all on positive terms: P and P * e


def route_bar(E, F, sig2):
    """relative bar of one element against the long-double value: (2 E + m) u"""
    return (2.0 * E + M_FAMILY[F] + (0 if sig2 == 1.0 else 1)) * U


def fma(a, b, c):
    """a * b + c rounded once (int / int division in Fraction.__float__ is correctly rounded)"""
    return float(Fraction(a) * Fraction(b) + Fraction(c))


@functools.lru_cache(maxsize=None)
def table():
    """2^(j / 4096) as exp_table_ready computes it: (double)exp2l(j / 4096.L)"""
    assert np.finfo(LD).nmant >= 63, "long double is not the x87 extended format here"
    j = np.arange(EXP_TAB).astype(LD)
    return np.exp2(j / LD(EXP_TAB)).astype(np.float64)


@functools.lru_cache(maxsize=None)
def table_true():
    """the correctly rounded table (mpmath, 60 digits) and each entry's true value"""
    with mpmath.workprec(200):
        true = [mpmath.power(2, mpmath.mpf(j) / EXP_TAB) for j in range(EXP_TAB)]
        return np.array([float(v) for v in true]), true


def exp_neg_tab(x, T=None):
    T = table() if T is None else T
    t = fma(x, LOG2E, MAGIC_TAB)
    n = t - MAGIC_TAB
    r = fma(-n, LN2_HI, x)
    r = fma(-n, LN2_LO, r)
    m = int(n * EXP_TAB)                        # the low word of t: 4096 k + j (exact)
    assert m == n * EXP_TAB and -2 ** 31 <= m < 2 ** 31
    Tj = float(T[m & (EXP_TAB - 1)])
    q = fma(r, 1.0 / 6.0, 0.5)
    q = fma(q, r, 1.0)
    q = q * r
    e = fma(Tj, q, Tj)
    return math.ldexp(e, m >> 12)               # k added to the exponent field: exact while the result is normal


def exp_neg_fast(x):
    t = fma(x, LOG2E, MAGIC)
    n = t - MAGIC
    r = fma(-n, LN2_HI, x)
    r = fma(-n, LN2_LO, r)
    q = FAST_C[0]
    for c in FAST_C[1:]:
        q = fma(q, r, c)
    q = fma(q, r, 1.0)
    q = fma(q, r, 1.0)
    return math.ldexp(q, int(n))


def arg_of(b):
    """the exp argument of a = 0, l = 1, sigma = 1 against the 1-D input b: coef * ((0 - b) * (0 - b)), coef = -0.5"""
    b = np.asarray(b, dtype=np.float64)
    return -0.5 * (b * b)


def _b_for(x):
    """the b >= 0 whose argument -0.5 fl(b^2) is nearest the real number x <= 0"""
    b0 = float(mpmath.sqrt(-2 * mpmath.mpf(x)))
    cand = [b0, math.nextafter(b0, 0.0), math.nextafter(b0, math.inf)]
    return min(cand, key=lambda b: abs(mpmath.mpf(float(arg_of(b))) - x))


def _with_neighbours(b):
    return [math.nextafter(b, 0.0), b, math.nextafter(b, math.inf)]


NOCHECK_EDGE = -689.9       # the largest |argument| of the core set: a bounding box with it still proves the domain


@functools.lru_cache(maxsize=None)
def directed():
    """-> dict: b_core (arguments in [-689.9, 0]: a launch on them takes the nocheck form), b_ext (arguments in
    [-700, -689.9)), and per part the arguments x and both emulated exps.  About 14 000 arguments, emulated once."""
    with mpmath.workprec(120):
        ln2 = mpmath.ln(2)
        step = ln2 / EXP_TAB
        bs = [0.0, 2.0 ** -26]                                              # arguments 0 and -2^-53
        for i in range(EXP_TAB):                                            # every tie of the first period
            bs += _with_neighbours(_b_for(-(i + mpmath.mpf(0.5)) * step))
        for k in (37, 1009):                                                # ... of every 64th entry far down
            for j in range(0, EXP_TAB, 64):
                x = -(k * EXP_TAB + j + mpmath.mpf(0.5)) * step
                if x >= -700:
                    bs += _with_neighbours(_b_for(x))
        k = 0
        while -k * ln2 >= -700:                                             # every binade boundary
            bs.append(_b_for(-k * ln2))
            k += 1
        for x in (NOCHECK_EDGE, -699.999, -700.0):
            bs.append(_b_for(mpmath.mpf(x)))
    b = np.unique(np.array(bs))
    while arg_of(b[-1]) < -700.0:                                           # the nearest reachable argument at or above -700
        b = np.append(b[:-1], math.nextafter(b[-1], 0.0))
    b = np.unique(b)
    x = arg_of(b)
    assert x.min() >= -700.0 and x.min() < -699.9999 and x.max() == 0.0
    edge = float(arg_of(_b_for(mpmath.mpf(NOCHECK_EDGE))))
    core = x >= edge
    out = {}
    for name, sel in (("core", core), ("ext", ~core)):
        out["b_" + name], out["x_" + name] = b[sel], x[sel]
        out["tab_" + name] = np.array([exp_neg_tab(float(v)) for v in x[sel]])
        out["fast_" + name] = np.array([exp_neg_fast(float(v)) for v in x[sel]])
    for v in out.values():
        v.setflags(write=False)
    return out


def ulp_errors(got, x):
    """|got - exp(x)| in ulp of the true value, against mpmath at 50 digits"""
    err = np.empty(len(x))
    with mpmath.workdps(50):
        for i, (g, xi) in enumerate(zip(got, x)):
            v = mpmath.exp(mpmath.mpf(float(xi)))
            ulp = mpmath.ldexp(1, int(mpmath.floor(mpmath.log(v, 2))) - 52)
            err[i] = float(abs(mpmath.mpf(float(g)) - v) / ulp)
    return err


def poly_ld(F, x):
    """P(t) of family F at t = -x, in long double"""
    assert np.finfo(LD).nmant >= 63
    t = -np.asarray(x, dtype=np.float64).astype(LD)
    return np.ones_like(t) if F <= 1 else LD(1) + t if F == 2 else (LD(1) + t) + (t * t) * LD(C3)


def value_ld(F, x, sig2):
    """sig2 P(t) exp(x) in long double from the double exp argument x = -t (P as include/gpmi.h defines it, with the
    double c3)"""
    xl = np.asarray(x, dtype=np.float64).astype(LD)
    return LD(sig2) * (poly_ld(F, x) * np.exp(xl))


def rel_error_u(got, ref_ld):
    """max |got - ref| / |ref| in units of u over the elements whose reference is a normal double"""
    ref_ld = np.asarray(ref_ld)
    ok = np.abs(ref_ld) >= LD(2.2250738585072014e-308)
    if not ok.any():
        return 0.0
    g = np.asarray(got, dtype=np.float64).astype(LD)
    return float(np.max(np.abs(g[ok] - ref_ld[ok]) / np.abs(ref_ld[ok])) / U)
