// exp_neg_fast: the polynomial exp of the kernel-matrix build, shared by rbf.hip and the leave-one-out gradient's
// derivative-matrix build (grad.hip).
#pragma once
#include <hip/hip_runtime.h>

namespace gpmi {

// exp(x) for the kernel's arguments (x <= 0): Cody-Waite reduction x = n*ln2 + r with the
// round-to-nearest n taken from the low bits of x*log2(e) + 1.5*2^52, a degree-11 minimax
// polynomial in r (|r| <= ln2/2; 1 + r + r^2 P(r) fitted for relative error by
// scripts/exp_poly_fit.py: 3.6e-18, 1.1e-17 with the coefficients rounded to double), and 2^n
// applied by adding n to the exponent field -- full-rate fp64 FMAs and one integer op, no
// v_rndne/v_cvt/v_ldexp.  The two leading coefficients are exactly 1, so exp(0) == 1 and the
// diagonal of K is sigma^2 exactly, as in NumPy.
// Valid while the result is a normal number; the caller falls back to the library exp
// for the whole wave if any lane is outside [-700, 0] (or NaN).  Error < 1 ulp (checked
// against NumPy at the 3-ulp parity tolerance of the K tests).
__device__ __forceinline__ double exp_neg_fast(double x) {
    const double MAGIC = 6755399441055744.0;                    // 1.5 * 2^52
    const double t = fma(x, 1.4426950408889634074, MAGIC);
    const double n = t - MAGIC;
    double r = fma(-n, 6.93147180369123816490e-01, x);          // ln2_hi (low bits zero: exact)
    r = fma(-n, 1.90821492927058770002e-10, r);                 // ln2_lo
    double q = 0x1.ad7f3c1cdbf13p-26;                           // c11
    q = fma(q, r, 0x1.28ad9b87c947cp-22);                       // c10
    q = fma(q, r, 0x1.71df25b4b9501p-19);                       // c9
    q = fma(q, r, 0x1.a01999e260c97p-16);                       // c8
    q = fma(q, r, 0x1.a01a012a0e822p-13);                       // c7
    q = fma(q, r, 0x1.6c16c18438b14p-10);                       // c6
    q = fma(q, r, 0x1.1111111127d10p-7);                        // c5
    q = fma(q, r, 0x1.555555555083ep-5);                        // c4
    q = fma(q, r, 0x1.55555555554f9p-3);                        // c3
    q = fma(q, r, 0x1.000000000000ap-1);                        // c2
    q = fma(q, r, 1.0);
    q = fma(q, r, 1.0);
    const int ni = __double2loint(t);                           // n in the low word of t (two's complement)
    return __hiloint2double(__double2hiint(q) + (ni << 20), __double2loint(q));
}

}  // namespace gpmi
