// Which kernel a launch of the kernel-matrix build (rbf.hip: launch_rbf) reaches, with what geometry: rbf_route() below
// is the ONE place that decides it.  Free of any HIP dependency like gpmi_route.h: hipcc compiles it into rbf.hip
// (launch_rbf switches over its answer), plain g++ under -fsanitize=address,undefined compiles it into
// tests/sanitize/kbuild_route_check.cpp, where tests/test_kbuild_route_cpu.py holds the route table of the GPU tests
// (tests/kbuild_route_table.py) against it.
#pragma once
#include <math.h>
#include <stddef.h>
#include <stdint.h>
#include <stdio.h>

#if defined(__HIPCC__)
#define GPMI_KROUTE_HD __host__ __device__
#else
#define GPMI_KROUTE_HD
#endif

namespace gpmi {

constexpr int RBF_TILE = 128;          // tile edge of every K-build kernel
constexpr int RBF_LDS_MAXD = 32;       // largest d staged in LDS; above: straight from global memory
constexpr int64_t RBF_STRIP_MIN_TILES = 4096;   // launches of at least this many tiles: 4 row tiles per work item

// Triangular tile enumeration of the symmetric build, and of the gradient kernels (grad.hip): linear index
// s = ti (ti + 1) / 2 + tj, 0 <= tj <= ti.  The float square root is a first guess only; the two loops make the answer exact for every s whose successor triangle number
// fits an int (ti <= 46339, far above the 1024 row tiles of N = 131072).
GPMI_KROUTE_HD inline void rbf_tri_tile(int s, int& ti, int& tj) {
    ti = (int)((sqrtf(8.f * (float)s + 1.f) - 1.f) * 0.5f);
    while ((ti + 1) * (ti + 2) / 2 <= s) ++ti;
    while (ti * (ti + 1) / 2 > s) --ti;
    tj = s - ti * (ti + 1) / 2;
}

enum class RbfKernel {
    Nothing,    // an empty shape (success)
    Invalid,    // unusable arguments (hipErrorInvalidValue)
    Regs,       // rbf_regs_kernel<D, F>: b columns in registers, table exp, persistent work items
    Lds,        // rbf_kernel<0, F>: both tile edges staged in LDS (F == 0 also serves kinds 1 .. 3 up to d = 32)
    Naive,      // rbf_naive_kernel<F>: operands straight from global memory
    Other,      // cov_other_kernel: kinds 1 .. 3 above d = 32
};

struct RbfRoute {
    RbfKernel kernel = RbfKernel::Invalid;
    int D = 0;          // Regs: the compile-time d
    int family = 0;     // the compile-time family F (0 for the kinds 1 .. 3)
    int Tm = 0, Tn = 0; // row and column tiles
    int tri = 0;        // triangular tile enumeration (symmetric, row0 == 0, square)
    int strip = 1;      // Regs: row tiles per work item
    int nitems = 0;     // Regs: strips x column tiles
    unsigned grid = 0;  // workgroups
    size_t lds = 0;     // dynamic LDS, bytes
    int nocheck = 0;    // host-proved: every exp argument of the launch lies in [-700, 0]
};

inline int rbf_family(int kind) { return (kind >= 4 && kind <= 6) ? kind - 3 : 0; }
inline bool rbf_stationary(int kind) { return kind == 0 || rbf_family(kind) != 0; }
// the d with a register specialisation
inline bool rbf_regs_d(int64_t d) { return (d >= 1 && d <= 8) || d == 16; }

// the symbol as a kernel trace prints it
inline const char* rbf_kernel_name(const RbfRoute& r, char (&buf)[48]) {
    switch (r.kernel) {
        case RbfKernel::Nothing: snprintf(buf, sizeof buf, "nothing"); break;
        case RbfKernel::Invalid: snprintf(buf, sizeof buf, "invalid"); break;
        case RbfKernel::Regs: snprintf(buf, sizeof buf, "rbf_regs_kernel<%d, %d>", r.D, r.family); break;
        case RbfKernel::Lds: snprintf(buf, sizeof buf, "rbf_kernel<0, %d>", r.family); break;
        case RbfKernel::Naive: snprintf(buf, sizeof buf, "rbf_naive_kernel<%d>", r.family); break;
        case RbfKernel::Other: snprintf(buf, sizeof buf, "cov_other_kernel"); break;
    }
    return buf;
}

// kind: RbfArgs::kind; rbf_blocks: Tuning::rbf_blocks; everything else as in RbfArgs
inline RbfRoute rbf_route(int kind, int64_t d, int64_t nrows, int64_t ncols, int symmetric, int64_t row0, double coef,
                          double max_sq, int rbf_blocks) {
    RbfRoute r;
    if (nrows <= 0 || ncols <= 0) { r.kernel = RbfKernel::Nothing; return r; }
    if (nrows % RBF_TILE || ncols % RBF_TILE || d <= 0) return r;
    if (symmetric && row0 % RBF_TILE) return r;
    if (kind < 0 || kind > 6 || (kind == 2 && d != 1)) return r;
    r.Tm = (int)(nrows / RBF_TILE);
    r.Tn = (int)(ncols / RBF_TILE);
    r.family = rbf_family(kind);
    // coef <= 0 and max_sq bounds every squared distance of this launch (NaN / unknown fail the test); a Matern's
    // argument is coef * sqrt(sq)
    const double max_arg = r.family ? coef * sqrt(max_sq) : coef * max_sq;
    r.nocheck = (max_sq >= 0.0 && coef <= 0.0 && max_arg * 1.000001 >= -690.0) ? 1 : 0;
    r.tri = (symmetric && row0 == 0 && r.Tm == r.Tn) ? 1 : 0;
    const int64_t nblk = r.tri ? (int64_t)r.Tm * (r.Tm + 1) / 2 : (int64_t)r.Tm * r.Tn;
    r.grid = (unsigned)nblk;
    const size_t lds = (size_t)2 * RBF_TILE * (size_t)d * sizeof(double);
    if (!rbf_stationary(kind)) {
        // lin / per / CO2 composite: the LDS-staged tile kernel (d <= 32), straight from global memory above that
        if (d <= RBF_LDS_MAXD) { r.kernel = RbfKernel::Lds; r.lds = lds; }
        else r.kernel = RbfKernel::Other;
        return r;
    }
    if (d > RBF_LDS_MAXD) { r.kernel = RbfKernel::Naive; return r; }
    if (!rbf_regs_d(d)) { r.kernel = RbfKernel::Lds; r.lds = lds; return r; }
    r.kernel = RbfKernel::Regs;
    r.D = (int)d;
    // big builds: 4 row tiles per block (b columns loaded once, 4x fewer block launches)
    r.strip = (nblk >= RBF_STRIP_MIN_TILES) ? 4 : 1;
    r.nitems = r.Tn * ((r.Tm + r.strip - 1) / r.strip);
    r.grid = (unsigned)(r.nitems < rbf_blocks ? r.nitems : rbf_blocks);
    return r;
}

}  // namespace gpmi
