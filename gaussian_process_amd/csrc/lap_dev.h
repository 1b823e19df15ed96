// Device helpers shared by the two Laplace classifiers (laplace.hip: binary, softmax.hip: multi-class): the enumeration
// of the lower 128 x 128 tiles, the fixed-order sum of the tile partials of a matrix-vector product, and the fixed-order
// workgroup reduction; and the grid of their one-thread-per-element kernels.
#pragma once
#include "gpmi_ctx.h"

namespace gpmi {
namespace lapdev {

typedef double d2 __attribute__((ext_vector_type(2)));

constexpr int LT = 128;        // tile edge (TILE)
constexpr int SYMV_THREADS = 256;
constexpr int VEC_THREADS = 256;

// workgroups of VEC_THREADS threads that cover n elements
inline unsigned grid_of(int64_t n) { return (unsigned)((n + VEC_THREADS - 1) / VEC_THREADS); }

// lower tile t (row-major enumeration of the lower triangle) -> (I, J), J <= I
__device__ __forceinline__ void tile_of(int64_t t, int64_t& I, int64_t& J) {
    int64_t i = (int64_t)((sqrt(8.0 * (double)t + 1.0) - 1.0) * 0.5);
    while (i * (i + 1) / 2 > t) --i;
    while ((i + 1) * (i + 2) / 2 <= t) ++i;
    I = i;
    J = t - i * (i + 1) / 2;
}

// y_i = sum_b slot (i / 128, b)[i % 128], b in index order
__device__ __forceinline__ double slot_sum(const double* __restrict__ part, int64_t nt, int64_t i) {
    const double* p = part + (i / LT) * nt * LT + (i % LT);
    double acc = 0.0;
    for (int64_t b = 0; b < nt; ++b) acc += p[b * LT];
    return acc;
}

// fixed-order reduction of two values over the workgroup; valid in thread 0
__device__ __forceinline__ void wg_reduce2(double& a, double& b, double* sh) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
        a += __shfl_down(a, off, 64);
        b += __shfl_down(b, off, 64);
    }
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    if (lane == 0) { sh[2 * wave] = a; sh[2 * wave + 1] = b; }
    __syncthreads();
    if (threadIdx.x == 0) {
        double sa = 0., sb = 0.;
        for (int v = 0; v < (int)(blockDim.x >> 6); ++v) { sa += sh[2 * v]; sb += sh[2 * v + 1]; }
        a = sa; b = sb;
    }
}

}  // namespace lapdev
}  // namespace gpmi
