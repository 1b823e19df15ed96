// Sparse GP regression with m inducing inputs Z (VFE: Titsias 2009; FITC: Snelson & Ghahramani 2006; GPML chapter 8) in
// the whitened form, for N far beyond what an N x N covariance allows: O(N m^2) flops, O(m^2 + N d) memory.
//
//   L = chol(K_uu + j I),  A = L^-1 K_uf (m x N),  q_i = |A[:, i]|^2,
//   Lambda_i = s (VFE)  or  s + sigma^2 - q_i (FITC),  A~ = A Lambda^-1/2,  y~ = Lambda^-1/2 y,
//   B = I + A~ A~^T,  L_B = chol(B),  c = L_B^-1 A~ y~
//   value = -N/2 log 2 pi - sum log diag L_B - 1/2 sum log Lambda_i - 1/2 y~^T y~ + 1/2 c^T c
//           [VFE: - sum_i (sigma^2 - q_i) / (2 s)]
//
// The training inputs stay resident; K_uf is never held.  For slabs of S training rows: K(X_slab, Z) is built as S rows
// of m_p columns (rbf.hip), carried through L by the TRSM sweep of driver.hip (row i becomes A[:, i]^T), passed once
// through sparse_row_kernel (q_i, Lambda_i, the scaling, y~_i and the three sums' partials) and accumulated:
// B += V^T V by gram_tn_kernel, g += V^T y~ by the transposed matrix-vector product of solve.hip.  B is factored with g
// riding as the y row, so c falls out of the sweep as m does in regression.
//
// gram_tn_kernel is the one hot kernel: C (128 x 128 tile of the lower triangle) = V[:, I]^T V[:, J] over a chunk of the
// slab's rows.  The contracted index is the row index of a row-major slab, so -- unlike the NT kernels of gemm_nt.hip --
// both MFMA operands are contiguous along the OUTPUT index: lane (fr = lane & 15, fg = lane >> 4) of a
// v_mfma_f64_16x16x4_f64 takes V[k + fg][col + fr] for A and for B alike, which is how the slab lies in memory.  A stage is
// 16 slab rows of the two 128-column strips, copied to LDS as they are (16-byte loads, a wave per 1 KiB row segment) and
// read back with 8-byte reads; odd rows are stored with column bit 4 flipped, so the two rows a half-wave reads fall
// into different halves of the banks.  The split of the slab's rows over workgroups (gram_plan) gives every CU work when
// the lower triangle has few tiles; each workgroup writes its partial tile, and gram_reduce_kernel adds the partials onto
// B in index order: no atomics, the same bits every run.
#include "gpmi_ctx.h"
#include "gpmi_sparse_plan.h"
#include "lap_dev.h"

namespace gpmi {

namespace {

using lapdev::tile_of;

typedef double d4 __attribute__((ext_vector_type(4)));
typedef double d2 __attribute__((ext_vector_type(2)));

constexpr int GK = 16;                         // slab rows per LDS stage
constexpr int GRAM_LDS = 2 * 2 * GK * TILE * 8;   // two stages of two operand strips
static_assert(SPARSE_TILE == TILE, "gpmi_sparse_plan.h plans in the tiles of the kernels");

// fixed-order sum over a workgroup of 256 threads; the result is valid in every thread
__device__ __forceinline__ double wg_sum256(double v, double* sh) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) v += __shfl_down(v, off, 64);
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    __syncthreads();                           // sh may still be read from a previous call
    if (lane == 0) sh[wave] = v;
    __syncthreads();
    return ((sh[0] + sh[1]) + sh[2]) + sh[3];
}

// One workgroup per slab row.  Rows >= nreal (the padding of the last slab) are set to zero.  part: [3][rows] --
// log Lambda_i, y~_i^2, sigma^2 - q_i.  bad: the smallest 1-based training row whose Lambda is not a positive finite
// number (FITC only).
constexpr int ROW_KEEP = 16;                   // 16-byte pieces a thread keeps in registers: rows up to 8192 columns are read once
__global__ __launch_bounds__(256) void sparse_row_kernel(double* __restrict__ W, int64_t ld, int64_t mp, int64_t nreal,
                                                         int64_t row0, const double* __restrict__ y, int method,
                                                         double noise, double sig2, double* __restrict__ q_out,
                                                         double* __restrict__ yt, double* __restrict__ part, int64_t rows,
                                                         unsigned long long* __restrict__ bad) {
    __shared__ double sh[4];
    const int64_t i = blockIdx.x;
    double* row = W + i * ld;
    const int tid = threadIdx.x;
    if (i >= nreal) {
        for (int64_t j = 2 * tid; j < mp; j += 512) *reinterpret_cast<d2*>(row + j) = d2{0.0, 0.0};
        if (tid == 0) { yt[i] = 0.0; part[i] = 0.0; part[rows + i] = 0.0; part[2 * rows + i] = 0.0; }
        return;
    }
    d2 keep[ROW_KEEP];
    double acc = 0.0;
#pragma unroll
    for (int k = 0; k < ROW_KEEP; ++k) {
        const int64_t j = 2 * tid + 512 * k;
        keep[k] = j < mp ? *reinterpret_cast<const d2*>(row + j) : d2{0.0, 0.0};
        acc = fma(keep[k].x, keep[k].x, acc);
        acc = fma(keep[k].y, keep[k].y, acc);
    }
    for (int64_t j = 2 * tid + 512 * ROW_KEEP; j < mp; j += 512) {
        const d2 v = *reinterpret_cast<const d2*>(row + j);
        acc = fma(v.x, v.x, acc);
        acc = fma(v.y, v.y, acc);
    }
    const double q = wg_sum256(acc, sh);
    const double lam = method ? (noise + sig2) - q : noise;
    const double sc = 1.0 / sqrt(lam);
#pragma unroll
    for (int k = 0; k < ROW_KEEP; ++k) {
        const int64_t j = 2 * tid + 512 * k;
        if (j < mp) *reinterpret_cast<d2*>(row + j) = d2{keep[k].x * sc, keep[k].y * sc};
    }
    for (int64_t j = 2 * tid + 512 * ROW_KEEP; j < mp; j += 512) {
        const d2 v = *reinterpret_cast<const d2*>(row + j);
        *reinterpret_cast<d2*>(row + j) = d2{v.x * sc, v.y * sc};
    }
    if (tid == 0) {
        if (!(lam > 0.0) || !isfinite(lam)) atomicMin(bad, (unsigned long long)(row0 + i + 1));
        const double yv = y[i] * sc;
        q_out[i] = q;
        yt[i] = yv;
        part[i] = log(lam);
        part[rows + i] = yv * yv;
        part[2 * rows + i] = sig2 - q;
    }
}

// acc[k] += sum_i part[k][i], k < 3: one workgroup, each thread adds its strided entries in index order
__global__ __launch_bounds__(256) void sparse_sums_kernel(const double* __restrict__ part, int64_t rows,
                                                          double* __restrict__ acc) {
    __shared__ double sh[4];
    for (int k = 0; k < 3; ++k) {
        double v = 0.0;
        for (int64_t i = threadIdx.x; i < rows; i += 256) v += part[k * rows + i];
        const double t = wg_sum256(v, sh);
        if (threadIdx.x == 0) acc[k] += t;
    }
}

// rec[0] = the value, rec[1..6] its terms: N/2 log 2 pi, sum log diag L_B, sum log Lambda, y~^T y~, c^T c, sum (sigma^2 - q)
__global__ void sparse_value_kernel(const double* __restrict__ acc, const double* __restrict__ red, double n, int method,
                                    double noise, double* __restrict__ rec) {
    if (threadIdx.x || blockIdx.x) return;
    const double c0 = 0.5 * n * 1.8378770664093453;       // log(2 pi)
    double v = -c0 - red[0] - 0.5 * acc[0] - 0.5 * acc[1] + 0.5 * red[1];
    if (!method) v -= acc[2] / (2.0 * noise);
    rec[0] = v; rec[1] = c0; rec[2] = red[0]; rec[3] = acc[0]; rec[4] = acc[1]; rec[5] = red[1]; rec[6] = acc[2];
}

// ---- the Gram kernel -------------------------------------------------------------------------------------------------
// grid (lower tiles, splits); workgroup = 4 waves (2 x 2), each a 64 x 64 quarter of the tile = 4 x 4 accumulators.
__global__ __launch_bounds__(256, 2) void gram_tn_kernel(const double* __restrict__ V, int64_t ld, int64_t rows,
                                                         int64_t chunk, double* __restrict__ part) {
    extern __shared__ __attribute__((aligned(16))) char smem_raw[];
    double* smem = reinterpret_cast<double*>(smem_raw);          // [stage][operand][k][128]
    int64_t I, J;
    tile_of(blockIdx.x, I, J);
    const int64_t k0 = (int64_t)blockIdx.y * chunk;
    const int64_t k1 = k0 + chunk < rows ? k0 + chunk : rows;
    const int nst = (int)((k1 - k0) / GK);
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int wr = (wave >> 1) * 64, wc = (wave & 1) * 64;
    const int fr = lane & 15, fg = lane >> 4;
    // staging: thread -> column pair cp of row kr + 4 i, i < 4 (a wave copies one 1 KiB row segment per instruction)
    const int cp = tid & 63, kr = tid >> 6;
    const double* a_src = V + (k0 + kr) * ld + I * TILE + 2 * cp;
    const double* b_src = V + (k0 + kr) * ld + J * TILE + 2 * cp;
    d2 ra[4], rb[4];
    auto load_stage = [&](int st) {
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const int64_t off = ((int64_t)st * GK + 4 * i) * ld;
            ra[i] = *reinterpret_cast<const d2*>(a_src + off);
            rb[i] = *reinterpret_cast<const d2*>(b_src + off);
        }
    };
    auto write_stage = [&](int buf) {
        double* sa = smem + buf * (2 * GK * TILE);
        double* sb = sa + GK * TILE;
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const int k = kr + 4 * i;
            const int col = (2 * cp) ^ ((k & 1) << 4);
            *reinterpret_cast<d2*>(sa + k * TILE + col) = ra[i];
            *reinterpret_cast<d2*>(sb + k * TILE + col) = rb[i];
        }
    };
    d4 acc[4][4];
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int j = 0; j < 4; ++j) acc[i][j] = d4{0., 0., 0., 0.};

    load_stage(0);
    write_stage(0);
    __syncthreads();
    for (int st = 0; st < nst; ++st) {
        const int buf = st & 1;
        load_stage(st + 1 < nst ? st + 1 : st);      // branch-free body: the last step re-loads its own rows
        const double* sa = smem + buf * (2 * GK * TILE);
        const double* sb = sa + GK * TILE;
#pragma unroll
        for (int t = 0; t < GK / 4; ++t) {
            const int k = 4 * t + fg;
            const int sw = (k & 1) << 4;
            double fa[4], fb[4];
#pragma unroll
            for (int i = 0; i < 4; ++i) fa[i] = sa[k * TILE + ((wr + 16 * i + fr) ^ sw)];
#pragma unroll
            for (int j = 0; j < 4; ++j) fb[j] = sb[k * TILE + ((wc + 16 * j + fr) ^ sw)];
#pragma unroll
            for (int i = 0; i < 4; ++i)
#pragma unroll
                for (int j = 0; j < 4; ++j)
                    acc[i][j] = __builtin_amdgcn_mfma_f64_16x16x4f64(fa[i], fb[j], acc[i][j], 0, 0, 0);
        }
        write_stage(buf ^ 1);                        // last read before the previous barrier
        __syncthreads();
    }
    // D layout of v_mfma_f64_16x16x4_f64: col = lane & 15, row = 4 v + (lane >> 4)
    double* P = part + ((int64_t)blockIdx.y * gridDim.x + blockIdx.x) * (TILE * TILE);
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int j = 0; j < 4; ++j)
#pragma unroll
            for (int v = 0; v < 4; ++v) P[(wr + 16 * i + 4 * v + fg) * TILE + wc + 16 * j + fr] = acc[i][j][v];
}

// B tile (I, J) += the partial tiles of the splits, in index order.  grid (lower tiles, 8): a workgroup adds 16 tile rows.
__global__ __launch_bounds__(256) void gram_reduce_kernel(const double* __restrict__ part, int nsplit, double* __restrict__ B,
                                                          int64_t ldb) {
    int64_t I, J;
    tile_of(blockIdx.x, I, J);
    const int64_t tile_sz = TILE * TILE, split_sz = (int64_t)gridDim.x * tile_sz;
    const double* P = part + (int64_t)blockIdx.x * tile_sz;
#pragma unroll
    for (int e = 0; e < 4; ++e) {
        const int idx = blockIdx.y * 1024 + e * 256 + threadIdx.x;      // 16-byte piece of the tile
        const int r = idx >> 6, cpair = idx & 63;
        double* dst = B + (I * TILE + r) * ldb + J * TILE + 2 * cpair;
        d2 v = *reinterpret_cast<const d2*>(dst);
        for (int z = 0; z < nsplit; ++z) {
            const d2 p = *reinterpret_cast<const d2*>(P + z * split_sz + r * TILE + 2 * cpair);
            v.x += p.x; v.y += p.y;
        }
        *reinterpret_cast<d2*>(dst) = v;
    }
}

// The launch plan of the Gram kernel (how many splits, of how many rows each) is gram_plan of gpmi_sparse_plan.h.

// ---- the gradient of the VFE bound -----------------------------------------------------------------------------------
// With u = L_B^-T c, p = L^-T u, T = L^-T (I - B^-1) L^-1 / s, beta = (y - K_fu p) / s and
// D_uu = -1/2 L^-T (B - 2 I + B^-1 + u u^T) L^-1 the derivatives of the bound w.r.t. K_fu and K_uu are
// D_fu = K_fu T + beta p^T and D_uu, and every hyper-parameter and Z reach the bound through the squared distances:
// with G = D o K only  sum G,  sum G (z_ik - z_jk)^2  per dimension k  and  sum_i G_ij (z_ik - z_jk)  per (j, k)  are
// needed.  sparse_contract_kernel forms them for a block of rows (a slab of K_fu with E = W T, or K_uu with E = D_uu and
// beta = 0), reading every element of W and of E once.
//
// grid (ceil(mp / 256), chunks of CT_ROWS rows); a wave owns 64 columns, a lane one column j: z_j, p_j and the 2 DW + 1
// accumulators stay in registers, the chunk's x_i and beta_i are staged in LDS once and read back as broadcasts.  No
// lane ever adds to another lane's sums, so the order of every sum is the row order; the chunks' partials
// (part[chunk][component][column]) are added in chunk order by launch_sum_fixed.  Rows >= nreal are never read;
// columns >= m write zeros.
constexpr int CT_ROWS = 128;
struct ContractArgs {
    const double* W;          // rows x ld: the covariances
    const double* E;          // rows x ld: dF/dK without the beta p^T term
    int64_t ld, nreal;        // leading dimension of both, rows that count
    const double* X;          // the rows' (scaled) inputs, nreal x d
    const double* beta;       // nreal, or null for zero
    const double* p;          // m
    const double* Z;          // the columns' (scaled) inputs, m x d
    int64_t m, mp;
    int d;
    double* part;             // [chunks][2 d + 1][mp]: sum G | sum G diff_k^2 (k < d) | sum G diff_k (k < d)
};
template <int DW>
__global__ __launch_bounds__(256) void sparse_contract_kernel(ContractArgs a) {
    __shared__ double xs[CT_ROWS * DW];
    __shared__ double bs[CT_ROWS];
    const int tid = threadIdx.x, d = a.d;
    const int64_t i0 = (int64_t)blockIdx.y * CT_ROWS;
    const int nrow = (int)(a.nreal - i0 < CT_ROWS ? a.nreal - i0 : CT_ROWS);
    for (int e = tid; e < CT_ROWS * DW; e += 256) {
        const int r = e / DW, k = e % DW;
        xs[e] = (r < nrow && k < d) ? a.X[(i0 + r) * d + k] : 0.0;
    }
    if (tid < CT_ROWS) bs[tid] = (a.beta && tid < nrow) ? a.beta[i0 + tid] : 0.0;
    __syncthreads();
    const int64_t j = (int64_t)blockIdx.x * 256 + tid;
    if (j >= a.mp) return;                                     // a whole wave: mp is a multiple of 128
    const bool real = j < a.m;
    double zj[DW], sq[DW], dz[DW];
#pragma unroll
    for (int k = 0; k < DW; ++k) {
        zj[k] = (real && k < d) ? a.Z[j * d + k] : 0.0;
        sq[k] = 0.0;
        dz[k] = 0.0;
    }
    const double pj = real ? a.p[j] : 0.0;
    double sg = 0.0;
    const double* Wp = a.W + i0 * a.ld + j;
    const double* Ep = a.E + i0 * a.ld + j;
    auto row = [&](int r, double w, double e) {
        const double g = fma(bs[r], pj, e) * w;
        sg += g;
#pragma unroll
        for (int k = 0; k < DW; ++k) {
            const double df = xs[r * DW + k] - zj[k];
            const double t = g * df;
            dz[k] += t;
            sq[k] = fma(t, df, sq[k]);
        }
    };
    int r = 0;
    for (; r + 4 <= nrow; r += 4) {
        double w[4], e[4];
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            w[q] = Wp[(int64_t)(r + q) * a.ld];
            e[q] = Ep[(int64_t)(r + q) * a.ld];
        }
#pragma unroll
        for (int q = 0; q < 4; ++q) row(r + q, w[q], e[q]);
    }
    for (; r < nrow; ++r) row(r, Wp[(int64_t)r * a.ld], Ep[(int64_t)r * a.ld]);
    double* P = a.part + (int64_t)blockIdx.y * (2 * d + 1) * a.mp + j;
    P[0] = real ? sg : 0.0;
#pragma unroll
    for (int k = 0; k < DW; ++k)
        if (k < d) {
            P[(int64_t)(1 + k) * a.mp] = real ? sq[k] : 0.0;
            P[(int64_t)(1 + d + k) * a.mp] = real ? dz[k] : 0.0;
        }
}

// acc (2 d + 1 components x mp columns) += the contraction of one block of rows
hipError_t launch_contract(hipStream_t s, const ContractArgs& a, double* acc) {
    if (a.nreal <= 0 || a.mp <= 0) return hipSuccess;
    if (a.d < 1 || a.d > 32 || a.mp % TILE) return hipErrorInvalidValue;
    const int64_t chunks = (a.nreal + CT_ROWS - 1) / CT_ROWS;
    if (chunks > 65535) return hipErrorInvalidValue;
    const dim3 grid((unsigned)((a.mp + 255) / 256), (unsigned)chunks);
    if (a.d <= 4) hipLaunchKernelGGL(sparse_contract_kernel<4>, grid, dim3(256), 0, s, a);
    else if (a.d <= 8) hipLaunchKernelGGL(sparse_contract_kernel<8>, grid, dim3(256), 0, s, a);
    else if (a.d <= 16) hipLaunchKernelGGL(sparse_contract_kernel<16>, grid, dim3(256), 0, s, a);
    else hipLaunchKernelGGL(sparse_contract_kernel<32>, grid, dim3(256), 0, s, a);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
    const int64_t n = (int64_t)(2 * a.d + 1) * a.mp;
    return launch_sum_fixed(s, a.part, chunks, n, n, acc, 1.0, acc);
}

// dst = the lower triangle of src, zeros above it (what the fused panel kernels leave above a factor's diagonal goes)
__global__ void sparse_tril_kernel(const double* __restrict__ src, double* __restrict__ dst, int64_t ld, int64_t n) {
    const int64_t i = blockIdx.y, j = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (j < n) dst[i * ld + j] = j <= i ? src[i * ld + j] : 0.0;
}

// rec[0] = tr B^-1 = -sum_{i < m} nBinv_ii, rec[1] = sum_{i < N} (sigma^2 - q_i), rec[2] = 0 (beta^T beta gathers there)
__global__ __launch_bounds__(256) void sparse_grad_scalars_kernel(const double* __restrict__ nBinv, int64_t ld, int64_t m,
                                                                  const double* __restrict__ q, int64_t N, double sig2,
                                                                  double* __restrict__ rec) {
    __shared__ double sh[4];
    double v = 0.0;
    for (int64_t i = threadIdx.x; i < m; i += 256) v -= nBinv[i * ld + i];
    const double tr = wg_sum256(v, sh);
    v = 0.0;
    for (int64_t i = threadIdx.x; i < N; i += 256) v += sig2 - q[i];
    const double tq = wg_sum256(v, sh);
    if (threadIdx.x == 0) { rec[0] = tr; rec[1] = tq; rec[2] = 0.0; }
}

// In: nB = -B, nBinv = -B^-1 (what C -= A B^T leaves in a zeroed C).  Out, in place: the cores of D_uu and of -T,
//   nB <- -1/2 (B - 2 I + B^-1 + u u^T),   nBinv <- (B^-1 - I) / s
__global__ void sparse_grad_core_kernel(double* __restrict__ nB, double* __restrict__ nBinv, const double* __restrict__ u,
                                        int64_t ld, int64_t n, double inv_s) {
    const int64_t i = blockIdx.y, j = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (j >= n) return;
    const double b = -nB[i * ld + j], bi = -nBinv[i * ld + j], eye = i == j ? 1.0 : 0.0;
    nB[i * ld + j] = -0.5 * (((b - 2.0 * eye) + bi) + u[i] * u[j]);
    nBinv[i * ld + j] = (bi - eye) * inv_s;
}

// beta_i = (y_i - dot_i) / s for i < nreal, and *sum += sum beta_i^2: one workgroup, index order per thread
__global__ __launch_bounds__(256) void sparse_beta_kernel(const double* __restrict__ y, const double* __restrict__ dot,
                                                          int64_t nreal, double inv_s, double* __restrict__ beta,
                                                          double* __restrict__ sum) {
    __shared__ double sh[4];
    double v = 0.0;
    for (int64_t i = threadIdx.x; i < nreal; i += 256) {
        const double b = (y[i] - dot[i]) * inv_s;
        beta[i] = b;
        v = fma(b, b, v);
    }
    const double t = wg_sum256(v, sh);
    if (threadIdx.x == 0) *sum += t;
}

// rec[0] = sum_j (F + U)[0][j], rec[1 + k] = sum_j (F + U)[1 + k][j], dz[j][k] = F[1 + d + k][j] + 2 U[1 + d + k][j]
// for the column sums F of the K_fu part and U of the K_uu part (the symmetric K_uu moves with z_j through both indices)
__global__ __launch_bounds__(256) void sparse_grad_final_kernel(const double* __restrict__ F, const double* __restrict__ U,
                                                                int64_t m, int64_t mp, int d, double* __restrict__ rec,
                                                                double* __restrict__ dz) {
    __shared__ double sh[4];
    for (int comp = 0; comp <= d; ++comp) {
        double v = 0.0;
        for (int64_t j = threadIdx.x; j < m; j += 256) v += F[comp * mp + j] + U[comp * mp + j];
        const double t = wg_sum256(v, sh);
        if (threadIdx.x == 0) rec[comp] = t;
    }
    for (int64_t e = threadIdx.x; e < m * d; e += 256) {
        const int64_t j = e / d, k = e % d;
        dz[e] = F[(1 + d + k) * mp + j] + 2.0 * U[(1 + d + k) * mp + j];
    }
}

}  // namespace

int64_t gram_part_doubles(int64_t rows, int64_t mp) { return gram_plan_doubles(rows, mp); }

hipError_t launch_gram_tn(hipStream_t s, const double* V, int64_t ldv, int64_t rows, int64_t mp, double* part, double* B,
                          int64_t ldb) {
    if (rows <= 0 || mp <= 0) return hipSuccess;
    if (rows % TILE || mp % TILE || ldv % 2 || ldb % 2) return hipErrorInvalidValue;
    const GramPlan p = gram_plan(rows, mp);
    if (p.ntiles > 0x7fffffff || p.nsplit > 65535) return hipErrorInvalidValue;
    hipLaunchKernelGGL(gram_tn_kernel, dim3((unsigned)p.ntiles, (unsigned)p.nsplit), dim3(256), GRAM_LDS, s, V, ldv, rows,
                       p.chunk, part);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(gram_reduce_kernel, dim3((unsigned)p.ntiles, 8), dim3(256), 0, s, (const double*)part, (int)p.nsplit,
                       B, ldb);
    return hipGetLastError();
}

int sparse_fit_impl(gpmi_ctx* c, const double* Z, int64_t m, double sigma, double ell, double noise_var, double jitter,
                    int method, double* value, int64_t* bad_pivot) {
    if (!c->res.have_train) return fail_arg("gpmi_sparse_fit: no training set (call gpmi_set_train)");
    if (c->kind != 0) return fail_arg("gpmi_sparse_fit: squared-exponential kernel only (gpmi_set_kernel kind 0)");
    if (method != GPMI_SPARSE_VFE && method != GPMI_SPARSE_FITC)
        return fail_arg("gpmi_sparse_fit: method must be GPMI_SPARSE_VFE (0) or GPMI_SPARSE_FITC (1)");
    if (m < 1 || m > c->N) return fail_arg("gpmi_sparse_fit: the number of inducing inputs must be in 1..N");
    if (!(ell != 0.0) || !std::isfinite(ell) || !std::isfinite(sigma))
        return fail_arg("gpmi_sparse_fit: ell must be non-zero and hyper-parameters finite");
    if (!(noise_var > 0.0) || !std::isfinite(noise_var)) return fail_arg("gpmi_sparse_fit: noise_var must be finite and > 0");
    if (!(jitter >= 0.0) || !std::isfinite(jitter)) return fail_arg("gpmi_sparse_fit: jitter must be finite and >= 0");
    hipStream_t st = c->stream;
    const int64_t N = c->N, d = c->d, Np = round_up(N, TILE);
    const int64_t mp = round_up(m, TILE), ldm = mp + c->ld_pad;
    const SparseSlabs slabs = sparse_slabs(N, c->sparse_slab, mp);      // gpmi_sparse_plan.h
    const int64_t S = slabs.S;
    c->res.drop_fit();
    c->spareA.release();               // any fit drops the buffer a removal kept
    c->timers_reset({GPMI_T_SPARSE, GPMI_T_KS, GPMI_T_SOLVE_V, GPMI_T_MEANVAR, GPMI_T_POSTCHOL, GPMI_T_CHOL});
    c->sig2 = sigma * sigma;
    c->coef = -.5 * (1 / (ell * ell));
    c->sigma = sigma; c->ell = ell; c->noise = noise_var;
    c->sp_m = m; c->sp_mp = mp; c->sp_ld = ldm; c->sp_method = method;

    // the inducing inputs, scaled as the test set is
    HIP_TRY(c->sp_Z.ensure((size_t)m * d * 8));
    Box raw;
    raw.assign(Z, m, d);
    if (c->ard()) {
        HIP_TRY(c->sp_Zraw.ensure((size_t)m * d * 8));
        HIP_TRY(hipMemcpyAsync(c->sp_Zraw.p, Z, (size_t)m * d * 8, hipMemcpyHostToDevice, st));
        HIP_TRY(launch_scale_inputs(st, c->sp_Zraw.as<double>(), c->ard_rdev.as<double>(), m, d, c->sp_Z.as<double>()));
        box_scale(raw, c->ard_r, c->boxU);
    } else {
        HIP_TRY(hipMemcpyAsync(c->sp_Z.p, Z, (size_t)m * d * 8, hipMemcpyHostToDevice, st));
        c->boxU = raw;
    }
    HIP_TRY(hipStreamSynchronize(st));           // Z is the caller's buffer
    const double* Zd = c->sp_Z.as<double>();

    // the workspaces of the Gram kernel and of the matrix-vector product are sized for every slab of the fit: the last
    // slab is shorter, and a shorter slab can have MORE splits than a full one
    const int64_t part_doubles = slabs.part_doubles, gemv_doubles = slabs.gemv_doubles;
    // sp_vec: g | the slab's g | y~ | the rows' partials [3][S] | acc[4] | red[4] | rec[8]
    HIP_TRY(c->sp_L.ensure((size_t)mp * ldm * 8));
    HIP_TRY(c->sp_B.ensure((size_t)(mp + TILE) * ldm * 8));
    HIP_TRY(c->sp_W.ensure((size_t)S * ldm * 8));
    c->sp_wrows = S;
    HIP_TRY(c->sp_q.ensure((size_t)Np * 8));
    HIP_TRY(c->sp_vec.ensure((size_t)(2 * mp + 4 * S + 16) * 8));
    HIP_TRY(c->sp_part.ensure((size_t)part_doubles * 8));
    HIP_TRY(c->sp_scr.ensure((size_t)gemv_doubles * 8));
    HIP_TRY(c->sp_info.ensure(32));
    double* Lm = c->sp_L.as<double>();
    double* Bm = c->sp_B.as<double>();
    double* W = c->sp_W.as<double>();
    double* g = c->sp_vec.as<double>();
    double* gs = g + mp;
    double* yt = gs + mp;
    double* rpart = yt + S;
    double* acc = rpart + 3 * S;
    double* red = acc + 4;
    double* rec = red + 4;
    int64_t* info = c->sp_info.as<int64_t>();
    unsigned long long* bad = reinterpret_cast<unsigned long long*>(info + 2);
    const int64_t big = std::numeric_limits<int64_t>::max();
    const int64_t init[3] = {big, big, -1};      // the two pivot words and the row word (all bits set: no bad row)
    HIP_TRY(hipMemcpyAsync(info, init, sizeof init, hipMemcpyHostToDevice, st));

    const size_t sp_all = c->span_begin(GPMI_T_SPARSE);
    // L = chol(K_uu + j I)
    size_t sp = c->span_begin(GPMI_T_CHOL);
    {
        const RbfArgs r = rbf_sym(c, Zd, m, c->boxU, jitter, mp, Lm, ldm);
        HIP_TRY(launch_rbf(st, r));
    }
    HIP_TRY(cholesky_inplace(c, Lm, ldm, mp, mp, info, false));
    c->span_end(sp);
    c->sp_fused = tuning().panel_fused;
    int64_t h_info[3];
    HIP_TRY(hipMemcpyAsync(h_info, info, 8, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    if (h_info[0] != big) {
        c->timers_collect();
        if (bad_pivot) *bad_pivot = h_info[0] + 1;
        if (value) *value = std::numeric_limits<double>::quiet_NaN();
        g_err = "gpmi_sparse_fit: K_uu + jitter I is not positive definite";
        return GPMI_ERR_NOT_PD;
    }

    // B = I, g = 0, the sums = 0
    HIP_TRY(hipMemsetAsync(Bm, 0, (size_t)(mp + TILE) * ldm * 8, st));
    HIP_TRY(launch_set_identity_diag(st, Bm, ldm, mp));
    HIP_TRY(hipMemsetAsync(g, 0, (size_t)mp * 8, st));
    HIP_TRY(hipMemsetAsync(acc, 0, 16 * 8, st));

    for (int64_t row0 = 0; row0 < Np; row0 += S) {
        const int64_t rows = std::min(S, Np - row0), nreal = std::min(rows, N - row0);
        sp = c->span_begin(GPMI_T_KS);
        const RbfArgs r = rbf_cross(c, c->x_train(), N, c->box_train(), Zd, m, c->boxU, row0, rows, mp, W, ldm);   // K(X_slab, Z)
        HIP_TRY(launch_rbf(st, r));
        c->span_end(sp);
        sp = c->span_begin(GPMI_T_SOLVE_V);
        HIP_TRY(solve_sweep_factor(c, Lm, ldm, mp, W, ldm, rows));       // row i <- A[:, i]^T
        c->span_end(sp);
        sp = c->span_begin(GPMI_T_MEANVAR);
        LAUNCH_TRY(sparse_row_kernel, dim3((unsigned)rows), dim3(256), 0, st, W, ldm, mp, nreal, row0,
                   (const double*)(c->y.as<double>() + row0), method, noise_var, c->sig2, c->sp_q.as<double>() + row0,
                   yt, rpart, rows, bad);
        LAUNCH_TRY(sparse_sums_kernel, dim3(1), dim3(256), 0, st, (const double*)rpart, rows, acc);
        HIP_TRY(launch_gemv_t(st, W, ldm, rows, mp, yt, gs, c->sp_scr.as<double>()));
        HIP_TRY(launch_sum_fixed(st, gs, 1, mp, mp, g, 1.0, g));
        c->span_end(sp);
        sp = c->span_begin(GPMI_T_POSTCHOL);
        HIP_TRY(launch_gram_tn(st, W, ldm, rows, mp, c->sp_part.as<double>(), Bm, ldm));
        c->span_end(sp);
    }

    // L_B = chol(B) with g as the y row: c = L_B^-1 g
    sp = c->span_begin(GPMI_T_CHOL);
    double* crow = Bm + mp * ldm;
    HIP_TRY(launch_set_yrow(st, crow, g, m, mp));
    HIP_TRY(cholesky_inplace(c, Bm, ldm, mp, mp + TILE, info + 1, false));
    c->span_end(sp);
    HIP_TRY(launch_lml_reduce(st, Bm, ldm, crow, m, red));
    LAUNCH_TRY(sparse_value_kernel, dim3(1), dim3(64), 0, st, (const double*)acc, (const double*)red, (double)N,
               method, noise_var, rec);
    c->span_end(sp_all);
    double h_rec[8];
    HIP_TRY(hipMemcpyAsync(h_rec, rec, sizeof h_rec, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipMemcpyAsync(h_info, info, sizeof h_info, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    c->timers_collect();
    if (h_info[2] != -1 || h_info[1] != big) {
        // a Lambda_i that is not positive (FITC) comes first: every later number is built on it
        if (bad_pivot) *bad_pivot = h_info[2] != -1 ? h_info[2] : m + 1 + h_info[1];
        if (value) *value = std::numeric_limits<double>::quiet_NaN();
        g_err = h_info[2] != -1 ? "gpmi_sparse_fit: FITC met Lambda_i = noise_var + sigma^2 - q_i that is not positive"
                                : "gpmi_sparse_fit: B = I + A Lambda^-1 A^T met a non-positive pivot";
        return GPMI_ERR_NOT_PD;
    }
    if (bad_pivot) *bad_pivot = 0;
    if (value) *value = h_rec[0];
    c->res.fit_done(Fit::Sparse);
    return GPMI_OK;
}

int sparse_predict_impl(gpmi_ctx* c, double* mu, double* out2, int want_sd) {
    if (!c->res.sparse()) return fail_arg("gpmi_sparse_predict: no sparse fit resident (call gpmi_sparse_fit)");
    if (!c->res.have_test) return fail_arg("gpmi_sparse_predict: no test set (call gpmi_set_test)");
    Tuning tn = c->tune;
    tn.panel_fused = c->sp_fused;          // solve with the kind of leaves that produced the resident factors
    TuneScope tune_scope(&tn);
    hipStream_t st = c->stream;
    const int64_t n = c->n, np_ = c->np_, m = c->sp_m, mp = c->sp_mp, ldm = c->sp_ld;
    const int64_t chunk = std::min(np_, c->sp_wrows);
    c->timers_reset({GPMI_T_KS, GPMI_T_SOLVE_V, GPMI_T_MEANVAR});
    HIP_TRY(c->sp_pred.ensure((size_t)np_ * 3 * 8));
    double* W = c->sp_W.as<double>();
    double* sq1 = c->sp_pred.as<double>();
    double* dot = sq1 + np_;
    double* sq2 = dot + np_;
    const double* Lm = c->sp_L.as<double>();
    const double* Bm = c->sp_B.as<double>();
    const double* cvec = Bm + mp * ldm;
    for (int64_t r0 = 0; r0 < np_; r0 += chunk) {
        const int64_t rows = std::min(chunk, np_ - r0);
        size_t sp = c->span_begin(GPMI_T_KS);
        const RbfArgs r = rbf_cross(c, c->x_test(), n, c->box_test(), c->sp_Z.as<double>(), m, c->boxU, r0, rows, mp, W, ldm);   // K(X*, Z)
        HIP_TRY(launch_rbf(st, r));
        c->span_end(sp);
        sp = c->span_begin(GPMI_T_SOLVE_V);
        HIP_TRY(solve_sweep_factor(c, Lm, ldm, mp, W, ldm, rows));                  // v1^T
        c->span_end(sp);
        sp = c->span_begin(GPMI_T_MEANVAR);
        HIP_TRY(launch_row_dots(st, W, ldm, rows, mp, cvec, nullptr, sq1 + r0));
        c->span_end(sp);
        sp = c->span_begin(GPMI_T_SOLVE_V);
        HIP_TRY(solve_sweep_factor(c, Bm, ldm, mp, W, ldm, rows));                  // v2^T
        c->span_end(sp);
        sp = c->span_begin(GPMI_T_MEANVAR);
        HIP_TRY(launch_row_dots(st, W, ldm, rows, mp, cvec, dot + r0, sq2 + r0));
        c->span_end(sp);
    }
    std::vector<double> h(3 * (size_t)np_);
    HIP_TRY(hipMemcpyAsync(h.data(), sq1, h.size() * 8, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    c->timers_collect();
    for (int64_t i = 0; i < n; ++i) {
        if (mu) mu[i] = h[np_ + i];
        if (out2) {
            const double var = (c->sig2 - h[i]) + h[2 * np_ + i];
            out2[i] = want_sd ? std::sqrt(var) : var;      // sqrt(< 0) -> NaN, as gpmi_predict_resident
        }
    }
    return GPMI_OK;
}

int sparse_get_impl(gpmi_ctx* c, double* c_out, double* q_out) {
    if (!c->res.sparse()) return fail_arg("gpmi_sparse_get: no sparse fit resident (call gpmi_sparse_fit)");
    hipStream_t st = c->stream;
    if (c_out)
        HIP_TRY(hipMemcpyAsync(c_out, c->sp_B.as<double>() + c->sp_mp * c->sp_ld, (size_t)c->sp_m * 8, hipMemcpyDeviceToHost, st));
    if (q_out) HIP_TRY(hipMemcpyAsync(q_out, c->sp_q.p, (size_t)c->N * 8, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    return GPMI_OK;
}

// The gradient of the VFE bound at the resident fit (include/gpmi.h: gpmi_sparse_grad).  The m-sized part runs on three
// m_p x ld workspaces G0, G1, G2 and the slab-sized E; every product is C -= A B^T into a zeroed C on the routed GEMM,
// so a chain of two products carries no sign.  Nothing of the fit is written: sp_W is a workspace already.
int sparse_grad_impl(gpmi_ctx* c, double* d_ell, double* d_sigma, double* d_noise, double* d_r, double* d_Z) {
    if (!c->res.sparse()) return fail_arg("gpmi_sparse_grad: no sparse fit resident (call gpmi_sparse_fit)");
    if (c->sp_method != GPMI_SPARSE_VFE)
        return fail_arg("gpmi_sparse_grad: the resident fit is FITC; only the gradient of the VFE bound is implemented");
    if (c->d > 32) return fail_arg("gpmi_sparse_grad: at most 32 input dimensions");
    Tuning tn = c->tune;
    tn.panel_fused = c->sp_fused;          // solve with the kind of leaves that produced the resident factors
    TuneScope tune_scope(&tn);
    hipStream_t st = c->stream;
    const int64_t N = c->N, Np = round_up(N, TILE), m = c->sp_m, mp = c->sp_mp, ldm = c->sp_ld, S = c->sp_wrows;
    const int d = (int)c->d, ncomp = 2 * d + 1;
    const double s = c->noise, inv_s = 1.0 / s;
    const int64_t erows = std::max(S, mp), chunks = (erows + CT_ROWS - 1) / CT_ROWS, ncol = (int64_t)ncomp * mp;
    const size_t mat = (size_t)mp * ldm * 8;
    HIP_TRY(c->sp_g0.ensure(mat));
    HIP_TRY(c->sp_g1.ensure(mat));
    HIP_TRY(c->sp_g2.ensure(mat));
    HIP_TRY(c->sp_gE.ensure((size_t)erows * ldm * 8));
    HIP_TRY(c->sp_gpart.ensure((size_t)(chunks * ncol) * 8));
    // sp_gvec: u | p | the slab's W p | beta | the column sums of the K_fu part | of the K_uu part | rec | dz
    const int64_t nrec = round_up(d + 4, 2);
    HIP_TRY(c->sp_gvec.ensure((size_t)(2 * mp + 2 * S + 2 * ncol + nrec + m * d) * 8));
    double* G0 = c->sp_g0.as<double>();
    double* G1 = c->sp_g1.as<double>();
    double* G2 = c->sp_g2.as<double>();
    double* E = c->sp_gE.as<double>();
    double* part = c->sp_gpart.as<double>();
    double* u = c->sp_gvec.as<double>();
    double* p = u + mp;
    double* dot = p + mp;
    double* beta = dot + S;
    double* colF = beta + S;
    double* colU = colF + ncol;
    double* rec = colU + ncol;
    double* dz = rec + nrec;
    double* W = c->sp_W.as<double>();
    const double* Lm = c->sp_L.as<double>();
    const double* Bm = c->sp_B.as<double>();
    const double* cvec = Bm + mp * ldm;
    const double* Zd = c->sp_Z.as<double>();
    const dim3 egrid((unsigned)((mp + 255) / 256), (unsigned)mp);

    // C (rows x mp) = -A B^T over K = mp
    auto neg_product = [&](double* C, const double* A, const double* B, int64_t rows) -> hipError_t {
        hipError_t e = hipMemsetAsync(C, 0, (size_t)rows * ldm * 8, st);
        if (e != hipSuccess) return e;
        return launch_gemm_nt(st, gemm_minus(C, ldm, A, ldm, B, ldm, rows, mp, mp));
    };

    c->timers_reset({GPMI_T_SPARSE, GPMI_T_KS, GPMI_T_SOLVE_V, GPMI_T_MEANVAR, GPMI_T_POSTCHOL, GPMI_T_CHOL});
    const size_t sp_all = c->span_begin(GPMI_T_SPARSE);
    // ---- the m-sized part: GPMI_T_CHOL
    size_t sp = c->span_begin(GPMI_T_CHOL);
    HIP_TRY(hipMemsetAsync(colF, 0, (size_t)(2 * ncol) * 8, st));
    HIP_TRY(inverse_transposed(c, Bm, ldm, mp, G0, ldm));                                            // G0 = L_B^-T
    HIP_TRY(launch_row_dots(st, G0, ldm, mp, mp, cvec, u, nullptr));       // u = L_B^-T c
    HIP_TRY(neg_product(G1, G0, G0, mp));                                  // G1 = -B^-1
    LAUNCH_TRY(sparse_grad_scalars_kernel, dim3(1), dim3(256), 0, st, (const double*)G1, ldm, m,
               (const double*)c->sp_q.as<double>(), N, c->sig2, rec);
    LAUNCH_TRY(sparse_tril_kernel, egrid, dim3(256), 0, st, Bm, G0, ldm, mp);      // G0 = L_B
    HIP_TRY(neg_product(G2, G0, G0, mp));                                  // G2 = -B
    LAUNCH_TRY(sparse_grad_core_kernel, egrid, dim3(256), 0, st, G2, G1, (const double*)u, ldm, mp, inv_s);
    HIP_TRY(inverse_transposed(c, Lm, ldm, mp, G0, ldm));                                            // G0 = L^-T
    HIP_TRY(launch_row_dots(st, G0, ldm, mp, mp, u, p, nullptr));          // p = L^-T u
    HIP_TRY(neg_product(E, G0, G1, mp));
    HIP_TRY(neg_product(G1, E, G0, mp));                                   // G1 = -T
    HIP_TRY(neg_product(E, G0, G2, mp));
    HIP_TRY(neg_product(G2, E, G0, mp));                                   // G2 = D_uu
    c->span_end(sp);

    ContractArgs ca;
    ca.ld = ldm; ca.p = p; ca.Z = Zd; ca.m = m; ca.mp = mp; ca.d = d; ca.part = part;
    // ---- the K_uu part: W = K(Z, Z) without the jitter, E = D_uu, beta = 0
    sp = c->span_begin(GPMI_T_KS);
    {
        const RbfArgs r = rbf_cross(c, Zd, m, c->boxU, Zd, m, c->boxU, 0, mp, mp, G0, ldm);
        HIP_TRY(launch_rbf(st, r));
    }
    c->span_end(sp);
    sp = c->span_begin(GPMI_T_MEANVAR);
    ca.W = G0; ca.E = G2; ca.nreal = m; ca.X = Zd; ca.beta = nullptr;
    HIP_TRY(launch_contract(st, ca, colU));
    c->span_end(sp);

    // ---- the K_fu part, slab by slab
    for (int64_t row0 = 0; row0 < Np; row0 += S) {
        const int64_t rows = std::min(S, Np - row0), nreal = std::min(rows, N - row0);
        sp = c->span_begin(GPMI_T_KS);
        const RbfArgs r = rbf_cross(c, c->x_train(), N, c->box_train(), Zd, m, c->boxU, row0, rows, mp, W, ldm);   // K(X_slab, Z)
        HIP_TRY(launch_rbf(st, r));
        c->span_end(sp);
        sp = c->span_begin(GPMI_T_SOLVE_V);
        HIP_TRY(launch_row_dots(st, W, ldm, nreal, mp, p, dot, nullptr));
        LAUNCH_TRY(sparse_beta_kernel, dim3(1), dim3(256), 0, st, (const double*)(c->y.as<double>() + row0),
                   (const double*)dot, nreal, inv_s, beta, rec + 2);
        c->span_end(sp);
        sp = c->span_begin(GPMI_T_POSTCHOL);
        HIP_TRY(neg_product(E, W, G1, rows));                              // E = W T
        c->span_end(sp);
        sp = c->span_begin(GPMI_T_MEANVAR);
        ca.W = W; ca.E = E; ca.nreal = nreal; ca.X = c->x_train() + row0 * d; ca.beta = beta;
        HIP_TRY(launch_contract(st, ca, colF));
        c->span_end(sp);
    }
    LAUNCH_TRY(sparse_grad_final_kernel, dim3(1), dim3(256), 0, st, (const double*)colF, (const double*)colU, m, mp,
               d, rec + 3, dz);
    c->span_end(sp_all);
    std::vector<double> h((size_t)(nrec + m * d));
    HIP_TRY(hipMemcpyAsync(h.data(), rec, (d_Z ? h.size() : (size_t)nrec) * 8, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    c->timers_collect();

    const double sigma = c->sigma, l = c->ell, l2 = l * l;
    const double sum_g = h[3];
    double sum_sq = 0.0;
    for (int k = 0; k < d; ++k) sum_sq += h[4 + k];
    if (d_ell) *d_ell = sum_sq / (l2 * l);
    if (d_sigma) *d_sigma = (2.0 / sigma) * sum_g - (double)N * sigma / s;
    if (d_noise) *d_noise = -((double)(N - m) + h[0]) / (2.0 * s) + 0.5 * h[2] + h[1] / (2.0 * s * s);
    for (int k = 0; k < d; ++k) {
        const double rk = c->ard() ? c->ard_r[(size_t)k] : 1.0;
        if (d_r) d_r[k] = h[4 + k] / (l2 * rk);
        if (d_Z)
            for (int64_t j = 0; j < m; ++j) d_Z[j * d + k] = h[(size_t)(nrec + j * d + k)] / (l2 * rk);
    }
    return GPMI_OK;
}

}  // namespace gpmi
