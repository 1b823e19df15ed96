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
#include "lap_dev.h"

namespace gpmi {

namespace {

using lapdev::tile_of;

typedef double d4 __attribute__((ext_vector_type(4)));
typedef double d2 __attribute__((ext_vector_type(2)));

constexpr int GK = 16;                         // slab rows per LDS stage
constexpr int GRAM_LDS = 2 * 2 * GK * TILE * 8;   // two stages of two operand strips
constexpr int64_t GRAM_TARGET_GROUPS = 1024;   // workgroups a launch aims at: four per CU of a 256-CU chip
constexpr int64_t DEFAULT_SLAB = 16384;

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

// The launch plan of the Gram kernel, a function of the shapes alone: the slab's rows are cut into nsplit chunks of
// `chunk` rows (a multiple of 128; the last may be shorter) so that tiles x splits reaches GRAM_TARGET_GROUPS where the
// slab has the rows for it.  One lower tile (m <= 128) and a slab of 256 rows already give two splits.
struct GramPlan { int64_t ntiles, nsplit, chunk; };
GramPlan gram_plan(int64_t rows, int64_t mp) {
    const int64_t nt = mp / TILE, units = rows / TILE;
    GramPlan p;
    p.ntiles = nt * (nt + 1) / 2;
    const int64_t want = (GRAM_TARGET_GROUPS + p.ntiles - 1) / p.ntiles;
    int64_t ns = std::min(units, want);
    const int64_t cu = (units + ns - 1) / ns;
    p.nsplit = (units + cu - 1) / cu;
    p.chunk = cu * TILE;
    return p;
}

}  // namespace

int64_t gram_part_doubles(int64_t rows, int64_t mp) {
    const GramPlan p = gram_plan(rows, mp);
    return p.ntiles * p.nsplit * TILE * TILE;
}

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
    const int64_t S = std::min(Np, c->sparse_slab ? round_up(c->sparse_slab, TILE) : DEFAULT_SLAB);
    c->res.drop_fit();
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

    // the last slab is shorter, and a shorter slab can have MORE splits than a full one (the chunk length is rounded)
    const int64_t last_rows = Np % S ? Np % S : S;
    const int64_t part_doubles = std::max(gram_part_doubles(S, mp), gram_part_doubles(last_rows, mp));
    const int64_t gemv_doubles = ((S + 63) / 64) * mp;
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
        hipLaunchKernelGGL(sparse_row_kernel, dim3((unsigned)rows), dim3(256), 0, st, W, ldm, mp, nreal, row0,
                           (const double*)(c->y.as<double>() + row0), method, noise_var, c->sig2, c->sp_q.as<double>() + row0,
                           yt, rpart, rows, bad);
        HIP_TRY(hipGetLastError());
        hipLaunchKernelGGL(sparse_sums_kernel, dim3(1), dim3(256), 0, st, (const double*)rpart, rows, acc);
        HIP_TRY(hipGetLastError());
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
    hipLaunchKernelGGL(sparse_value_kernel, dim3(1), dim3(64), 0, st, (const double*)acc, (const double*)red, (double)N,
                       method, noise_var, rec);
    HIP_TRY(hipGetLastError());
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

}  // namespace gpmi
