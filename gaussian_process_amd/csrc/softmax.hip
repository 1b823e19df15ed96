// Multi-class GP classification by the Laplace approximation (Rasmussen & Williams, GPML, Algorithms 3.3 and 3.4, softmax
// likelihood, labels 0 .. C-1, one latent function per class, all with the same squared-exponential prior): the
// memory-bound kernels around the existing hot path and the Newton driver.
//
// Per Newton step the O(N^3) work is C x [Cholesky of B_c = I + s_c s_c^T o K, the triangular sweep V_c = S_c L_c^-T,
// the lower NT GEMM V_c V_c^T = E_c] and the Cholesky of sum_c E_c, all by the drivers of driver.hip.  K is built once
// per fit and kept (the C factorisations of a step all start from it).  What is new here:
//   softmax_symv_kernel<NV>  one matrix times up to C vectors over its lower tiles: F = A K and K B in ONE read of K's
//                            lower triangle from memory (NV vectors per pass over a tile, the tile's later passes come
//                            from cache), and E_c x_c for all classes in one launch (one matrix per blockIdx.y)
//   softmax_bmat_kernel      A <- I + s_c s_c^T o K on the lower tiles, from the kept K
//   softmax_newton_kernel    per point: F from the tile partials (or the halved step), P, sqrt(P), Y - P,
//                            B = P o F - P o sum_c(P o F) + Y - P and the partials of Psi (max-subtracted logsumexp)
//   (newton_psi_kernel of laplace.hip: Psi in a fixed order with the Cholesky's pivot word and the solve's give-up word)
//   softmax_vec_kernel       C vectors from the tile partials (K b_c; c_c = E_c K b_c and sum_c c_c)
//   softmax_esum_kernel      A <- sum_c E_c on the lower tiles (identity on the padding)
//   softmax_update_kernel    A <- B - C + [E_c t]_c (keeping the previous A, F for step halving)
//   (launch_mirror_lower of grad.hip: lower triangle of every E_c -> its upper triangle, prediction multiplies by the
//   full matrix; the gradient mirrors K the same way)
//   softmax_rowdot_kernel    prediction: mu* = R (Y - P)^T and B_c[i] . R[i]
//   softmax_gram_kernel      prediction: Sigma[i] = [U_c[:, i] . U_c'[:, i]] + diag(sigma^2 - B_c[i] . R[i])
//   softmax_sample_kernel    prediction: C x C Cholesky per test point and the mean of softmax(mu* + chol(Sigma) z_s)
//   softmax_s2_kernel        gradient: per training point, s2 from its C x C posterior covariance and P
//   softmax_z_kernel         gradient: z_c = s2_c - v_c + E_c t from the tile partials
//   softmax_weight_kernel    gradient: Wm = -sum_c E_c + Gamma + sum_c (g_c g_c^T + z_c g_c^T + g_c z_c^T) on the lower tiles
// The GEMM that forms V V^T subtracts (the fast route of gemm_nt): the buffers hold -E_c, and every consumer here takes
// the sign back.  Every reduction runs in a fixed order (no atomics), so two fits give the same bits.
// Host side: the fit is a problem object (SoftmaxNewton) for newton_iterate of gpmi_state.h, with the skeleton of
// laplace.hip; the gradient ends in regress.hip's ARD trace ending, which reads the backward solve's give-up word here.
#include "gpmi_ctx.h"
#include "lap_dev.h"

namespace gpmi {

namespace {

using namespace lapdev;

constexpr int MAXC = GPMI_SOFTMAX_MAX_CLASSES;

struct SymvArgs {
    const double* M;           // matrix m at M + m * mstride, leading dimension ld, nt x nt tiles (lower ones are read)
    int64_t mstride, ld, nt;
    const double* x;           // vector v of matrix m at x + m * xstride + v * nt * 128
    int64_t xstride;
    int nvec;                  // vectors per matrix
    double* part;              // tile partials of (m, v) at part + (m * nvec + v) * nt * nt * 128
};

// The multi-vector form of laplace_symv_kernel<false>: one workgroup per lower tile (I, J), the same lane layout
// (lane (g, q) of wave w reads row 32 * step + 8 * w + g at columns 16 k + 2 q (+1): every 16-byte load of a wave covers
// one whole 128-byte line of eight rows), the same slots: slot (I, J) <- K_IJ x_J, slot (J, I) <- K_IJ^T x_I, the diagonal
// tile puts both halves of its lower triangle into slot (I, I).  The vectors' tile segments sit in LDS; the column
// accumulators (16 per vector and lane) bound NV.
template <int NV>
__global__ __launch_bounds__(SYMV_THREADS) void softmax_symv_kernel(SymvArgs p) {
    __shared__ __attribute__((aligned(16))) double xs[2][NV][LT];      // [0]: x_J, [1]: x_I
    __shared__ double rowsum[NV][LT];
    __shared__ double colsum[SYMV_THREADS / 64][NV][LT];
    int64_t I, J;
    tile_of(blockIdx.x, I, J);
    const bool diag = I == J;
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6, g = lane >> 3, q = lane & 7;
    const int64_t m = blockIdx.y, Np = p.nt * LT, pstride = p.nt * p.nt * LT;
    const double* T = p.M + m * p.mstride + I * LT * p.ld + J * LT;
    const double* xm = p.x + m * p.xstride;
    double* pm = p.part + m * p.nvec * pstride;
    for (int v0 = 0; v0 < p.nvec; v0 += NV) {
        for (int e = threadIdx.x; e < 2 * NV * LT; e += SYMV_THREADS) {
            const int which = e / (NV * LT), j = (e / LT) % NV, t = e % LT;
            xs[which][j][t] = v0 + j < p.nvec ? xm[(int64_t)(v0 + j) * Np + (which ? I : J) * LT + t] : 0.0;
        }
        __syncthreads();
        double cacc[NV][16];
#pragma unroll
        for (int j = 0; j < NV; ++j)
#pragma unroll
            for (int k = 0; k < 16; ++k) cacc[j][k] = 0.0;
#pragma unroll 1
        for (int st = 0; st < 4; ++st) {
            const int r = 32 * st + 8 * w + g;
            d2 kv[8];
#pragma unroll
            for (int k = 0; k < 8; ++k) kv[k] = *reinterpret_cast<const d2*>(T + (int64_t)r * p.ld + 16 * k + 2 * q);
            if (diag) {                                   // lower triangle only
#pragma unroll
                for (int k = 0; k < 8; ++k) {
                    const int c0 = 16 * k + 2 * q;
                    if (c0 > r) kv[k].x = 0.0;
                    if (c0 + 1 > r) kv[k].y = 0.0;
                }
            }
#pragma unroll
            for (int j = 0; j < NV; ++j) {
                const double xr = xs[1][j][r];
                double rp = 0.0;
#pragma unroll
                for (int k = 0; k < 8; ++k) {
                    const int c0 = 16 * k + 2 * q;
                    const d2 xv = *reinterpret_cast<const d2*>(&xs[0][j][c0]);
                    rp = fma(kv[k].x, xv.x, rp);
                    rp = fma(kv[k].y, xv.y, rp);
                    // column part: the diagonal tile's diagonal belongs to the row part
                    cacc[j][2 * k] = fma((diag && c0 == r) ? 0.0 : kv[k].x, xr, cacc[j][2 * k]);
                    cacc[j][2 * k + 1] = fma((diag && c0 + 1 == r) ? 0.0 : kv[k].y, xr, cacc[j][2 * k + 1]);
                }
                rp += __shfl_xor(rp, 1, 64);
                rp += __shfl_xor(rp, 2, 64);
                rp += __shfl_xor(rp, 4, 64);
                if (q == 0) rowsum[j][r] = rp;
            }
        }
        // column part: sum over the eight row groups of the wave, then over the four waves (fixed order)
#pragma unroll
        for (int j = 0; j < NV; ++j) {
#pragma unroll
            for (int k = 0; k < 16; ++k) {
                double v = cacc[j][k];
                v += __shfl_xor(v, 8, 64);
                v += __shfl_xor(v, 16, 64);
                v += __shfl_xor(v, 32, 64);
                cacc[j][k] = v;
            }
            if (g == 0) {
#pragma unroll
                for (int k = 0; k < 8; ++k) {
                    colsum[w][j][16 * k + 2 * q] = cacc[j][2 * k];
                    colsum[w][j][16 * k + 2 * q + 1] = cacc[j][2 * k + 1];
                }
            }
        }
        __syncthreads();
        for (int e = threadIdx.x; e < NV * LT; e += SYMV_THREADS) {
            const int j = e / LT, t = e % LT;
            if (v0 + j >= p.nvec) continue;
            double* pv = pm + (int64_t)(v0 + j) * pstride;
            const double cs = ((colsum[0][j][t] + colsum[1][j][t]) + colsum[2][j][t]) + colsum[3][j][t];
            if (diag) {
                pv[(I * p.nt + I) * LT + t] = rowsum[j][t] + cs;
            } else {
                pv[(I * p.nt + J) * LT + t] = rowsum[j][t];
                pv[(J * p.nt + I) * LT + t] = cs;
            }
        }
        __syncthreads();
    }
}

// One workgroup per lower tile: out = I + s s^T o K (real rows and columns only, the padding becomes exactly the
// identity).  Diagonal tiles are written whole, from K's lower triangle.
__global__ __launch_bounds__(VEC_THREADS) void softmax_bmat_kernel(const double* __restrict__ K, double* __restrict__ out,
                                                                   int64_t ld, int64_t N, const double* __restrict__ s) {
    int64_t I, J;
    tile_of(blockIdx.x, I, J);
    const bool diag = I == J;
    for (int e = threadIdx.x; e < LT * LT / 2; e += VEC_THREADS) {
        const int r = e / (LT / 2), c0 = 2 * (e % (LT / 2));
        const int64_t gi = I * LT + r, gj = J * LT + c0;
        double k0, k1;
        if (!diag) {
            const d2 kv = *reinterpret_cast<const d2*>(K + gi * ld + gj);
            k0 = kv.x; k1 = kv.y;
        } else {
            k0 = c0 <= r ? K[gi * ld + gj] : K[gj * ld + gi];
            k1 = c0 + 1 <= r ? K[gi * ld + gj + 1] : K[(gj + 1) * ld + gi];
        }
        const double si = s[gi];
        double b0 = (gi < N && gj < N) ? (si * s[gj]) * k0 : 0.0;
        double b1 = (gi < N && gj + 1 < N) ? (si * s[gj + 1]) * k1 : 0.0;
        if (gi == gj) b0 = 1.0 + b0;
        if (gi == gj + 1) b1 = 1.0 + b1;
        *reinterpret_cast<d2*>(out + gi * ld + gj) = d2{b0, b1};
    }
}

// One workgroup per lower tile: out = sum_c E_c = -(sum_c nE_c), classes in index order; 1 on the padded diagonal.
// Diagonal tiles are written whole, from the lower triangles.
__global__ __launch_bounds__(VEC_THREADS) void softmax_esum_kernel(const double* __restrict__ nE, int64_t estride, int C,
                                                                   double* __restrict__ out, int64_t ld, int64_t N) {
    int64_t I, J;
    tile_of(blockIdx.x, I, J);
    const bool diag = I == J;
    for (int e = threadIdx.x; e < LT * LT / 2; e += VEC_THREADS) {
        const int r = e / (LT / 2), c0 = 2 * (e % (LT / 2));
        const int64_t gi = I * LT + r, gj = J * LT + c0;
        const int64_t o0 = (!diag || c0 <= r) ? gi * ld + gj : gj * ld + gi;
        const int64_t o1 = (!diag || c0 + 1 <= r) ? gi * ld + gj + 1 : (gj + 1) * ld + gi;
        double a0 = 0.0, a1 = 0.0;
        for (int c = 0; c < C; ++c) {
            a0 += nE[c * estride + o0];
            a1 += nE[c * estride + o1];
        }
        a0 = -a0; a1 = -a1;
        if (gi == gj && gi >= N) a0 = 1.0;
        if (gi == gj + 1 && gi >= N) a1 = 1.0;
        *reinterpret_cast<d2*>(out + gi * ld + gj) = d2{a0, a1};
    }
}

struct SoftVecs {          // each C x Np, class-major
    double *a, *a_prev, *f, *f_prev, *s, *g, *b;
};

// One thread per point.  mode 0: F = A K from the tile partials; mode 1: the halved step, A <- (A + A_prev) / 2,
// F <- (F + F_prev) / 2.  Then P = softmax over the classes, s = sqrt(P), g = Y - P, B = P o F - P o sum_c(P o F) + Y - P;
// entries past N are 0.  psi_part[2 blk] = sum A o F, psi_part[2 blk + 1] = sum_i (F[label_i, i] - logsumexp_c F_ci).
__global__ __launch_bounds__(VEC_THREADS) void softmax_newton_kernel(int mode, const double* __restrict__ part, int64_t nt,
                                                                     int64_t N, int64_t Np, int C,
                                                                     const double* __restrict__ y, SoftVecs v,
                                                                     double* __restrict__ psi_part) {
    __shared__ double sh[2 * (VEC_THREADS / 64)];
    const int64_t i = (int64_t)blockIdx.x * VEC_THREADS + threadIdx.x;
    const int64_t pstride = nt * nt * LT;
    double af = 0.0, lp = 0.0;
    if (i < Np) {
        double f[MAXC], pr[MAXC];
        double fmx = -INFINITY;
#pragma unroll
        for (int c = 0; c < MAXC; ++c) {
            f[c] = 0.0; pr[c] = 0.0;
            if (c < C) {
                const int64_t o = c * Np + i;
                double a;
                if (mode == 0) {
                    a = v.a[o];
                    f[c] = i < N ? slot_sum(part + c * pstride, nt, i) : 0.0;
                } else {
                    a = (v.a[o] + v.a_prev[o]) / 2;
                    f[c] = (v.f[o] + v.f_prev[o]) / 2;
                    v.a[o] = a;
                }
                v.f[o] = f[c];
                if (i < N) af = fma(a, f[c], af);
                fmx = fmax(fmx, f[c]);
            }
        }
        if (i < N) {
            const int lab = (int)y[i];
            double se = 0.0, spf = 0.0, flab = 0.0;
#pragma unroll
            for (int c = 0; c < MAXC; ++c)
                if (c < C) { pr[c] = exp(f[c] - fmx); se += pr[c]; }
#pragma unroll
            for (int c = 0; c < MAXC; ++c)
                if (c < C) {
                    pr[c] = pr[c] / se;
                    spf += pr[c] * f[c];
                    if (c == lab) flab = f[c];
                }
            lp = flab - (fmx + log(se));
#pragma unroll
            for (int c = 0; c < MAXC; ++c)
                if (c < C) {
                    const int64_t o = c * Np + i;
                    const double yc = c == lab ? 1.0 : 0.0;
                    v.s[o] = sqrt(pr[c]);
                    v.g[o] = yc - pr[c];
                    v.b[o] = ((pr[c] * f[c] - pr[c] * spf) + yc) - pr[c];
                }
        } else {
            for (int c = 0; c < C; ++c) {
                const int64_t o = c * Np + i;
                v.s[o] = 0.0; v.g[o] = 0.0; v.b[o] = 0.0;
            }
        }
    }
    wg_reduce2(af, lp, sh);
    if (threadIdx.x == 0) { psi_part[2 * blockIdx.x] = af; psi_part[2 * blockIdx.x + 1] = lp; }
}

// out_c[i] = sign * (tile partials of vector c summed), 0 past N; total (optional) = sum_c out_c[i] in index order
__global__ __launch_bounds__(VEC_THREADS) void softmax_vec_kernel(const double* __restrict__ part, int64_t nt, int64_t N,
                                                                  int64_t Np, int C, double sign, double* __restrict__ out,
                                                                  double* __restrict__ total) {
    const int64_t i = (int64_t)blockIdx.x * VEC_THREADS + threadIdx.x;
    if (i >= Np) return;
    const int64_t pstride = nt * nt * LT;
    double t = 0.0;
    for (int c = 0; c < C; ++c) {
        const double val = i < N ? sign * slot_sum(part + c * pstride, nt, i) : 0.0;
        out[c * Np + i] = val;
        t += val;
    }
    if (total) total[i] = t;
}

// A_prev <- A, F_prev <- F, A_c <- B_c - C_c + E_c t  (the partials hold -E_c t)
__global__ __launch_bounds__(VEC_THREADS) void softmax_update_kernel(const double* __restrict__ part, int64_t nt, int64_t N,
                                                                     int64_t Np, int C, const double* __restrict__ cc,
                                                                     SoftVecs v) {
    const int64_t i = (int64_t)blockIdx.x * VEC_THREADS + threadIdx.x;
    if (i >= Np) return;
    const int64_t pstride = nt * nt * LT;
    for (int c = 0; c < C; ++c) {
        const int64_t o = c * Np + i;
        v.a_prev[o] = v.a[o];
        v.f_prev[o] = v.f[o];
        v.a[o] = i < N ? (v.b[o] - cc[o]) - slot_sum(part + c * pstride, nt, i) : 0.0;
    }
}

// V[i][i] = s[i]
__global__ __launch_bounds__(VEC_THREADS) void softmax_seed_kernel(double* __restrict__ V, int64_t ld, int64_t Np,
                                                                   const double* __restrict__ s) {
    const int64_t i = (int64_t)blockIdx.x * VEC_THREADS + threadIdx.x;
    if (i < Np) V[i * ld + i] = s[i];
}

// One workgroup per row i of R: out[i * C + c] = sum_j R[i][j] Z_c[i][j] in a fixed order, Z_c[i] = Z + c * zc + i * zr
__global__ __launch_bounds__(VEC_THREADS) void softmax_rowdot_kernel(const double* __restrict__ R, int64_t ld, int64_t ncols,
                                                                     const double* __restrict__ Z, int64_t zc, int64_t zr,
                                                                     int C, double* __restrict__ out) {
    __shared__ double sh[2 * (VEC_THREADS / 64)];
    const int64_t i = blockIdx.x;
    const double* Rr = R + i * ld;
    for (int c = 0; c < C; ++c) {
        const double* z = Z + c * zc + i * zr;
        double acc = 0.0, unused = 0.0;
        for (int64_t j = 2 * threadIdx.x; j < ncols; j += 2 * VEC_THREADS) {
            const d2 r = *reinterpret_cast<const d2*>(Rr + j);
            const d2 zv = *reinterpret_cast<const d2*>(z + j);
            acc = fma(r.x, zv.x, acc);
            acc = fma(r.y, zv.y, acc);
        }
        wg_reduce2(acc, unused, sh);
        if (threadIdx.x == 0) out[i * C + c] = acc;
        __syncthreads();
    }
}

// One workgroup per test point i: cov[i][c][e] = U_c[i] . U_e[i] (row c * np + i of U), + sig2 - dd[i][c] where c == e
__global__ __launch_bounds__(VEC_THREADS) void softmax_gram_kernel(const double* __restrict__ U, int64_t ld, int64_t np,
                                                                   int64_t ncols, int C, double sig2,
                                                                   const double* __restrict__ dd, double* __restrict__ cov) {
    __shared__ double sh[2 * (VEC_THREADS / 64)];
    const int64_t i = blockIdx.x;
    for (int c = 0; c < C; ++c)
        for (int e = 0; e <= c; ++e) {
            const double* uc = U + (c * np + i) * ld;
            const double* ue = U + (e * np + i) * ld;
            double acc = 0.0, unused = 0.0;
            for (int64_t j = 2 * threadIdx.x; j < ncols; j += 2 * VEC_THREADS) {
                const d2 a = *reinterpret_cast<const d2*>(uc + j);
                const d2 b = *reinterpret_cast<const d2*>(ue + j);
                acc = fma(a.x, b.x, acc);
                acc = fma(a.y, b.y, acc);
            }
            wg_reduce2(acc, unused, sh);
            if (threadIdx.x == 0) {
                if (c == e) acc += sig2 - dd[i * C + c];
                cov[(i * C + c) * C + e] = acc;
                cov[(i * C + e) * C + c] = acc;
            }
            __syncthreads();
        }
}

// One workgroup per test point: L = chol(cov[i]) (a pivot <= 0 becomes 0 with its column), then
// prob[i][c] = (1 / S) sum_s softmax(mu[i] + L z_s)_c: every thread sums its samples s = t, t + 256, ..., the 256 partial
// sums are added in thread order
__global__ __launch_bounds__(VEC_THREADS) void softmax_sample_kernel(int C, int64_t S, const double* __restrict__ mu,
                                                                     const double* __restrict__ cov,
                                                                     const double* __restrict__ z, double* __restrict__ prob) {
    __shared__ double L[MAXC][MAXC];
    __shared__ double m[MAXC];
    __shared__ double partial[VEC_THREADS][MAXC];
    const int64_t i = blockIdx.x;
    if (threadIdx.x == 0) {
        const double* Sg = cov + i * C * C;
        for (int r = 0; r < C; ++r) {
            m[r] = mu[i * C + r];
            for (int k = 0; k < C; ++k) L[r][k] = 0.0;
        }
        for (int j = 0; j < C; ++j) {
            double dj = Sg[j * C + j];
            for (int k = 0; k < j; ++k) dj -= L[j][k] * L[j][k];
            if (!(dj > 0.0)) continue;                       // the column stays 0
            const double piv = sqrt(dj);
            L[j][j] = piv;
            for (int r = j + 1; r < C; ++r) {
                double t = Sg[r * C + j];
                for (int k = 0; k < j; ++k) t -= L[r][k] * L[j][k];
                L[r][j] = t / piv;
            }
        }
    }
    __syncthreads();
    double acc[MAXC], gv[MAXC];
#pragma unroll
    for (int c = 0; c < MAXC; ++c) acc[c] = 0.0;
    for (int64_t s = threadIdx.x; s < S; s += VEC_THREADS) {
        const double* zs = z + s * C;
        double mx = -INFINITY, se = 0.0;
#pragma unroll
        for (int c = 0; c < MAXC; ++c)
            if (c < C) {
                double t = m[c];
                for (int k = 0; k <= c; ++k) t += L[c][k] * zs[k];
                gv[c] = t;
                mx = fmax(mx, t);
            }
#pragma unroll
        for (int c = 0; c < MAXC; ++c)
            if (c < C) { gv[c] = exp(gv[c] - mx); se += gv[c]; }
#pragma unroll
        for (int c = 0; c < MAXC; ++c)
            if (c < C) acc[c] += gv[c] / se;
    }
#pragma unroll
    for (int c = 0; c < MAXC; ++c)
        if (c < C) partial[threadIdx.x][c] = acc[c];
    __syncthreads();
    if ((int)threadIdx.x < C) {
        double t = 0.0;
        for (int k = 0; k < VEC_THREADS; ++k) t += partial[k][threadIdx.x];
        prob[i * C + threadIdx.x] = t / (double)S;
    }
}

// Gradient, one thread per training point: P from F as softmax_newton_kernel forms it (maximum subtracted), then from the
// point's C x C posterior covariance Sg = cov[i]
//     q_c = Sg_cc - 2 sum_e Sg_ce pi_e,   s2_c = -(pi_c (q_c - sum_e pi_e q_e)) / 2
// (= -1/2 sum_pq Sg_pq dW_pq/df_c for W = diag(pi) - pi pi^T; e runs in index order).  0 past N.
__global__ __launch_bounds__(VEC_THREADS) void softmax_s2_kernel(int64_t N, int64_t Np, int C, const double* __restrict__ F,
                                                                 const double* __restrict__ cov, double* __restrict__ s2) {
    const int64_t i = (int64_t)blockIdx.x * VEC_THREADS + threadIdx.x;
    if (i >= Np) return;
    if (i >= N) {
        for (int c = 0; c < C; ++c) s2[c * Np + i] = 0.0;
        return;
    }
    double pr[MAXC], q[MAXC];
    double fmx = -INFINITY, se = 0.0;
#pragma unroll
    for (int c = 0; c < MAXC; ++c) {
        pr[c] = 0.0;
        if (c < C) { pr[c] = F[c * Np + i]; fmx = fmax(fmx, pr[c]); }
    }
#pragma unroll
    for (int c = 0; c < MAXC; ++c)
        if (c < C) { pr[c] = exp(pr[c] - fmx); se += pr[c]; }
#pragma unroll
    for (int c = 0; c < MAXC; ++c)
        if (c < C) pr[c] = pr[c] / se;
    const double* Sg = cov + i * C * C;
    double pq = 0.0;
#pragma unroll
    for (int c = 0; c < MAXC; ++c) {
        q[c] = 0.0;
        if (c < C) {
            double sp = 0.0;
#pragma unroll
            for (int e = 0; e < MAXC; ++e)
                if (e < C) sp = fma(Sg[c * C + e], pr[e], sp);
            q[c] = Sg[c * C + c] - 2.0 * sp;
            pq = fma(pr[c], q[c], pq);
        }
    }
#pragma unroll
    for (int c = 0; c < MAXC; ++c)
        if (c < C) s2[c * Np + i] = -0.5 * (pr[c] * (q[c] - pq));
}

// z_c = (s2_c - v_c) + E_c t from the tile partials of (-E_c) t; 0 past N
__global__ __launch_bounds__(VEC_THREADS) void softmax_z_kernel(const double* __restrict__ part, int64_t nt, int64_t N,
                                                                int64_t Np, int C, const double* __restrict__ s2,
                                                                const double* __restrict__ v, double* __restrict__ z) {
    const int64_t i = (int64_t)blockIdx.x * VEC_THREADS + threadIdx.x;
    if (i >= Np) return;
    const int64_t pstride = nt * nt * LT;
    for (int c = 0; c < C; ++c) {
        const int64_t o = c * Np + i;
        z[o] = i < N ? (s2[o] - v[o]) - slot_sum(part + c * pstride, nt, i) : 0.0;
    }
}

// One workgroup per lower tile (I, J) of the gradient's weight matrix, written over nGam (which holds -Gamma there):
//     Wm = (sum_c nE_c - nGam) + sum_c (g_ci g_ck + z_ci g_ck + g_ci z_ck)
// i.e. -sum_c E_c + Gamma plus the rank-3C term, classes in index order in both sums; one read of the C + 1 tiles and
// one write.  The tile's row and column segments of the 2 C vectors sit in LDS (4 C x 128 doubles, dynamic).  Whole
// tiles: the E_c are mirrored and the product behind nGam computes its diagonal tiles whole.
__global__ __launch_bounds__(VEC_THREADS) void softmax_weight_kernel(const double* __restrict__ nE, int64_t estride, int C,
                                                                     double* __restrict__ nGam, int64_t ld, int64_t Np,
                                                                     const double* __restrict__ g,
                                                                     const double* __restrict__ z) {
    extern __shared__ __attribute__((aligned(16))) double wv[];       // [4][C][LT]: g_I, z_I, g_J, z_J
    int64_t I, J;
    tile_of(blockIdx.x, I, J);
    for (int e = threadIdx.x; e < 4 * C * LT; e += VEC_THREADS) {
        const int which = e / (C * LT), c = (e / LT) % C, t = e % LT;
        const double* src = (which & 1) ? z : g;
        wv[e] = src[(int64_t)c * Np + ((which & 2) ? J : I) * LT + t];
    }
    __syncthreads();
    const double *gI = wv, *zI = wv + C * LT, *gJ = wv + 2 * C * LT, *zJ = wv + 3 * C * LT;
    for (int e = threadIdx.x; e < LT * LT / 2; e += VEC_THREADS) {
        const int r = e / (LT / 2), c0 = 2 * (e % (LT / 2));
        const int64_t o = (I * LT + r) * ld + J * LT + c0;
        double e0 = 0.0, e1 = 0.0, t0 = 0.0, t1 = 0.0;
        for (int c = 0; c < C; ++c) {
            const d2 ev = *reinterpret_cast<const d2*>(nE + c * estride + o);
            e0 += ev.x; e1 += ev.y;
            const double gi = gI[c * LT + r], zi = zI[c * LT + r];
            const d2 gk = *reinterpret_cast<const d2*>(&gJ[c * LT + c0]);
            const d2 zk = *reinterpret_cast<const d2*>(&zJ[c * LT + c0]);
            t0 = fma(gi, gk.x, t0); t0 = fma(zi, gk.x, t0); t0 = fma(gi, zk.x, t0);
            t1 = fma(gi, gk.y, t1); t1 = fma(zi, gk.y, t1); t1 = fma(gi, zk.y, t1);
        }
        const d2 gm = *reinterpret_cast<const d2*>(nGam + o);
        *reinterpret_cast<d2*>(nGam + o) = d2{(e0 - gm.x) + t0, (e1 - gm.y) + t1};
    }
}

// vectors per pass over a tile: the fewest passes with at most 4 vectors each, spread evenly
int symv_chunk(int nvec) {
    const int passes = (nvec + 3) / 4;
    return (nvec + passes - 1) / passes;
}

hipError_t launch_symv(hipStream_t st, const SymvArgs& a, int nmat) {
    const dim3 grid((unsigned)(a.nt * (a.nt + 1) / 2), (unsigned)nmat);
    switch (symv_chunk(a.nvec)) {
        case 1: hipLaunchKernelGGL(softmax_symv_kernel<1>, grid, dim3(SYMV_THREADS), 0, st, a); break;
        case 2: hipLaunchKernelGGL(softmax_symv_kernel<2>, grid, dim3(SYMV_THREADS), 0, st, a); break;
        case 3: hipLaunchKernelGGL(softmax_symv_kernel<3>, grid, dim3(SYMV_THREADS), 0, st, a); break;
        default: hipLaunchKernelGGL(softmax_symv_kernel<4>, grid, dim3(SYMV_THREADS), 0, st, a); break;
    }
    return hipGetLastError();
}

// Vectors of the softmax state in c->sm.  C x Np each: A, A_prev, F, F_prev, sqrt(P), Y - P, B, K B, C; then Np each: sum_c C_c
// and 2 for the backward solve (its right-hand side, its solution); then the Psi partials, the read-back record and the
// C + 1 pairs of launch_logdiag_sumsq.
enum { SV_A, SV_AP, SV_F, SV_FP, SV_S, SV_G, SV_B, SV_KB, SV_CC, SV_MATS };
enum { SW_CSUM, SW_X, SW_VECS = SW_X + 2 };

}  // namespace

static const char* const PIVOT_TEXT = "a Cholesky factorisation met a non-positive pivot";

// The multi-class fit as newton_iterate's problem (gpmi_state.h).  h is the last read-back record: h[0] ends as Psi at
// the mode.
namespace {
struct SoftmaxNewton {
    gpmi_ctx* c;
    int C;
    bool chain;
    int64_t nblk;
    SoftVecs v;
    double *K, *V, *nE, *part;     // Kn, U, sm_E, sm_part
    double *kb, *cc, *wv;          // K B and C (C x Np each), the Np-vectors behind the matrices of c->sm
    double *psi_part, *rec, *zrec; // ... then the Psi partials, the read-back record, the log-diagonal sums
    SymvArgs kx, ex;               // K times C vectors; -E_c times one vector each
    double h[3];

    int forward() {
        kx.x = v.a;                                                   // 1. F = A K
        HIP_TRY(launch_symv(c->stream, kx, 1));
        return GPMI_OK;
    }
    // 1., 2. Psi of the iterate, with the previous Cholesky's pivot word and backward solve's give-up word
    int evaluate(int mode, double* psi) {
        LAUNCH_TRY(softmax_newton_kernel, dim3((unsigned)nblk), dim3(VEC_THREADS), 0, c->stream, mode, (const double*)part,
                   c->Np / TILE, c->N, c->Np, C, (const double*)c->y.as<double>(), v, psi_part);
        const int rc = newton_readback(c, psi_part, nblk, chain, rec, h, "gpmi_softmax_fit", PIVOT_TEXT);
        *psi = h[0];
        return rc;
    }
    int factor(bool last) {
        hipStream_t st = c->stream;
        const int64_t N = c->N, Np = c->Np, nt = Np / TILE, ld = c->ldA, msize = Np * ld;
        const unsigned tiles = (unsigned)(nt * (nt + 1) / 2);
        double* A = c->A.as<double>();
        // 3. per class: L_c = chol(I + s_c s_c^T o K) in A, V = S_c L_c^-T, -E_c = -V V^T (lower tiles)
        HIP_TRY(launch_fill_rows(st, c->m_row(), ld, TILE, Np, 0.0));     // nothing rides in these factorisations
        for (int k = 0; k < C; ++k) {
            const double* sk = v.s + (int64_t)k * Np;
            LAUNCH_TRY(softmax_bmat_kernel, dim3(tiles), dim3(VEC_THREADS), 0, st, (const double*)K, A, ld, N, sk);
            HIP_TRY(cholesky_inplace(c, A, ld, Np, c->Mp, c->info.as<int64_t>(), false));
            c->res.factor_replaced(tuning().panel_fused);
            HIP_TRY(launch_logdiag_sumsq(st, A, ld, N, nullptr, 0, zrec + 2 * k));
            HIP_TRY(launch_fill_rows(st, V, ld, Np, Np, 0.0));
            LAUNCH_TRY(softmax_seed_kernel, dim3(grid_of(Np)), dim3(VEC_THREADS), 0, st, V, ld, Np, sk);
            HIP_TRY(solve_sweep(c, V, ld, Np, true));
            HIP_TRY(neg_gram_lower(c, V, nE + (int64_t)k * msize, ld, Np));
        }
        if (!last) {                                                  // 4. c_c = E_c (K b_c), sum_c c_c rides with M
            kx.x = v.b;
            HIP_TRY(launch_symv(st, kx, 1));
            LAUNCH_TRY(softmax_vec_kernel, dim3(grid_of(Np)), dim3(VEC_THREADS), 0, st, (const double*)part, nt, N, Np, C, 1.0,
                       kb, (double*)nullptr);
            ex.x = kb; ex.xstride = Np;
            HIP_TRY(launch_symv(st, ex, C));
            LAUNCH_TRY(softmax_vec_kernel, dim3(grid_of(Np)), dim3(VEC_THREADS), 0, st, (const double*)part, nt, N, Np, C, -1.0,
                       cc, wv + SW_CSUM * Np);
            HIP_TRY(launch_set_yrow(st, c->m_row(), wv + SW_CSUM * Np, N, Np));
        }
        // 5. M = chol(sum_c E_c) in A
        LAUNCH_TRY(softmax_esum_kernel, dim3(tiles), dim3(VEC_THREADS), 0, st, (const double*)nE, msize, C, A, ld, N);
        HIP_TRY(cholesky_inplace(c, A, ld, Np, c->Mp, c->info.as<int64_t>(), false));
        c->res.factor_replaced(tuning().panel_fused);
        HIP_TRY(launch_logdiag_sumsq(st, A, ld, N, nullptr, 0, zrec + 2 * C));
        return GPMI_OK;
    }
    int step() {
        const int64_t Np = c->Np;
        double* x = nullptr;                                          // 6. t = M^-T M^-1 sum_c c_c, A <- B - C + [E_c t]
        HIP_TRY(backward_solve_resident(c, wv + SW_X * Np, &x));
        ex.x = x; ex.xstride = 0;
        HIP_TRY(launch_symv(c->stream, ex, C));
        LAUNCH_TRY(softmax_update_kernel, dim3(grid_of(Np)), dim3(VEC_THREADS), 0, c->stream, (const double*)part, Np / TILE,
                   c->N, Np, C, (const double*)cc, v);
        return GPMI_OK;
    }
};
}  // namespace

int softmax_fit_impl(gpmi_ctx* c, int C, double sigma, double ell, double tol, int max_iter, double* log_q, int* iters,
                     int* converged, double* f_hat) {
    int rc = classifier_fit_check(c, "gpmi_softmax_fit",
                                  C < 2 || C > MAXC ? "n_classes must lie in [2, GPMI_SOFTMAX_MAX_CLASSES]" : nullptr, sigma,
                                  ell, tol, max_iter);
    if (rc) return rc;
    if ((rc = classifier_labels_check(c, "gpmi_softmax_fit",
                                      [](double v, int nc) { return v >= 0.0 && v < (double)nc && v == std::floor(v); },
                                      C, "labels must be integers in [0, n_classes)")))
        return rc;
    bool chain = false;
    if ((rc = classifier_fit_begin(c, sigma, ell, &chain)) != GPMI_OK) return rc;
    hipStream_t st = c->stream;
    const int64_t N = c->N, Np = c->Np, nt = Np / TILE, ld = c->ldA;
    const int64_t nblk = (Np + VEC_THREADS - 1) / VEC_THREADS;
    const int64_t msize = Np * ld;                  // doubles of one N x N matrix
    HIP_TRY(c->Kn.ensure((size_t)msize * 8));       // K
    HIP_TRY(c->U.ensure((size_t)msize * 8));        // V_c = S_c L_c^-T
    HIP_TRY(c->sm_E.ensure((size_t)C * msize * 8)); // -E_c
    HIP_TRY(c->sm.ensure(((size_t)(SV_MATS * C + SW_VECS) * Np + 2 * nblk + 8 + 2 * (MAXC + 1)) * 8));
    HIP_TRY(c->sm_part.ensure((size_t)C * nt * nt * TILE * 8));
    double* Sm = c->sm.as<double>();
    auto mat = [&](int k) { return Sm + (int64_t)k * C * Np; };
    SoftmaxNewton p;
    p.c = c; p.C = C; p.chain = chain; p.nblk = nblk;
    p.v = SoftVecs{mat(SV_A), mat(SV_AP), mat(SV_F), mat(SV_FP), mat(SV_S), mat(SV_G), mat(SV_B)};
    p.K = c->Kn.as<double>(); p.V = c->U.as<double>(); p.nE = c->sm_E.as<double>(); p.part = c->sm_part.as<double>();
    p.kb = mat(SV_KB); p.cc = mat(SV_CC); p.wv = mat(SV_MATS);
    p.psi_part = p.wv + SW_VECS * Np; p.rec = p.psi_part + 2 * nblk; p.zrec = p.rec + 8;
    p.kx.M = p.K; p.kx.mstride = 0; p.kx.ld = ld; p.kx.nt = nt; p.kx.xstride = 0; p.kx.nvec = C; p.kx.part = p.part;
    p.ex.M = p.nE; p.ex.mstride = msize; p.ex.ld = ld; p.ex.nt = nt; p.ex.nvec = 1; p.ex.part = p.part;
    HIP_TRY(hipMemsetAsync(p.v.a, 0, (size_t)C * Np * 8, st));
    HIP_TRY(launch_rbf(st, rbf_sym(c, c->x_train(), N, c->box_train(), 0.0, Np, p.K, ld)));    // K, once per fit
    int it = 0;
    bool conv = false;
    if ((rc = newton_iterate(p, tol, max_iter, &it, &conv)) != GPMI_OK) return rc;
    for (int k = 0; k < C; ++k)                                       // prediction multiplies by the whole E_c
        HIP_TRY(launch_mirror_lower(st, p.nE + (int64_t)k * msize, ld, Np));
    std::vector<double> red(2 * (size_t)(C + 1));
    int64_t info = 0;
    HIP_TRY(hipMemcpyAsync(red.data(), p.zrec, red.size() * 8, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipMemcpyAsync(&info, c->info.p, sizeof info, hipMemcpyDeviceToHost, st));
    if (f_hat)
        HIP_TRY(hipMemcpy2DAsync(f_hat, (size_t)N * 8, p.v.f, (size_t)Np * 8, (size_t)N * 8, (size_t)C, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    c->timers_collect();
    if (info != NO_BAD_PIVOT) { g_err = std::string("gpmi_softmax_fit: ") + PIVOT_TEXT; return GPMI_ERR_NOT_PD; }
    // log q = Psi - sum_c sum log diag L_c - sum log diag M
    double z = 0.0;
    for (int k = 0; k < C; ++k) z += red[2 * (size_t)k];
    if (log_q) *log_q = (p.h[0] - z) - red[2 * (size_t)C];
    if (iters) *iters = it;
    if (converged) *converged = conv ? 1 : 0;
    c->sm_classes = C;
    c->res.fit_done(Fit::Softmax);
    return GPMI_OK;
}

// The latent covariance of GPML Algorithm 3.4 at np points from their cross-covariance rows R = K(points, X) (np x Np,
// leading dimension ldr): B_c = R E_c in Bc (C np rows, leading dimension ldr), dd[i][c] = B_c[i] . R[i], one sweep
// U_c^T = B_c M^-T over all classes, cov[i] = [U_c[i] . U_e[i]] + diag(sigma^2 - dd[i]).  The prediction runs it on
// K(X*, X), the gradient on K itself.
static int latent_cov(gpmi_ctx* c, const double* R, int64_t ldr, int64_t np, double* Bc, double* dd, double* cov) {
    hipStream_t st = c->stream;
    const int C = c->sm_classes;
    const int64_t Np = c->Np, ld = c->ldA, msize = Np * ld;
    const double* nE = c->sm_E.as<double>();
    HIP_TRY(launch_fill_rows(st, Bc, ldr, C * np, Np, 0.0));
    for (int k = 0; k < C; ++k) {                                     // B_c = R E_c = 0 - R (-E_c)^T
        HIP_TRY(launch_gemm_nt(st, gemm_minus(Bc + (int64_t)k * np * ldr, ldr, R, ldr, nE + (int64_t)k * msize, ld, np, Np, Np)));
    }
    LAUNCH_TRY(softmax_rowdot_kernel, dim3((unsigned)np), dim3(VEC_THREADS), 0, st, R, ldr, Np, (const double*)Bc, np * ldr,
               ldr, C, dd);                                           // B_c[i] . R[i]
    HIP_TRY(solve_sweep(c, Bc, ldr, C * np));                         // U_c^T = B_c M^-T, all classes in one sweep
    LAUNCH_TRY(softmax_gram_kernel, dim3((unsigned)np), dim3(VEC_THREADS), 0, st, (const double*)Bc, ldr, np, Np, C, c->sig2,
               (const double*)dd, cov);
    return GPMI_OK;
}

int softmax_predict_impl(gpmi_ctx* c, double* mu, double* cov, int64_t S, const double* normals, double* prob) {
    if (!c->res.softmax()) return fail_arg("gpmi_softmax_predict: no softmax fit resident (call gpmi_softmax_fit)");
    if (!c->res.have_test) return fail_arg("gpmi_softmax_predict: no test set (call gpmi_set_test)");
    if (S < 0 || (S > 0 && (!normals || !prob))) return fail_arg("gpmi_softmax_predict: n_samples > 0 needs normals and prob");
    const Tuning tn = resident_tuning(c);
    TuneScope tune_scope(&tn);
    hipStream_t st = c->stream;
    const int C = c->sm_classes;
    const int64_t Np = c->Np, np_ = c->np_, n = c->n;
    const int64_t ldV = Np + c->ld_pad;                   // what predict_front makes c->ldV
    HIP_TRY(c->sm_B.ensure((size_t)C * np_ * ldV * 8));
    HIP_TRY(c->sm_out.ensure(((size_t)np_ * C * (3 + C) + (size_t)S * C) * 8));
    int rc = predict_front(c, -1);                        // R = K(X*, X)
    if (rc) return rc;
    double* R = c->V.as<double>();
    double* Bc = c->sm_B.as<double>();
    double* o_mu = c->sm_out.as<double>();
    double* o_dd = o_mu + np_ * C;
    double* o_prob = o_dd + np_ * C;
    double* o_cov = o_prob + np_ * C;
    double* o_z = o_cov + np_ * C * C;
    const double* G = c->sm.as<double>() + (int64_t)SV_G * C * Np;
    LAUNCH_TRY(softmax_rowdot_kernel, dim3((unsigned)np_), dim3(VEC_THREADS), 0, st, (const double*)R, ldV, Np, G, Np,
               (int64_t)0, C, o_mu);                                  // mu* = R (Y - P)^T
    if ((rc = latent_cov(c, R, ldV, np_, Bc, o_dd, o_cov)) != GPMI_OK) return rc;
    if (S > 0) {
        HIP_TRY(hipMemcpyAsync(o_z, normals, (size_t)S * C * 8, hipMemcpyHostToDevice, st));
        LAUNCH_TRY(softmax_sample_kernel, dim3((unsigned)n), dim3(VEC_THREADS), 0, st, C, S, (const double*)o_mu,
                   (const double*)o_cov, (const double*)o_z, o_prob);
    }
    if (mu) HIP_TRY(hipMemcpyAsync(mu, o_mu, (size_t)n * C * 8, hipMemcpyDeviceToHost, st));
    if (cov) HIP_TRY(hipMemcpyAsync(cov, o_cov, (size_t)n * C * C * 8, hipMemcpyDeviceToHost, st));
    if (S > 0) HIP_TRY(hipMemcpyAsync(prob, o_prob, (size_t)n * C * 8, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    c->timers_collect();
    return GPMI_OK;
}

// The gradient of log q at the resident fit w.r.t. the hyper-parameters of the shared kernel (include/gpmi.h has the
// formulas; GPML prints no algorithm for the multi-class case).  It reads M (A), K (Kn, whose lower triangle it mirrors
// into the upper one: the same bits every call), the -E_c, F and G = Y - P, and writes scratch only:
//   1. Sigma_i, the C x C posterior covariance at every training point: latent_cov with R = K (C matrices in sm_B)
//   2. s2 by softmax_s2_kernel
//   3. z = s2 - R K_blk s2: K s2_c, v_c = E_c (K s2_c), t = M^-T M^-1 sum_c v_c (the forward half as a one-row sweep in
//      U, the backward half by the resident factor's solve), z_c = s2_c - v_c + E_c t
//   4. -Gamma = -sum_c T_c^T T_c into the first matrix of sm_B (dead since 1.): per class U <- -E_c, the sweep
//      U <- U M^-T = -T_c^T, and the lower-tile product by the subtracting GEMM
//   5. Wm over -Gamma by softmax_weight_kernel
//   6. the d + 3 sums of grad_ard_kernel in its regression form with Kn := Wm and alpha := 0 (weight = Wm_ij exactly)
// The vectors live in loov.  V is not touched.
int softmax_grad_impl(gpmi_ctx* c, double* d_r, double* d_ell, double* d_sigma) {
    if (!c->res.softmax()) return fail_arg("gpmi_softmax_grad: no softmax fit resident (call gpmi_softmax_fit)");
    const Tuning tn = resident_tuning(c);
    TuneScope tune_scope(&tn);
    hipStream_t st = c->stream;
    const int C = c->sm_classes;
    const int64_t N = c->N, Np = c->Np, nt = Np / TILE, ld = c->ldA, msize = Np * ld;
    c->timers_reset({GPMI_T_GRAD});
    // C x Np each: s2, K s2, v, z; Np each: sum_c v_c, the backward solve's two, zeros; then Sigma and the row dots
    const size_t nvec = (size_t)(4 * C + 4 + C * C + C) * Np;
    {
        hipError_t e = c->sm_B.ensure((size_t)C * msize * 8);
        if (e == hipSuccess) e = c->loov.ensure(nvec * 8);
        if (e != hipSuccess) {
            (void)hipGetLastError();
            return fail_runtime(e, "gpmi_softmax_grad: workspace");
        }
    }
    HIP_TRY(c->sm_part.ensure((size_t)C * nt * nt * TILE * 8));
    double* s2 = c->loov.as<double>();
    double *ks2 = s2 + (int64_t)C * Np, *vv = ks2 + (int64_t)C * Np, *z = vv + (int64_t)C * Np;
    double *vsum = z + (int64_t)C * Np, *x2 = vsum + Np, *zero = x2 + 2 * Np;
    double *cov = zero + Np, *dd = cov + (int64_t)C * C * Np;
    double* K = c->Kn.as<double>();
    double* U = c->U.as<double>();
    double* Bc = c->sm_B.as<double>();
    double* part = c->sm_part.as<double>();
    const double* nE = c->sm_E.as<double>();
    const double* F = c->sm.as<double>() + (int64_t)SV_F * C * Np;
    const double* G = c->sm.as<double>() + (int64_t)SV_G * C * Np;
    const unsigned tiles = (unsigned)(nt * (nt + 1) / 2);
    int rc;

    const size_t sp = c->span_begin(GPMI_T_GRAD);
    HIP_TRY(launch_mirror_lower(st, K, ld, Np));                      // K whole: its rows are the R of latent_cov
    if ((rc = latent_cov(c, K, ld, Np, Bc, dd, cov)) != GPMI_OK) return rc;                  // 1.
    LAUNCH_TRY(softmax_s2_kernel, dim3(grid_of(Np)), dim3(VEC_THREADS), 0, st, N, Np, C, F, (const double*)cov, s2);   // 2.

    SymvArgs kx;                                                                             // 3.
    kx.M = K; kx.mstride = 0; kx.ld = ld; kx.nt = nt; kx.x = s2; kx.xstride = 0; kx.nvec = C; kx.part = part;
    HIP_TRY(launch_symv(st, kx, 1));
    LAUNCH_TRY(softmax_vec_kernel, dim3(grid_of(Np)), dim3(VEC_THREADS), 0, st, (const double*)part, nt, N, Np, C, 1.0, ks2,
               (double*)nullptr);
    SymvArgs ex;
    ex.M = nE; ex.mstride = msize; ex.ld = ld; ex.nt = nt; ex.x = ks2; ex.xstride = Np; ex.nvec = 1; ex.part = part;
    HIP_TRY(launch_symv(st, ex, C));
    LAUNCH_TRY(softmax_vec_kernel, dim3(grid_of(Np)), dim3(VEC_THREADS), 0, st, (const double*)part, nt, N, Np, C, -1.0, vv,
               vsum);
    HIP_TRY(launch_fill_rows(st, U, ld, TILE, Np, 0.0));              // M^-1 sum_c v_c: row 0 of a one-tile sweep
    HIP_TRY(launch_set_yrow(st, U, vsum, N, Np));
    HIP_TRY(solve_sweep(c, U, ld, TILE));
    HIP_TRY(hipMemcpyAsync(x2, U, (size_t)Np * 8, hipMemcpyDeviceToDevice, st));
    double* t = nullptr;
    HIP_TRY(backward_solve_rhs(c, x2, &t));
    ex.x = t; ex.xstride = 0;
    HIP_TRY(launch_symv(st, ex, C));
    LAUNCH_TRY(softmax_z_kernel, dim3(grid_of(Np)), dim3(VEC_THREADS), 0, st, (const double*)part, nt, N, Np, C,
               (const double*)s2, (const double*)vv, z);

    HIP_TRY(launch_fill_rows(st, Bc, ld, Np, Np, 0.0));                                      // 4.
    for (int k = 0; k < C; ++k) {
        HIP_TRY(hipMemcpyAsync(U, nE + (int64_t)k * msize, (size_t)msize * 8, hipMemcpyDeviceToDevice, st));
        HIP_TRY(solve_sweep(c, U, ld, Np));
        HIP_TRY(neg_gram_lower_dense(c, U, Bc, ld, Np));
    }
    LAUNCH_TRY(softmax_weight_kernel, dim3(tiles), dim3(VEC_THREADS), (size_t)4 * C * LT * sizeof(double), st, nE, msize, C,
               Bc, ld, Np, G, (const double*)z);                                             // 5.

    HIP_TRY(hipMemsetAsync(zero, 0, (size_t)Np * 8, st));                                    // 6.
    GradArdArgs ga;
    ga.Z = c->x_train(); ga.n = N; ga.d = c->d;
    ga.alpha = zero; ga.Kn = Bc; ga.ld = ld; ga.coef = c->coef;
    ga.family = 0;
    std::vector<double> sums;                             // backward_solve_rhs ran: its give-up word is read
    if ((rc = grad_ard_finish(c, ga, sp, "gpmi_softmax_grad", &sums))) return rc;
    grad_ard_scale(c, ga, sums, c->ell * c->ell, d_r, d_ell, d_sigma, nullptr);      // the noise slot is unused
    return GPMI_OK;
}

}  // namespace gpmi
