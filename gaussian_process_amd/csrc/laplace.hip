// Binary GP classification by the Laplace approximation (Rasmussen & Williams, GPML, Algorithms 3.1 and 3.2, logistic
// likelihood, labels +-1): the memory-bound kernels around the existing hot path and the Newton driver.
//
// Each Newton step factors B = I + W^1/2 K W^1/2 (always SPD) with the blocked Cholesky of driver.hip, the right-hand side
// c = W^1/2 K b riding in the y row; the backward solve is the one behind gpmi_get_alpha.  What is new here:
//   laplace_symv_kernel<false>  f = K a over the lower tiles of the freshly built K (one read of the lower triangle)
//   laplace_symv_kernel<true>   u = K b and, in the same pass, K <- B on the lower tiles (one read, one write)
//   laplace_newton_kernel       f from the tile partials (or the halved step), pi, W^1/2, grad, b and the partials of Psi
//   newton_psi_kernel           Psi = -a^T f / 2 + sum log p(y|f) in a fixed order, with the Cholesky's pivot word and the
//                               backward solve's give-up word, so an iteration reads back one small record (softmax.hip
//                               uses it too, with the rest of the Newton skeleton at the end of this file's kernels)
//   laplace_rhs_kernel          c = W^1/2 (K b) from the tile partials
//   laplace_update_kernel       a <- b - W^1/2 x (keeping the previous a, f for step halving)
//   laplace_rows_kernel         prediction: f* = K(X*, X) grad, then the rows are scaled by W^1/2 in place
//   laplace_quad_kernel         prediction: V* = sigma^2 - |v|^2 and pi* = int expit(z) N(z | f*, V*) dz
//   laplace_s2_kernel           gradient: s2 = -(1 - [B^-1]_ii) (1 - 2 pi) / 2 from kappa and f^
//   laplace_z_kernel            gradient: z = s2 + s o (Kn t) from the tile partials
// Every reduction runs in a fixed order (no atomics), so two fits give the same bits.
// Host side: the fit is a problem object (LaplaceNewton) for newton_iterate of gpmi_state.h, which owns the loop; what
// softmax.hip shares is classifier_fit_check, classifier_labels_check, classifier_fit_begin and newton_readback; the
// gradient ends in regress.hip's ARD trace ending (grad_ard_finish, grad_ard_scale), the prediction starts with predict_front.
#include "gpmi_ctx.h"
#include "lap_dev.h"

namespace gpmi {

namespace {

using namespace lapdev;      // d2, LT, SYMV_THREADS, VEC_THREADS, tile_of, slot_sum, wg_reduce2

__device__ __forceinline__ double expit(double z) {
    if (z >= 0.0) return 1.0 / (1.0 + exp(-z));
    const double e = exp(z);
    return e / (1.0 + e);
}

// One workgroup per lower tile (I, J) of the nt x nt tile grid.  Partial sums go to slots of 128 doubles:
//   slot (I, J) <- K_IJ x_J         (rows of tile (I, J))
//   slot (J, I) <- K_IJ^T x_I       (J < I: the tile read a second time as the upper tile (J, I))
// and the diagonal tile puts both halves (c <= r, and r > c transposed) into slot (I, I), so y_a = sum_b slot (a, b).
// Lane (g = lane / 8, q = lane % 8) of wave w reads row r = 32 * step + 8 * w + g at columns 16 k + 2 q (+1), k = 0..7:
// every 16-byte load instruction of a wave covers eight rows, one whole 128-byte line of each.
// SCALE: K_IJ is overwritten by B_IJ = delta_ij + s_i s_j K_ij (lower triangle of the diagonal tiles; real rows and
// columns only, the padding becomes exactly the identity).
template <bool SCALE>
__global__ __launch_bounds__(SYMV_THREADS) void laplace_symv_kernel(double* __restrict__ A, int64_t ld, int64_t nt,
                                                                    int64_t N, const double* __restrict__ x,
                                                                    const double* __restrict__ s,
                                                                    double* __restrict__ part) {
    __shared__ double rowsum[LT];
    __shared__ double colsum[SYMV_THREADS / 64][LT];
    int64_t I, J;
    tile_of(blockIdx.x, I, J);
    const bool diag = I == J;
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6, g = lane >> 3, q = lane & 7;
    double* T = A + I * LT * ld + J * LT;
    const double* xI = x + I * LT;
    const double* xJ = x + J * LT;
    double xj[16], cacc[16], sj[16];
#pragma unroll
    for (int k = 0; k < 8; ++k) {
        const d2 v = *reinterpret_cast<const d2*>(xJ + 16 * k + 2 * q);
        xj[2 * k] = v.x; xj[2 * k + 1] = v.y;
        cacc[2 * k] = 0.0; cacc[2 * k + 1] = 0.0;
        if (SCALE) {
            const d2 u = *reinterpret_cast<const d2*>(s + J * LT + 16 * k + 2 * q);
            sj[2 * k] = u.x; sj[2 * k + 1] = u.y;
        }
    }
    // one row step (8 loads of 16 bytes per lane) at a time: the registers stay under 128 and four workgroups share a CU
#pragma unroll 1
    for (int st = 0; st < 4; ++st) {
        const int r = 32 * st + 8 * w + g;
        d2 kv[8];
#pragma unroll
        for (int k = 0; k < 8; ++k) kv[k] = *reinterpret_cast<const d2*>(T + (int64_t)r * ld + 16 * k + 2 * q);
        const double xr = xI[r];
        double rp = 0.0;
#pragma unroll
        for (int k = 0; k < 8; ++k) {
            const int c0 = 16 * k + 2 * q;
            double k0 = kv[k].x, k1 = kv[k].y;
            if (diag) {                                   // lower triangle only: row part c <= r, column part r > c
                rp = fma(c0 <= r ? k0 : 0.0, xj[2 * k], rp);
                rp = fma(c0 + 1 <= r ? k1 : 0.0, xj[2 * k + 1], rp);
                cacc[2 * k] = fma(r > c0 ? k0 : 0.0, xr, cacc[2 * k]);
                cacc[2 * k + 1] = fma(r > c0 + 1 ? k1 : 0.0, xr, cacc[2 * k + 1]);
            } else {
                rp = fma(k0, xj[2 * k], rp);
                rp = fma(k1, xj[2 * k + 1], rp);
                cacc[2 * k] = fma(k0, xr, cacc[2 * k]);
                cacc[2 * k + 1] = fma(k1, xr, cacc[2 * k + 1]);
            }
        }
        rp += __shfl_xor(rp, 1, 64);
        rp += __shfl_xor(rp, 2, 64);
        rp += __shfl_xor(rp, 4, 64);
        if (q == 0) rowsum[r] = rp;
        if (SCALE) {
            const int64_t gi = I * LT + r;
            const double si = s[gi];
            double* Tr = T + (int64_t)r * ld;
#pragma unroll
            for (int k = 0; k < 8; ++k) {
                const int c0 = 16 * k + 2 * q;
                const int64_t gj = J * LT + c0;
                double b0 = (gi < N && gj < N) ? (si * sj[2 * k]) * kv[k].x : 0.0;
                double b1 = (gi < N && gj + 1 < N) ? (si * sj[2 * k + 1]) * kv[k].y : 0.0;
                if (gi == gj) b0 = 1.0 + b0;
                if (gi == gj + 1) b1 = 1.0 + b1;
                if (!diag) {
                    *reinterpret_cast<d2*>(Tr + c0) = d2{b0, b1};
                } else {
                    if (c0 <= r) Tr[c0] = b0;
                    if (c0 + 1 <= r) Tr[c0 + 1] = b1;
                }
            }
        }
    }
    // column part: sum over the eight row groups of the wave, then over the four waves (fixed order)
#pragma unroll
    for (int k = 0; k < 16; ++k) {
        double v = cacc[k];
        v += __shfl_xor(v, 8, 64);
        v += __shfl_xor(v, 16, 64);
        v += __shfl_xor(v, 32, 64);
        cacc[k] = v;
    }
    if (g == 0) {
#pragma unroll
        for (int k = 0; k < 8; ++k) {
            colsum[w][16 * k + 2 * q] = cacc[2 * k];
            colsum[w][16 * k + 2 * q + 1] = cacc[2 * k + 1];
        }
    }
    __syncthreads();
    if (threadIdx.x < LT) {
        const int t = threadIdx.x;
        const double cs = ((colsum[0][t] + colsum[1][t]) + colsum[2][t]) + colsum[3][t];
        if (diag) {
            part[(I * nt + I) * LT + t] = rowsum[t] + cs;
        } else {
            part[(I * nt + J) * LT + t] = rowsum[t];
            part[(J * nt + I) * LT + t] = cs;
        }
    }
}

struct NewtonVecs {
    double *a, *a_prev, *f, *f_prev, *s, *grad, *b;
};

// mode 0: f = K a from the tile partials; mode 1: the halved step, a <- (a + a_prev) / 2, f <- (f + f_prev) / 2.
// Then t = (y + 1) / 2, pi = expit(f), W = pi (1 - pi), s = sqrt(W), grad = t - pi, b = W f + grad; entries past N are 0.
// psi_part[2 blk] = sum a_i f_i, psi_part[2 blk + 1] = sum log p(y_i | f_i) = -softplus(-y_i f_i).
__global__ __launch_bounds__(VEC_THREADS) void laplace_newton_kernel(int mode, const double* __restrict__ part, int64_t nt,
                                                                     int64_t N, int64_t Np, const double* __restrict__ y,
                                                                     NewtonVecs v, double* __restrict__ psi_part) {
    __shared__ double sh[2 * (VEC_THREADS / 64)];
    const int64_t i = (int64_t)blockIdx.x * VEC_THREADS + threadIdx.x;
    double af = 0.0, lp = 0.0;
    if (i < Np) {
        double a, f;
        if (mode == 0) {
            a = v.a[i];
            f = i < N ? slot_sum(part, nt, i) : 0.0;
        } else {
            a = (v.a[i] + v.a_prev[i]) / 2;
            f = (v.f[i] + v.f_prev[i]) / 2;
            v.a[i] = a;
        }
        v.f[i] = f;
        double s = 0.0, gr = 0.0, b = 0.0;
        if (i < N) {
            const double yi = y[i];
            const double t = (yi + 1) / 2;
            const double pi = expit(f);
            const double W = pi * (1 - pi);
            s = sqrt(W);
            gr = t - pi;
            b = W * f + gr;
            const double z = -yi * f;                        // log p = -softplus(z), overflow-safe
            lp = -(fmax(z, 0.0) + log1p(exp(-fabs(z))));
            af = a * f;
        }
        v.s[i] = s; v.grad[i] = gr; v.b[i] = b;
    }
    wg_reduce2(af, lp, sh);
    if (threadIdx.x == 0) { psi_part[2 * blockIdx.x] = af; psi_part[2 * blockIdx.x + 1] = lp; }
}

// out[0] = Psi = -a^T f / 2 + sum log p, out[1] = the Cholesky's first bad pivot (INT64_MAX: none) as a double,
// out[2] = the backward solve's give-up word (0 without one)
__global__ __launch_bounds__(VEC_THREADS) void newton_psi_kernel(const double* __restrict__ psi_part, int64_t nblk,
                                                                 const int64_t* __restrict__ info,
                                                                 const int* __restrict__ flag, double* __restrict__ out) {
    __shared__ double sh[2 * (VEC_THREADS / 64)];
    double af = 0.0, lp = 0.0;
    for (int64_t k = threadIdx.x; k < nblk; k += VEC_THREADS) { af += psi_part[2 * k]; lp += psi_part[2 * k + 1]; }
    wg_reduce2(af, lp, sh);
    if (threadIdx.x == 0) {
        out[0] = -0.5 * af + lp;
        out[1] = (double)*info;
        out[2] = flag ? (double)*flag : 0.0;
    }
}

// c = s o (K b) from the tile partials, 0 past N
__global__ __launch_bounds__(VEC_THREADS) void laplace_rhs_kernel(const double* __restrict__ part, int64_t nt, int64_t N,
                                                                  int64_t Np, const double* __restrict__ s,
                                                                  double* __restrict__ c) {
    const int64_t i = (int64_t)blockIdx.x * VEC_THREADS + threadIdx.x;
    if (i >= Np) return;
    c[i] = i < N ? s[i] * slot_sum(part, nt, i) : 0.0;
}

// a_prev <- a, f_prev <- f, a <- b - s o x
__global__ __launch_bounds__(VEC_THREADS) void laplace_update_kernel(int64_t N, int64_t Np, const double* __restrict__ x,
                                                                     NewtonVecs v) {
    const int64_t i = (int64_t)blockIdx.x * VEC_THREADS + threadIdx.x;
    if (i >= Np) return;
    v.a_prev[i] = v.a[i];
    v.f_prev[i] = v.f[i];
    v.a[i] = i < N ? v.b[i] - v.s[i] * x[i] : 0.0;
}

// one workgroup per row of R = K(X*, X): fbar[row] = R_row . grad (fixed order), then R_row <- R_row o s
__global__ __launch_bounds__(VEC_THREADS) void laplace_rows_kernel(double* __restrict__ R, int64_t ld, int64_t ncols,
                                                                   const double* __restrict__ grad,
                                                                   const double* __restrict__ s, double* __restrict__ fbar) {
    __shared__ double sh[2 * (VEC_THREADS / 64)];
    double* Rr = R + (int64_t)blockIdx.x * ld;
    double acc = 0.0, unused = 0.0;
    for (int64_t j = 2 * threadIdx.x; j < ncols; j += 2 * VEC_THREADS) {
        const d2 r = *reinterpret_cast<const d2*>(Rr + j);
        const d2 gv = *reinterpret_cast<const d2*>(grad + j);
        const d2 sv = *reinterpret_cast<const d2*>(s + j);
        acc = fma(r.x, gv.x, acc);
        acc = fma(r.y, gv.y, acc);
        *reinterpret_cast<d2*>(Rr + j) = d2{r.x * sv.x, r.y * sv.y};
    }
    wg_reduce2(acc, unused, sh);
    if (threadIdx.x == 0) fbar[blockIdx.x] = acc;
}

// var = sig2 - sq; prob = sum_k w_k expit(fbar + sqrt(max(var, 0)) t_k), t_k = -T + k h (k = 0..M), w_k = h phi(t_k) with
// the two end weights halved: the composite trapezoid rule of laplace_quad_nodes
__global__ __launch_bounds__(VEC_THREADS) void laplace_quad_kernel(int64_t n, const double* __restrict__ fbar,
                                                                   const double* __restrict__ sq, double sig2, int M,
                                                                   double T, double h, double* __restrict__ var,
                                                                   double* __restrict__ prob) {
    const int64_t i = (int64_t)blockIdx.x * VEC_THREADS + threadIdx.x;
    if (i >= n) return;
    const double v = sig2 - sq[i];
    const double sd = sqrt(fmax(v, 0.0));
    const double mu = fbar[i];
    const double c = h * 0.39894228040143267794;     // h / sqrt(2 pi)
    double acc = 0.0;
    for (int k = 0; k <= M; ++k) {
        const double t = -T + k * h;
        double wk = c * exp(-0.5 * t * t);
        if (k == 0 || k == M) wk = 0.5 * wk;
        acc = fma(wk, expit(mu + sd * t), acc);
    }
    var[i] = v;
    prob[i] = acc;
}

// s2_i = -(1 - kappa_i) (1 - 2 pi_i) / 2 with pi = expit(f^): half the diagonal of Sigma = (K^-1 + W)^-1 times the third
// derivative of log p (Sigma_ii W_i = 1 - [B^-1]_ii and the logistic's third derivative is -W (1 - 2 pi): W cancels, so
// saturated points lose nothing); 0 past N
__global__ __launch_bounds__(VEC_THREADS) void laplace_s2_kernel(int64_t N, int64_t Np, const double* __restrict__ kappa,
                                                                 const double* __restrict__ f, double* __restrict__ s2) {
    const int64_t i = (int64_t)blockIdx.x * VEC_THREADS + threadIdx.x;
    if (i >= Np) return;
    s2[i] = i < N ? -0.5 * ((1.0 - kappa[i]) * (1.0 - 2.0 * expit(f[i]))) : 0.0;
}

// z = s2 + s o (Kn t) from the tile partials of Kn t (Kn = -B^-1, t = s o (K s2): z = s2 - R K s2), 0 past N
__global__ __launch_bounds__(VEC_THREADS) void laplace_z_kernel(const double* __restrict__ part, int64_t nt, int64_t N,
                                                                int64_t Np, const double* __restrict__ s,
                                                                const double* __restrict__ s2, double* __restrict__ z) {
    const int64_t i = (int64_t)blockIdx.x * VEC_THREADS + threadIdx.x;
    if (i >= Np) return;
    z[i] = i < N ? fma(s[i], slot_sum(part, nt, i), s2[i]) : 0.0;
}

}  // namespace

hipError_t launch_newton_psi(hipStream_t st, const double* psi_part, int64_t nblk, const int64_t* info, const int* flag,
                             double* out) {
    hipLaunchKernelGGL(newton_psi_kernel, dim3(1), dim3(VEC_THREADS), 0, st, psi_part, nblk, info, flag, out);
    return hipGetLastError();
}

int newton_readback(gpmi_ctx* c, const double* psi_part, int64_t nblk, bool chain, double* rec, double (&h)[3],
                    const char* api, const char* pivot_text) {
    hipStream_t st = c->stream;
    HIP_TRY(launch_newton_psi(st, psi_part, nblk, c->info.as<int64_t>(), chain ? c->flag.as<int>() : nullptr, rec));
    HIP_TRY(hipMemcpyAsync(h, rec, sizeof h, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    c->timers_collect();
    const std::string who = std::string(api) + ": ";
    if (h[1] != (double)NO_BAD_PIVOT) { g_err = who + pivot_text; return GPMI_ERR_NOT_PD; }
    if (h[2] != 0.0) return fail_gave_up(api);
    if (!std::isfinite(h[0])) return fail_arg((who + "the objective is not finite").c_str());
    return GPMI_OK;
}

int classifier_fit_check(const gpmi_ctx* c, const char* api, const char* own, double sigma, double ell, double tol,
                         int max_iter) {
    const std::string who = std::string(api) + ": ";
    if (!c->res.have_train) return fail_arg((who + "no training set (call gpmi_set_train)").c_str());
    if (c->kind != 0) return fail_arg((who + "squared-exponential kernel only (gpmi_set_kernel kind 0)").c_str());
    if (own) return fail_arg((who + own).c_str());
    if (!(ell != 0.0) || !std::isfinite(ell) || !std::isfinite(sigma))
        return fail_arg((who + "ell must be non-zero and hyper-parameters finite").c_str());
    if (!(tol >= 0.0) || !std::isfinite(tol)) return fail_arg((who + "tol must be finite and >= 0").c_str());
    if (max_iter < 0) return fail_arg((who + "max_iter must be >= 0").c_str());
    return GPMI_OK;
}

int classifier_labels_check(gpmi_ctx* c, const char* api, bool (*ok)(double, int), int n_classes, const char* text) {
    std::vector<double> hy((size_t)c->N);
    HIP_TRY(hipMemcpyAsync(hy.data(), c->y.p, (size_t)c->N * 8, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
    for (double v : hy)
        if (!ok(v, n_classes)) return fail_arg((std::string(api) + ": " + text).c_str());
    return GPMI_OK;
}

int classifier_fit_begin(gpmi_ctx* c, double sigma, double ell, bool* chain) {
    c->res.drop_fit();                    // a classifier's factor replaces whatever was resident: no other state survives
    c->release_sparse_grad();
    int rc = ensure_train_buffers(c, 0, false);
    if (rc) return rc;
    c->sig2 = sigma * sigma;
    c->coef = -.5 * (1 / (ell * ell));
    c->sigma = sigma; c->ell = ell;
    *chain = tuning().panel_fused && tuning().trsv_vinv >= 2;
    if (*chain) {                         // the give-up word is read from the first iteration on
        HIP_TRY(c->flag.ensure(64));
        HIP_TRY(hipMemsetAsync(c->flag.p, 0, 64, c->stream));
    }
    HIP_TRY(hipMemcpyAsync(c->info.p, &NO_BAD_PIVOT, sizeof NO_BAD_PIVOT, hipMemcpyHostToDevice, c->stream));
    return GPMI_OK;
}

// The node count of the prediction's quadrature (mirrored in tests/laplace_ref.py).  The integrand
// expit(mu + sqrt(V) t) phi(t) is analytic in the strip |Im t| < pi / sqrt(V); with a = 0.9 pi / sqrt(V) the composite
// trapezoid rule's error is about 2 M(a) exp(a^2 / 2 - 2 pi a / h) (M(a) < 4: |expit| on the strip's edge), so
// h = 2 pi a / (36 + a^2 / 2) keeps it near 1e-15.  V* <= sigma^2, so the spacing for V = sigma^2 serves every test
// point.  h is capped at 0.25 (from a >= 8 pi on the cap holds by itself: a' = 2 pi / h inside the strip gives
// exp(-2 pi^2 / h^2)); [-T, T] = [-8.5, 8.5] drops 2 Q(8.5) < 2e-17 of the Gaussian mass.
void laplace_quad_nodes(double sig2, int* M, double* T, double* h) {
    *T = 8.5;
    double step = 0.25;
    if (sig2 > 0.0) {
        const double a = 0.9 * M_PI / std::sqrt(sig2);
        if (a < 8 * M_PI) step = std::min(0.25, 2 * M_PI * a / (36.0 + 0.5 * a * a));
    }
    const double m = std::ceil(2 * *T / step);
    *M = (int)std::min(m, 1e8);
    *h = 2 * *T / *M;
}

// Vectors of the Laplace state, Np doubles each, in c->lap: a, a_prev, f, f_prev, s, grad, b, c, then 2 Np for the
// backward solve (its right-hand side, its solution), then the Psi partials and the read-back record.
enum { LV_A, LV_AP, LV_F, LV_FP, LV_S, LV_G, LV_B, LV_C, LV_X, LV_COUNT = LV_X + 2 };

static NewtonVecs newton_vecs(gpmi_ctx* c) {
    double* L = c->lap.as<double>();
    const int64_t Np = c->Np;
    return NewtonVecs{L + LV_A * Np, L + LV_AP * Np, L + LV_F * Np, L + LV_FP * Np, L + LV_S * Np, L + LV_G * Np,
                      L + LV_B * Np};
}

// over the lower tiles of M (Np x Np, leading dimension ld): the freshly built K in A during the fit
static hipError_t launch_symv(gpmi_ctx* c, double* M, int64_t ld, bool scale, const double* x) {
    const int64_t nt = c->Np / TILE;
    const unsigned tiles = (unsigned)(nt * (nt + 1) / 2);
    double* s = c->lap.as<double>() + LV_S * c->Np;
    if (scale)
        hipLaunchKernelGGL(laplace_symv_kernel<true>, dim3(tiles), dim3(SYMV_THREADS), 0, c->stream, M, ld, nt, c->N, x, s,
                           c->lap_part.as<double>());
    else
        hipLaunchKernelGGL(laplace_symv_kernel<false>, dim3(tiles), dim3(SYMV_THREADS), 0, c->stream, M, ld, nt, c->N, x, s,
                           c->lap_part.as<double>());
    return hipGetLastError();
}

static const char* const PIVOT_TEXT = "B = I + W^1/2 K W^1/2 met a non-positive pivot";

// The binary fit as newton_iterate's problem (gpmi_state.h).  h is the last read-back record: h[0] ends as Psi(f^).
namespace {
struct LaplaceNewton {
    gpmi_ctx* c;
    bool chain;
    int64_t nblk;
    NewtonVecs v;
    RbfArgs r;                 // K into A
    double *psi_part, *rec;
    double h[3];

    int forward() {
        HIP_TRY(launch_rbf(c->stream, r));                            // 1. K
        HIP_TRY(launch_symv(c, c->A.as<double>(), c->ldA, false, v.a));   // 2. f = K a
        return GPMI_OK;
    }
    // 3., 4. Psi of the iterate, with the previous Cholesky's pivot word and backward solve's give-up word
    int evaluate(int mode, double* psi) {
        LAUNCH_TRY(laplace_newton_kernel, dim3((unsigned)nblk), dim3(VEC_THREADS), 0, c->stream, mode,
                   (const double*)c->lap_part.as<double>(), c->Np / TILE, c->N, c->Np, (const double*)c->y.as<double>(), v,
                   psi_part);
        const int rc = newton_readback(c, psi_part, nblk, chain, rec, h, "gpmi_laplace_fit", PIVOT_TEXT);
        *psi = h[0];
        return rc;
    }
    int factor(bool) {
        hipStream_t st = c->stream;
        const int64_t N = c->N, Np = c->Np;
        double* cv = c->lap.as<double>() + LV_C * Np;
        HIP_TRY(launch_symv(c, c->A.as<double>(), c->ldA, true, v.b));    // 5. u = K b, K <- B
        LAUNCH_TRY(laplace_rhs_kernel, dim3(grid_of(Np)), dim3(VEC_THREADS), 0, st, (const double*)c->lap_part.as<double>(),
                   Np / TILE, N, Np, (const double*)v.s, cv);
        HIP_TRY(launch_set_yrow(st, c->m_row(), cv, N, Np));          // 6. c rides: m = L^-1 c
        HIP_TRY(cholesky_inplace(c, c->A.as<double>(), c->ldA, Np, c->Mp, c->info.as<int64_t>(), false));
        c->res.factor_replaced(tuning().panel_fused);
        return GPMI_OK;
    }
    int step() {
        double* x = nullptr;                                          // 7. x = L^-T m, a = b - s o x
        HIP_TRY(backward_solve_resident(c, c->lap.as<double>() + LV_X * c->Np, &x));
        LAUNCH_TRY(laplace_update_kernel, dim3(grid_of(c->Np)), dim3(VEC_THREADS), 0, c->stream, c->N, c->Np,
                   (const double*)x, v);
        return GPMI_OK;
    }
};
}  // namespace

int laplace_fit_impl(gpmi_ctx* c, double sigma, double ell, double tol, int max_iter, double* log_q, int* iters,
                     int* converged, double* f_hat) {
    int rc = classifier_fit_check(c, "gpmi_laplace_fit", nullptr, sigma, ell, tol, max_iter);
    if (rc) return rc;
    if ((rc = classifier_labels_check(c, "gpmi_laplace_fit", [](double v, int) { return v == 1.0 || v == -1.0; }, 2,
                                      "labels must be exactly -1 or +1")))
        return rc;
    bool chain = false;
    if ((rc = classifier_fit_begin(c, sigma, ell, &chain)) != GPMI_OK) return rc;
    hipStream_t st = c->stream;
    const int64_t N = c->N, Np = c->Np, nt = Np / TILE;
    const int64_t nblk = (Np + VEC_THREADS - 1) / VEC_THREADS;
    HIP_TRY(c->lap.ensure(((size_t)LV_COUNT * Np + 2 * nblk + 8) * 8));
    HIP_TRY(c->lap_part.ensure((size_t)nt * nt * TILE * 8));
    double* A = c->A.as<double>();
    LaplaceNewton p;
    p.c = c; p.chain = chain; p.nblk = nblk; p.v = newton_vecs(c);
    p.psi_part = c->lap.as<double>() + LV_COUNT * Np; p.rec = p.psi_part + 2 * nblk;
    p.r = rbf_sym(c, c->x_train(), N, c->box_train(), 0.0, Np, A, c->ldA);
    HIP_TRY(hipMemsetAsync(p.v.a, 0, (size_t)Np * 8, st));
    HIP_TRY(launch_fill_rows(st, c->m_row(), c->ldA, TILE, Np, 0.0));
    int it = 0;
    bool conv = false;
    if ((rc = newton_iterate(p, tol, max_iter, &it, &conv)) != GPMI_OK) return rc;
    // log q = Psi(f^) - sum log L_ii(B(f^))  (GPML eq. 3.32 at the mode)
    HIP_TRY(launch_lml_reduce(st, A, c->ldA, c->m_row(), N, p.rec + 4));
    double red[2];
    int64_t info = 0;
    HIP_TRY(hipMemcpyAsync(red, p.rec + 4, sizeof red, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipMemcpyAsync(&info, c->info.p, sizeof info, hipMemcpyDeviceToHost, st));
    if (f_hat) HIP_TRY(hipMemcpyAsync(f_hat, p.v.f, (size_t)N * 8, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    c->timers_collect();
    if (info != NO_BAD_PIVOT) { g_err = std::string("gpmi_laplace_fit: ") + PIVOT_TEXT; return GPMI_ERR_NOT_PD; }
    if (log_q) *log_q = p.h[0] - red[0];
    if (iters) *iters = it;
    if (converged) *converged = conv ? 1 : 0;
    c->res.fit_done(Fit::Laplace);
    return GPMI_OK;
}

int laplace_predict_impl(gpmi_ctx* c, double* f_mean, double* f_var, double* prob) {
    if (!c->res.laplace()) return fail_arg("gpmi_laplace_predict: no Laplace fit resident (call gpmi_laplace_fit)");
    if (!c->res.have_test) return fail_arg("gpmi_laplace_predict: no test set (call gpmi_set_test)");
    const Tuning tn = resident_tuning(c);
    TuneScope tune_scope(&tn);
    hipStream_t st = c->stream;
    const int64_t Np = c->Np, np_ = c->np_, n = c->n;
    HIP_TRY(c->lap_out.ensure((size_t)np_ * 5 * 8));
    int rc = predict_front(c, -1);                        // R = K(X*, X)
    if (rc) return rc;
    double* V = c->V.as<double>();
    double* o = c->lap_out.as<double>();
    const double* grad = c->lap.as<double>() + LV_G * Np;
    const double* s = c->lap.as<double>() + LV_S * Np;
    LAUNCH_TRY(laplace_rows_kernel, dim3((unsigned)np_), dim3(VEC_THREADS), 0, st, V, c->ldV, Np, grad, s, o);
    HIP_TRY(solve_sweep(c, V, c->ldV, np_));                        // v^T = (R W^1/2) L^-T
    HIP_TRY(launch_row_dots(st, V, c->ldV, np_, Np, grad, o + np_, o + 2 * np_));
    int M = 0;
    double T = 0., hq = 0.;
    laplace_quad_nodes(c->sig2, &M, &T, &hq);
    LAUNCH_TRY(laplace_quad_kernel, dim3(grid_of(n)), dim3(VEC_THREADS), 0, st, n, (const double*)o,
               (const double*)(o + 2 * np_), c->sig2, M, T, hq, o + 3 * np_, o + 4 * np_);
    if (f_mean) HIP_TRY(hipMemcpyAsync(f_mean, o, (size_t)n * 8, hipMemcpyDeviceToHost, st));
    if (f_var) HIP_TRY(hipMemcpyAsync(f_var, o + 3 * np_, (size_t)n * 8, hipMemcpyDeviceToHost, st));
    if (prob) HIP_TRY(hipMemcpyAsync(prob, o + 4 * np_, (size_t)n * 8, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    c->timers_collect();
    return GPMI_OK;
}

// The gradient of log q at the resident fit (GPML Algorithm 5.1; include/gpmi.h has the formulas).  U = L^-T, kappa_i =
// [B^-1]_ii from U's rows and Kn = -B^-1 = -U U^T as the regression gradients form them; K rebuilt into U's buffer, which
// is dead by then, for t = s o (K s2); z = s2 + s o (Kn t); then the fused trace of grad.hip with the classifier's weight.
// Reads L, a, f^, s and grad only; its vectors live in loov, the tile partials in lap_part (scratch of the fit).
int laplace_grad_impl(gpmi_ctx* c, double* d_r, double* d_ell, double* d_sigma) {
    if (!c->res.laplace()) return fail_arg("gpmi_laplace_grad: no Laplace fit resident (call gpmi_laplace_fit)");
    const Tuning tn = resident_tuning(c);
    TuneScope tune_scope(&tn);
    hipStream_t st = c->stream;
    const int64_t N = c->N, Np = c->Np, nt = Np / TILE, ld = c->ldA;
    HIP_TRY(c->loov.ensure((size_t)(4 * Np + 8) * 8));
    HIP_TRY(c->lap_part.ensure((size_t)nt * nt * TILE * 8));
    size_t sp = 0;
    int rc = factor_inverse_front(c, GPMI_T_GRAD, true, nullptr, &sp);
    if (rc) return rc;
    double* kappa = c->loov.as<double>();
    double *s2 = kappa + Np, *t = s2 + Np, *z = t + Np;
    double *Kb = c->U.as<double>(), *Kn = c->Kn.as<double>();
    const double* L = c->lap.as<double>();
    const double *a = L + LV_A * Np, *f = L + LV_F * Np, *s = L + LV_S * Np, *g = L + LV_G * Np;
    HIP_TRY(launch_loo_kappa(st, Kb, ld, N, kappa));                 // U is still L^-T here
    LAUNCH_TRY(laplace_s2_kernel, dim3(grid_of(Np)), dim3(VEC_THREADS), 0, st, N, Np, (const double*)kappa, f, s2);
    HIP_TRY(launch_rbf(st, rbf_sym(c, c->x_train(), N, c->box_train(), 0.0, Np, Kb, ld)));
    HIP_TRY(launch_symv(c, Kb, ld, false, s2));
    LAUNCH_TRY(laplace_rhs_kernel, dim3(grid_of(Np)), dim3(VEC_THREADS), 0, st, (const double*)c->lap_part.as<double>(), nt,
               N, Np, s, t);
    HIP_TRY(launch_symv(c, Kn, ld, false, t));
    LAUNCH_TRY(laplace_z_kernel, dim3(grid_of(Np)), dim3(VEC_THREADS), 0, st, (const double*)c->lap_part.as<double>(), nt,
               N, Np, s, (const double*)s2, z);

    GradArdArgs ga;
    ga.Z = c->x_train(); ga.n = N; ga.d = c->d;
    ga.alpha = a; ga.Kn = Kn; ga.ld = ld; ga.coef = c->coef;
    ga.family = 0;
    ga.lap_s = s; ga.lap_z = z; ga.lap_g = g;
    std::vector<double> sums;                             // no backward solve ran: no give-up word to read
    if ((rc = grad_ard_finish(c, ga, sp, nullptr, &sums))) return rc;
    grad_ard_scale(c, ga, sums, c->ell * c->ell, d_r, d_ell, d_sigma, nullptr);
    return GPMI_OK;
}

}  // namespace gpmi
