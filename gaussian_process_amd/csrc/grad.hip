// grad.hip -- gradient of the log marginal likelihood w.r.t. the hyper-parameters of the squared-exponential
// and Matern kernels.
//
// Reference: tune_hyperparms_regression.py:31-64 (gradient_ascent):
//     l_grad   = sigma**2 * exp(-.5*sqdist/l**2) * (sqdist/l**3)            (:54)
//     l_matrix = dot(dot(alpha, alpha.T) - K_y, l_grad); l_var = .5*trace   (:55-57)
// and the commented-out sigma twin (:46-52, sigma_grad = 2*sigma*exp(...)).
// The reference forms two N x N products to read off a trace; trace(W D) with
// D symmetric is sum_ij W_ij D_ij, so one fused pass over the matrix does it:
// D_ij is recomputed from X (as in the K build), W_ij = alpha_i alpha_j - Kinv_ij
// reads Kinv once.  HBM-read bound: 8 B per element.
//
// One 128 x 128 tile per block, a column pair x 32 rows per thread, X tiles in LDS
// (d <= 32) or straight from global memory; per-block partial sums, reduced in a
// fixed order (bitwise reproducible); the host adds the per-tile partials in order.
//
// The three "recompute the kernel element from X, multiply by a weight" kernels (grad_trace_kernel, grad_ard_kernel,
// loo_dmat_kernel) take the per-element function as a compile-time family F (cov_family: 0 squared exponential,
// 1 / 2 / 3 Matern nu = 1/2, 3/2, 5/2).  For a Matern, with t = a sqrt(sq), a = -coef:
//     K / sigma^2 = P(t) e^-t,   dK/dl = sigma^2 a^2 H(t) sq / l,   dK/dz-scale_k likewise with (z_ik - z_jk)^2,
//     H(t) = -(1/t) d(P e^-t)/dt = e^-t / t,  e^-t,  (1 + t) e^-t / 3
// H_1/2 is singular at t = 0 but always multiplied by a squared difference <= sq: it is SELECTED to 0 there (duplicate
// training points), never divided.  Tile enumeration, staging, accumulators and reduction orders are the same for
// every family, and the family-0 instantiations are the code they were before the families existed.
#include <algorithm>

#include "exp_dev.h"
#include "gpmi_internal.h"

namespace gpmi {

namespace {

constexpr int RT = 128;
constexpr int GRAD_MAXD = 32;

struct GradDev {
    const double* A;        // rows: nA x d
    const double* B;        // cols: nB x d
    int64_t nA, nB;
    int d;
    int64_t row0;           // first global row of this launch (index into A and alpha_r)
    int64_t rend;           // row0 + nrows: the last tile row may reach past it, but Kinv holds nrows rows only
    int Tm, Tn;
    const double* alpha_r;  // length nA
    const double* alpha_c;  // length nB
    const double* Kinv;     // element (row0 + r, c) at Kinv[r * ld + c]
    int64_t ld;
    double kinv_sign;       // Kinv holds sign * K_y^-1 (the LAUUM product is accumulated negated)
    double coef, sig2, two_sigma, inv_l3;
    int tri;                // 1: lower tiles only (triangular enumeration), strictly-lower elements count twice
    double* partial;        // 2 doubles per block
};

// K / sigma^2 = P(t) e^-t and H(t) of Matern family F (1, 2, 3) from the squared distance; coef = -a
template <int F>
__device__ __forceinline__ void matern_kh(double coef, double sq, double& k, double& h) {
    const double t = -coef * sqrt(sq);
    const double e = exp(-t);
    if constexpr (F == 1) {
        k = e;
        h = (t > 0.0) ? e / t : 0.0;           // a select: sq == 0 (or t underflowed) contributes nothing
    } else if constexpr (F == 2) {
        k = (1.0 + t) * e;
        h = e;
    } else {
        k = ((1.0 + t) + (t * t) * (1.0 / 3.0)) * e;
        h = ((1.0 + t) * e) * (1.0 / 3.0);
    }
}

template <bool LDS, int F>
__global__ __launch_bounds__(256) void grad_trace_kernel(const GradDev p) {
    extern __shared__ __attribute__((aligned(16))) double lds[];
    __shared__ double red[2][256];
    int ti, tj;
    if (p.tri) {
        const int s = blockIdx.x;
        ti = (int)((sqrtf(8.f * (float)s + 1.f) - 1.f) * 0.5f);
        while ((ti + 1) * (ti + 2) / 2 <= s) ++ti;
        while (ti * (ti + 1) / 2 > s) --ti;
        tj = s - ti * (ti + 1) / 2;
    } else {
        ti = blockIdx.x / p.Tn;
        tj = blockIdx.x - ti * p.Tn;
    }
    const int d = p.d;
    const int64_t grow0 = p.row0 + (int64_t)ti * RT;
    const int64_t gcol0 = (int64_t)tj * RT;
    const int tid = threadIdx.x;
    double* As = lds;               // [RT][d]
    double* Bs = lds + RT * d;      // [d][RT]
    if (LDS) {
        for (int e = tid; e < RT * d; e += 256) {
            const int r = e / d, k = e - r * d;
            const int64_t ga = grow0 + r, gb = gcol0 + r;
            As[r * d + k] = (ga < p.nA) ? p.A[ga * d + k] : 0.0;
            Bs[k * RT + r] = (gb < p.nB) ? p.B[gb * d + k] : 0.0;
        }
        __syncthreads();
    }
    const int cp = tid & 63, rg = tid >> 6;
    const int64_t gc = gcol0 + 2 * cp;
    const double ac0 = (gc < p.nB) ? p.alpha_c[gc] : 0.0;
    const double ac1 = (gc + 1 < p.nB) ? p.alpha_c[gc + 1] : 0.0;
    double acc_l = 0.0, acc_s = 0.0;
    for (int r = 0; r < 32; ++r) {
        const int lr = 32 * rg + r;
        const int64_t gr = grow0 + lr;
        if (gr >= p.rend) break;                                 // wave-uniform
        double s0 = 0.0, s1 = 0.0;
        if (LDS) {
            const double* ar = &As[lr * d];
            const double* bc = &Bs[2 * cp];
            for (int k = 0; k < d; ++k) {
                const double a = ar[k];
                const double e0 = a - bc[k * RT], e1 = a - bc[k * RT + 1];
                s0 = fma(e0, e0, s0);
                s1 = fma(e1, e1, s1);
            }
        } else {
            const double* ar = p.A + gr * d;
            const double* b0 = p.B + ((gc < p.nB) ? gc : 0) * d;
            const double* b1 = p.B + ((gc + 1 < p.nB) ? gc + 1 : 0) * d;
            for (int k = 0; k < d; ++k) {
                const double a = ar[k];
                const double e0 = a - b0[k], e1 = a - b1[k];
                s0 = fma(e0, e0, s0);
                s1 = fma(e1, e1, s1);
            }
        }
        const double ar_ = p.alpha_r[gr];
        const double* kp = p.Kinv + ((int64_t)ti * RT + lr) * p.ld + gc;
        const double k0 = (gc < p.nB) ? kp[0] : 0.0;
        const double k1 = (gc + 1 < p.nB) ? kp[1] : 0.0;
        double x0, x1, h0, h1;                                   // K / sigma^2 and what multiplies sq in dK/dl
        if constexpr (F == 0) {
            x0 = exp(p.coef * s0); x1 = exp(p.coef * s1);
        } else {
            matern_kh<F>(p.coef, s0, x0, h0);
            matern_kh<F>(p.coef, s1, x1, h1);
        }
        double w0 = (gc < p.nB) ? fma(ar_, ac0, -p.kinv_sign * k0) : 0.0;
        double w1 = (gc + 1 < p.nB) ? fma(ar_, ac1, -p.kinv_sign * k1) : 0.0;
        if (p.tri) {
            // symmetric case: only elements on or below the diagonal are valid in Kinv (the GEMM
            // that produced it skips whatever lies above); strictly-lower elements count twice
            w0 *= (gc < gr) ? 2.0 : (gc == gr) ? 1.0 : 0.0;
            w1 *= (gc + 1 < gr) ? 2.0 : (gc + 1 == gr) ? 1.0 : 0.0;
        }
        // dK/dl = sigma^2 exp(.) sq / l^3 ; dK/dsigma = 2 sigma exp(.)     (Matern: sigma^2 H sq a^2 / l ; 2 sigma P e^-t)
        if constexpr (F == 0) acc_l += w0 * (p.sig2 * x0 * (s0 * p.inv_l3)) + w1 * (p.sig2 * x1 * (s1 * p.inv_l3));
        else acc_l += w0 * (p.sig2 * h0 * (s0 * p.inv_l3)) + w1 * (p.sig2 * h1 * (s1 * p.inv_l3));
        acc_s += w0 * (p.two_sigma * x0) + w1 * (p.two_sigma * x1);
    }
    red[0][tid] = acc_l;
    red[1][tid] = acc_s;
    __syncthreads();
    for (int off = 128; off > 0; off >>= 1) {
        if (tid < off) {
            red[0][tid] += red[0][tid + off];
            red[1][tid] += red[1][tid + off];
        }
        __syncthreads();
    }
    if (tid == 0) {
        p.partial[2 * (size_t)blockIdx.x] = red[0][0];
        p.partial[2 * (size_t)blockIdx.x + 1] = red[1][0];
    }
}

// ---- d + 3 traces: per-dimension lengthscales (ARD), l, sigma, noise ---------------------------------------------
// A sibling of grad_trace_kernel over the lower tiles of Kn = -K_y^-1 (the same tile enumeration, LDS staging
// and rows per thread; the thread's two columns lie 64 apart so that a wave reads both edges densely), so that gpmi_lml_grad keeps its bits.  Per element: e_k^2 = (z_ik - z_jk)^2 for the DC dimensions of this
// launch (zero beyond d), x = exp(coef * sum over ALL d of e_k^2), then
//     acc_k += w x e_k^2,   acc_l += w x sq,   acc_s += w x,   acc_n += w on the diagonal
// with w = alpha_i alpha_j - K_y^-1_ij, strictly-lower elements counted twice (a Matern family: x = H(t) in acc_k and
// acc_l, x = P(t) e^-t in acc_s).  The accumulators are indexed by
// compile-time constants only (every loop over them is unrolled), so they live in registers.  Block partials go out
// component-major (partial[j * nblk + block]) and are summed by ard_reduce_kernel in a fixed order.
struct ArdDev {
    const double* Z;
    int64_t n;
    int d, k0;              // this launch covers dimensions k0 .. k0 + DC
    const double* alpha;
    const double* Kn;
    int64_t ld;
    double coef;
    double* partial;
    int64_t nblk;
};
// The binary classifier's variant (gpmi_laplace_grad): alpha is a, Kn is -B^-1 and the weight of element (i, j) is
//     w = a_i a_j + s_i s_j Kn_ij + z_i g_j + z_j g_i
// -- four more vector loads per row and per column, two more multiplications and two more FMAs per element, no noise sum
// (its slot is written 0).
// A separate instantiation (LAP, family 0 only) with its own argument block: the regression instantiations are the code
// they were.
struct ArdLapDev : ArdDev {
    const double* s;
    const double* z;
    const double* g;
};
template <bool LAP> struct ArdDevOf { typedef ArdDev type; };
template <> struct ArdDevOf<true> { typedef ArdLapDev type; };

template <int DC, bool LDS, int F, bool LAP = false>
__global__ __launch_bounds__(256) void grad_ard_kernel(const typename ArdDevOf<LAP>::type p) {
    extern __shared__ __attribute__((aligned(16))) double lds[];
    __shared__ double red[4][DC + 3];
    const int s = blockIdx.x;
    int ti = (int)((sqrtf(8.f * (float)s + 1.f) - 1.f) * 0.5f);
    while ((ti + 1) * (ti + 2) / 2 <= s) ++ti;
    while (ti * (ti + 1) / 2 > s) --ti;
    const int tj = s - ti * (ti + 1) / 2;
    const int d = p.d;
    const int64_t grow0 = (int64_t)ti * RT, gcol0 = (int64_t)tj * RT;
    const int tid = threadIdx.x;
    double* As = lds;               // [RT][DC]
    double* Bs = lds + RT * DC;     // [DC][RT]
    if (LDS) {                      // d <= DC, k0 == 0: dimensions d .. DC are zero on both edges
        for (int e = tid; e < RT * DC; e += 256) {
            const int r = e / DC, k = e - r * DC;
            const int64_t ga = grow0 + r, gb = gcol0 + r;
            As[r * DC + k] = (k < d && ga < p.n) ? p.Z[ga * d + k] : 0.0;
            Bs[k * RT + r] = (k < d && gb < p.n) ? p.Z[gb * d + k] : 0.0;
        }
        __syncthreads();
    }
    const int cp = tid & 63, rg = tid >> 6;
    const int64_t gc = gcol0 + cp;      // the thread's columns: gc and gc + 64 (dense LDS and Kn reads across the wave)
    double acc[DC];
#pragma unroll
    for (int k = 0; k < DC; ++k) acc[k] = 0.0;
    double acc_l = 0.0, acc_s = 0.0, acc_n = 0.0;
    for (int r = 0; r < 32; ++r) {
        const int lr = 32 * rg + r;
        const int64_t gr = grow0 + lr;
        if (gr >= p.n) break;                                    // wave-uniform
        const double ar_ = p.alpha[gr];
        const double* kp = p.Kn + gr * p.ld + gc;
        double sr_ = 0.0, zr_ = 0.0, gr_ = 0.0;
        if constexpr (LAP) { sr_ = p.s[gr]; zr_ = p.z[gr]; gr_ = p.g[gr]; }
#pragma unroll
        for (int c = 0; c < 2; ++c) {                            // the thread's two columns, one after the other
            const int64_t g = gc + 64 * c;
            const bool in = g < p.n;
            double e2[DC];
            double sq = 0.0;
            if (LDS) {
                const double* ar = &As[lr * DC];
                const double* bc = &Bs[cp + 64 * c];
#pragma unroll
                for (int k = 0; k < DC; ++k) {
                    const double e = ar[k] - bc[k * RT];
                    e2[k] = e * e;
                    sq += e2[k];
                }
            } else {
                const double* ar = p.Z + gr * d;
                const double* b = p.Z + (in ? g : 0) * d;
#pragma unroll
                for (int k = 0; k < DC; ++k) {
                    const int kk = p.k0 + k;
                    const double e = (kk < d) ? ar[kk] - b[kk] : 0.0;
                    e2[k] = e * e;
                    sq += e2[k];
                }
                for (int kk = 0; kk < p.k0; ++kk) {
                    const double e = ar[kk] - b[kk];
                    sq = fma(e, e, sq);
                }
                for (int kk = p.k0 + DC; kk < d; ++kk) {
                    const double e = ar[kk] - b[kk];
                    sq = fma(e, e, sq);
                }
            }
            // Kn holds -K_y^-1, valid on and below the diagonal only
            double w;
            if constexpr (LAP) {
                w = 0.0;
                if (in && g <= gr) {
                    w = fma(ar_, p.alpha[g], (sr_ * p.s[g]) * kp[64 * c]);
                    w = fma(zr_, p.g[g], w);
                    w = fma(p.z[g], gr_, w);
                }
                if (g != gr) w += w;
            } else {
                w = (in && g <= gr) ? fma(ar_, p.alpha[g], kp[64 * c]) : 0.0;
                if (g == gr) acc_n += w;
                else w += w;
            }
            double wx, ws;                                       // the weight of the lengthscale sums and of sigma's
            if constexpr (F == 0) {
                wx = ws = w * exp(p.coef * sq);
            } else {
                double kk, hh;
                matern_kh<F>(p.coef, sq, kk, hh);
                wx = w * hh;
                ws = w * kk;
            }
#pragma unroll
            for (int k = 0; k < DC; ++k) acc[k] = fma(wx, e2[k], acc[k]);
            acc_l = fma(wx, sq, acc_l);
            acc_s += ws;
        }
    }
    // 64 lanes by a butterfly, then the four waves in order: the same order every run
    const int wave = tid >> 6;
    auto wave_sum = [](double v) {
#pragma unroll
        for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off, 64);
        return v;
    };
#pragma unroll
    for (int k = 0; k < DC; ++k) {
        const double v = wave_sum(acc[k]);
        if (cp == 0) red[wave][k] = v;
    }
    {
        const double vl = wave_sum(acc_l), vs = wave_sum(acc_s), vn = wave_sum(acc_n);
        if (cp == 0) { red[wave][DC] = vl; red[wave][DC + 1] = vs; red[wave][DC + 2] = vn; }
    }
    __syncthreads();
    if (tid < DC + 3)
        p.partial[(int64_t)tid * p.nblk + blockIdx.x] = ((red[0][tid] + red[1][tid]) + red[2][tid]) + red[3][tid];
}

// out[j] = sum over the blocks of partial[j * nblk + b]: thread t adds blocks t, t + 256, ... in order, then a fixed tree
__global__ __launch_bounds__(256) void ard_reduce_kernel(const double* partial, int64_t nblk, double* out) {
    __shared__ double sh[256];
    const double* in = partial + (int64_t)blockIdx.x * nblk;
    double v = 0.0;
    for (int64_t b = threadIdx.x; b < nblk; b += 256) v += in[b];
    sh[threadIdx.x] = v;
    __syncthreads();
    for (int off = 128; off > 0; off >>= 1) {
        if ((int)threadIdx.x < off) sh[threadIdx.x] += sh[threadIdx.x + off];
        __syncthreads();
    }
    if (threadIdx.x == 0) out[blockIdx.x] = sh[0];
}

// ---- 11 basis sums of the CO2 composite kernel (kind 3; CO2_example.py:9-64) ----------------------------------------
// A sibling of grad_ard_kernel: the same lower-tile enumeration over Kn = -K_y^-1, the same columns and rows per thread,
// the same weight w = alpha_i alpha_j + Kn_ij (strictly-lower elements twice), the same reduction orders and
// ard_reduce_kernel behind it.  Per element, with sq the squared distance and r = sqrt(sq):
//     e1 = exp(n1 sq)   s2 = sin^2(pi r)   q2 = exp(n4 sq + n5 s2)   u = cu sq   p3 = exp(n8 log1p(u))   e4 = exp(n10 sq)
//     S1 += w e1   S2 += w e1 sq   S3 += w q2   S4 += w q2 sq   S5 += w q2 s2
//     S6 += w p3   S7 += w p3 sq / (1 + u)   S8 += w p3 (u / (1 + u) - log1p(u))   S9 += w e4   S10 += w e4 sq
//     S11 += w on the diagonal
// The six constants come from the host (regress.hip: lml_grad_co2_impl), which also turns the sums into the twelve
// derivatives.  Every term is regular at sq == 0 (e1 = 1, s2 = 0, u = 0): nothing is selected on the diagonal or for
// duplicate points.  LDS: d <= GRAD_MAXD, both tile edges staged as in grad_trace_kernel; beyond, X comes from global
// memory.  Accumulators are named by compile-time constants only.
constexpr int CO2_NS = 11;

struct Co2Dev {
    const double* Z;
    int64_t n;
    int d;
    const double* alpha;
    const double* Kn;
    int64_t ld;
    double n1, n4, n5, cu, n8, n10;
    double* partial;
    int64_t nblk;
};

template <bool LDS>
__global__ __launch_bounds__(256) void grad_co2_kernel(const Co2Dev p) {
    extern __shared__ __attribute__((aligned(16))) double lds[];
    __shared__ double red[4][CO2_NS];
    const int s = blockIdx.x;
    int ti = (int)((sqrtf(8.f * (float)s + 1.f) - 1.f) * 0.5f);
    while ((ti + 1) * (ti + 2) / 2 <= s) ++ti;
    while (ti * (ti + 1) / 2 > s) --ti;
    const int tj = s - ti * (ti + 1) / 2;
    const int d = p.d;
    const int64_t grow0 = (int64_t)ti * RT, gcol0 = (int64_t)tj * RT;
    const int tid = threadIdx.x;
    double* As = lds;               // [RT][d]
    double* Bs = lds + RT * d;      // [d][RT]
    if (LDS) {
        for (int e = tid; e < RT * d; e += 256) {
            const int r = e / d, k = e - r * d;
            const int64_t ga = grow0 + r, gb = gcol0 + r;
            As[r * d + k] = (ga < p.n) ? p.Z[ga * d + k] : 0.0;
            Bs[k * RT + r] = (gb < p.n) ? p.Z[gb * d + k] : 0.0;
        }
        __syncthreads();
    }
    const int cp = tid & 63, rg = tid >> 6;
    const int64_t gc = gcol0 + cp;      // the thread's columns: gc and gc + 64
    double acc[CO2_NS];
#pragma unroll
    for (int k = 0; k < CO2_NS; ++k) acc[k] = 0.0;
    for (int r = 0; r < 32; ++r) {
        const int lr = 32 * rg + r;
        const int64_t gr = grow0 + lr;
        if (gr >= p.n) break;                                    // wave-uniform
        const double ar_ = p.alpha[gr];
        const double* kp = p.Kn + gr * p.ld + gc;
#pragma unroll
        for (int c = 0; c < 2; ++c) {
            const int64_t g = gc + 64 * c;
            const bool in = g < p.n;
            double sq = 0.0;
            if (LDS) {
                const double* ar = &As[lr * d];
                const double* bc = &Bs[cp + 64 * c];
                for (int k = 0; k < d; ++k) {
                    const double e = ar[k] - bc[k * RT];
                    sq = fma(e, e, sq);
                }
            } else {
                const double* ar = p.Z + gr * d;
                const double* b = p.Z + (in ? g : 0) * d;
                for (int k = 0; k < d; ++k) {
                    const double e = ar[k] - b[k];
                    sq = fma(e, e, sq);
                }
            }
            // Kn holds -K_y^-1, valid on and below the diagonal only
            double w = (in && g <= gr) ? fma(ar_, p.alpha[g], kp[64 * c]) : 0.0;
            if (g == gr) acc[10] += w;
            else w += w;
            const double sn = sin(M_PI * sqrt(sq));
            const double s2 = sn * sn;
            const double u = p.cu * sq;
            const double l1p = log1p(u);
            const double rc = 1.0 / (1.0 + u);
            const double w1 = w * exp(p.n1 * sq);
            const double w2 = w * exp(fma(p.n4, sq, p.n5 * s2));
            const double w3 = w * exp(p.n8 * l1p);
            const double w4 = w * exp(p.n10 * sq);
            acc[0] += w1;
            acc[1] = fma(w1, sq, acc[1]);
            acc[2] += w2;
            acc[3] = fma(w2, sq, acc[3]);
            acc[4] = fma(w2, s2, acc[4]);
            acc[5] += w3;
            acc[6] = fma(w3, sq * rc, acc[6]);
            acc[7] = fma(w3, u * rc - l1p, acc[7]);
            acc[8] += w4;
            acc[9] = fma(w4, sq, acc[9]);
        }
    }
    // 64 lanes by a butterfly, then the four waves in order: the same order every run
    const int wave = tid >> 6;
#pragma unroll
    for (int k = 0; k < CO2_NS; ++k) {
        double v = acc[k];
#pragma unroll
        for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off, 64);
        if (cp == 0) red[wave][k] = v;
    }
    __syncthreads();
    if (tid < CO2_NS)
        p.partial[(int64_t)tid * p.nblk + blockIdx.x] = ((red[0][tid] + red[1][tid]) + red[2][tid]) + red[3][tid];
}

__global__ void scale_inputs_kernel(const double* X, const double* r, int64_t total, int d, double* Z) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < total) Z[i] = X[i] / r[i % d];
}

__global__ void set_identity_kernel(double* V, int64_t ld, int64_t n) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) V[i * ld + i] = 1.0;
}

// ---- leave-one-out cross-validation (GPML section 5.4.2) ------------------------------------------------------------
// Small N^2 passes around the N^3 products of gpmi_loo / gpmi_loo_grad (regress.hip).  The row kernels give one wave a
// row: lane t reads the column pairs 2t, 2t + 128, ... with 16-byte loads (a wave reads 1 KiB per instruction) and adds
// them in that order, the 64 lanes meet in a butterfly -- the same order every run.  They read rows and columns < n
// only: whatever the identity padding holds contributes nothing.
typedef double dbl2 __attribute__((ext_vector_type(2)));

__device__ __forceinline__ double wave_sum64(double v) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off, 64);
    return v;
}

// kappa_i = sum_{j >= i} U_ij^2: the diagonal of K_y^-1 = U U^T, U = L^-T upper triangular
__global__ __launch_bounds__(256) void loo_kappa_kernel(const double* __restrict__ U, int64_t ld, int64_t n,
                                                        double* __restrict__ kappa) {
    const int lane = threadIdx.x & 63;
    const int64_t i = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (i >= n) return;                                          // wave-uniform
    const double* row = U + i * ld;
    double acc = 0.0;
#pragma unroll 4
    for (int64_t j = (i & ~(int64_t)1) + 2 * lane; j < n; j += 128) {
        const dbl2 v = *reinterpret_cast<const dbl2*>(row + j);
        const double a = (j >= i) ? v.x : 0.0, b = (j + 1 < n) ? v.y : 0.0;
        acc = fma(a, a, acc);
        acc = fma(b, b, acc);
    }
    acc = wave_sum64(acc);
    if (lane == 0) kappa[i] = acc;
}

__global__ __launch_bounds__(256) void loo_points_kernel(const double* __restrict__ y, const double* __restrict__ alpha,
                                                         const double* __restrict__ kappa, int64_t n, double* __restrict__ mu,
                                                         double* __restrict__ var, double* __restrict__ logp) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const double k = kappa[i], yi = y[i];
    const double v = 1.0 / k, m = yi - alpha[i] / k, e = yi - m;
    mu[i] = m;
    var[i] = v;
    logp[i] = -.5 * log(v) - e * e / (2.0 * v) - 0.91893853320467274178;      // .5 log(2 pi)
}

// upper(i < j) <- lower(j, i), 64 x 64 tiles transposed through LDS (rows padded by one double: a wave's column read
// touches every bank pair once per 32 lanes)
__global__ __launch_bounds__(256) void mirror_lower_kernel(double* A, int64_t ld) {
    __shared__ double tile[64][65];
    const int ti = blockIdx.y, tj = blockIdx.x;
    if (tj > ti) return;
    const int c = threadIdx.x & 63, r0 = threadIdx.x >> 6;
    const double* src = A + ((int64_t)ti * 64) * ld + (int64_t)tj * 64;
    for (int r = r0; r < 64; r += 4) tile[r][c] = src[(int64_t)r * ld + c];
    __syncthreads();
    double* dst = A + ((int64_t)tj * 64) * ld + (int64_t)ti * 64;
    for (int r = r0; r < 64; r += 4)
        if (ti != tj || c > r) dst[(int64_t)r * ld + c] = tile[c][r];
}

// D_ab = K_ab sq_ab = sig2 exp(coef sq_ab) sq_ab in full (dK/dl = D / l^3; a Matern family: D_ab = sig2 H(t_ab) sq_ab,
// dK/dl = a^2 D / l, with the library exp), zero on padded rows and columns.  The tile
// loop, the staging and the squared distance of grad_trace_kernel; exp by the K build's polynomial while every lane of
// the wave is inside its domain.  D_ab and D_ba are the same bits ((a - b)^2 == (b - a)^2, the same order over k).
struct DmatDev {
    const double* Z;
    int64_t n;
    int d;
    double coef, sig2;
    double* D;
    int64_t ld;
};

template <bool LDS, int F>
__global__ __launch_bounds__(256) void loo_dmat_kernel(const DmatDev p) {
    extern __shared__ __attribute__((aligned(16))) double lds[];
    const int ti = blockIdx.y, tj = blockIdx.x;
    const int d = p.d;
    const int64_t grow0 = (int64_t)ti * RT, gcol0 = (int64_t)tj * RT;
    const int tid = threadIdx.x;
    double* As = lds;               // [RT][d]
    double* Bs = lds + RT * d;      // [d][RT]
    if (LDS) {
        for (int e = tid; e < RT * d; e += 256) {
            const int r = e / d, k = e - r * d;
            const int64_t ga = grow0 + r, gb = gcol0 + r;
            As[r * d + k] = (ga < p.n) ? p.Z[ga * d + k] : 0.0;
            Bs[k * RT + r] = (gb < p.n) ? p.Z[gb * d + k] : 0.0;
        }
        __syncthreads();
    }
    const int cp = tid & 63, rg = tid >> 6;
    const int64_t gc = gcol0 + 2 * cp;
    const bool in0 = gc < p.n, in1 = gc + 1 < p.n;
    for (int r = 0; r < 32; ++r) {
        const int lr = 32 * rg + r;
        const int64_t gr = grow0 + lr;
        const bool inr = gr < p.n;                               // wave-uniform
        double s0 = 0.0, s1 = 0.0;
        if (LDS) {
            const double* ar = &As[lr * d];
            const double* bc = &Bs[2 * cp];
            for (int k = 0; k < d; ++k) {
                const double a = ar[k];
                const double e0 = a - bc[k * RT], e1 = a - bc[k * RT + 1];
                s0 = fma(e0, e0, s0);
                s1 = fma(e1, e1, s1);
            }
        } else {
            const double* ar = p.Z + (inr ? gr : 0) * d;
            const double* b0 = p.Z + (in0 ? gc : 0) * d;
            const double* b1 = p.Z + (in1 ? gc + 1 : 0) * d;
            for (int k = 0; k < d; ++k) {
                const double a = ar[k];
                const double e0 = a - b0[k], e1 = a - b1[k];
                s0 = fma(e0, e0, s0);
                s1 = fma(e1, e1, s1);
            }
        }
        double e0, e1;
        if constexpr (F == 0) {
            const double x0 = p.coef * s0, x1 = p.coef * s1;
            const bool ok = (x0 >= -700.0) & (x0 <= 0.0) & (x1 >= -700.0) & (x1 <= 0.0);
            if (__builtin_amdgcn_ballot_w64(!ok) == 0) {
                e0 = exp_neg_fast(x0);
                e1 = exp_neg_fast(x1);
            } else {
                e0 = exp(x0);
                e1 = exp(x1);
            }
        } else {
            double k0, k1;
            matern_kh<F>(p.coef, s0, k0, e0);                    // e = H(t): D = sig2 H sq
            matern_kh<F>(p.coef, s1, k1, e1);
        }
        dbl2 v;
        v.x = (inr && in0) ? (p.sig2 * e0) * s0 : 0.0;
        v.y = (inr && in1) ? (p.sig2 * e1) * s1 : 0.0;
        *reinterpret_cast<dbl2*>(p.D + gr * p.ld + gc) = v;
    }
}

// per row i < n: sq_i = sum_j M_ij^2, d0_i = sum_j M_ij x0_j, d1_i = sum_j M_ij x1_j (FULL), or d0 alone
template <bool FULL>
__global__ __launch_bounds__(256) void row_pass_kernel(const double* __restrict__ M, int64_t ld, int64_t n,
                                                       const double* __restrict__ x0, const double* __restrict__ x1,
                                                       double* __restrict__ sq, double* __restrict__ d0, double* __restrict__ d1) {
    const int lane = threadIdx.x & 63;
    const int64_t i = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (i >= n) return;                                          // wave-uniform
    const double* row = M + i * ld;
    double as = 0.0, a0 = 0.0, a1 = 0.0;
#pragma unroll 4
    for (int64_t j = 2 * lane; j < n; j += 128) {
        const bool in1 = j + 1 < n;
        const dbl2 m = *reinterpret_cast<const dbl2*>(row + j);
        const dbl2 u = *reinterpret_cast<const dbl2*>(x0 + j);
        const double my = in1 ? m.y : 0.0;
        a0 = fma(m.x, u.x, a0);
        a0 = fma(my, in1 ? u.y : 0.0, a0);
        if (FULL) {
            const dbl2 w = *reinterpret_cast<const dbl2*>(x1 + j);
            as = fma(m.x, m.x, as);
            as = fma(my, my, as);
            a1 = fma(m.x, w.x, a1);
            a1 = fma(my, in1 ? w.y : 0.0, a1);
        }
    }
    a0 = wave_sum64(a0);
    if (FULL) { as = wave_sum64(as); a1 = wave_sum64(a1); }
    if (lane == 0) {
        d0[i] = a0;
        if (FULL) { sq[i] = as; d1[i] = a1; }
    }
}

// out_i = sum_{j < n} C_ij B_ij
__global__ __launch_bounds__(256) void row_dot2_kernel(const double* __restrict__ C, int64_t ldc, const double* __restrict__ B,
                                                       int64_t ldb, int64_t nrows, int64_t n, double* __restrict__ out) {
    const int lane = threadIdx.x & 63;
    const int64_t i = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (i >= nrows) return;                                      // wave-uniform
    const double* c = C + i * ldc;
    const double* b = B + i * ldb;
    double acc = 0.0;
#pragma unroll 4
    for (int64_t j = 2 * lane; j < n; j += 128) {
        const dbl2 u = *reinterpret_cast<const dbl2*>(c + j);
        const dbl2 v = *reinterpret_cast<const dbl2*>(b + j);
        acc = fma(u.x, v.x, acc);
        acc = fma((j + 1 < n) ? u.y : 0.0, (j + 1 < n) ? v.y : 0.0, acc);
    }
    acc = wave_sum64(acc);
    if (lane == 0) out[i] = acc;
}

// block 0: l, block 1: sigma, block 2: noise (gpmi_internal.h: LooGradArgs).  Thread t adds points t, t + 256, ... in
// order, then a fixed tree.
__global__ __launch_bounds__(256) void loo_grad_sums_kernel(const LooGradArgs p) {
    __shared__ double sh[256];
    const int comp = blockIdx.x;
    double acc = 0.0;
    for (int64_t i = threadIdx.x; i < p.n; i += 256) {
        const double a = p.alpha[i], k = p.kappa[i];
        double r, s;
        if (comp == 0) { r = -p.un[i]; s = -p.sn[i]; }
        else if (comp == 1) { r = a + p.noise * p.qn[i]; s = k - p.noise * p.cn[i]; }
        else { r = -p.qn[i]; s = p.cn[i]; }
        acc += (a * r - .5 * (1.0 + a * a / k) * s) / k;
    }
    sh[threadIdx.x] = acc;
    __syncthreads();
    for (int off = 128; off > 0; off >>= 1) {
        if ((int)threadIdx.x < off) sh[threadIdx.x] += sh[threadIdx.x + off];
        __syncthreads();
    }
    if (threadIdx.x == 0) p.out3[comp] = sh[0];
}

}  // namespace

hipError_t launch_set_identity_diag(hipStream_t s, double* V, int64_t ld, int64_t n) {
    if (n <= 0) return hipSuccess;
    hipLaunchKernelGGL(set_identity_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, V, ld, n);
    return hipGetLastError();
}

hipError_t launch_scale_inputs(hipStream_t s, const double* X, const double* r, int64_t n, int64_t d, double* Z) {
    const int64_t total = n * d;
    if (total <= 0) return hipSuccess;
    hipLaunchKernelGGL(scale_inputs_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, s, X, r, total, (int)d, Z);
    return hipGetLastError();
}

int64_t grad_ard_blocks(const GradArdArgs& a) {
    const int64_t T = (a.n + RT - 1) / RT;
    return T * (T + 1) / 2;
}
// dimensions per launch: the narrowest of 4 / 8 / 16 / 32 that holds d, 32 beyond
int64_t grad_ard_width(const GradArdArgs& a) { return a.d <= 4 ? 4 : a.d <= 8 ? 8 : a.d <= 16 ? 16 : 32; }
int64_t grad_ard_launches(const GradArdArgs& a) { return a.d <= GRAD_MAXD ? 1 : (a.d + GRAD_MAXD - 1) / GRAD_MAXD; }

template <int DC, int F>
static void grad_ard_go(hipStream_t s, const ArdDev& p) {
    hipLaunchKernelGGL((grad_ard_kernel<DC, true, F>), dim3((unsigned)p.nblk), dim3(256), (size_t)2 * RT * DC * sizeof(double), s, p);
}

template <int DC>
static void laplace_ard_go(hipStream_t s, const ArdLapDev& p) {
    hipLaunchKernelGGL((grad_ard_kernel<DC, true, 0, true>), dim3((unsigned)p.nblk), dim3(256), (size_t)2 * RT * DC * sizeof(double), s, p);
}

static void laplace_ard_launch(hipStream_t s, const ArdLapDev& p, int64_t d, int w) {
    if (d > GRAD_MAXD) hipLaunchKernelGGL((grad_ard_kernel<32, false, 0, true>), dim3((unsigned)p.nblk), dim3(256), 0, s, p);
    else if (w == 4) laplace_ard_go<4>(s, p);
    else if (w == 8) laplace_ard_go<8>(s, p);
    else if (w == 16) laplace_ard_go<16>(s, p);
    else laplace_ard_go<32>(s, p);
}

template <int F>
static void grad_ard_launch(hipStream_t s, const ArdDev& p, int64_t d, int w) {
    if (d > GRAD_MAXD) hipLaunchKernelGGL((grad_ard_kernel<32, false, F>), dim3((unsigned)p.nblk), dim3(256), 0, s, p);
    else if (w == 4) grad_ard_go<4, F>(s, p);
    else if (w == 8) grad_ard_go<8, F>(s, p);
    else if (w == 16) grad_ard_go<16, F>(s, p);
    else grad_ard_go<32, F>(s, p);
}

hipError_t launch_grad_ard(hipStream_t s, const GradArdArgs& a) {
    if (a.n <= 0 || a.d <= 0) return hipSuccess;
    if (a.family < 0 || a.family > 3) return hipErrorInvalidValue;
    const bool lap = a.lap_s != nullptr;
    if (lap && (a.family != 0 || !a.lap_z || !a.lap_g)) return hipErrorInvalidValue;
    ArdLapDev p;
    p.Z = a.Z; p.n = a.n; p.d = (int)a.d; p.alpha = a.alpha; p.Kn = a.Kn; p.ld = a.ld; p.coef = a.coef;
    p.partial = a.partial; p.nblk = grad_ard_blocks(a);
    p.s = a.lap_s; p.z = a.lap_z; p.g = a.lap_g;
    const int w = (int)grad_ard_width(a);
    const int64_t nl = grad_ard_launches(a);
    for (int64_t q = 0; q < nl; ++q) {       // d > 32: every launch recomputes the whole squared distance and reads Kn again
        p.k0 = (int)(q * GRAD_MAXD);
        if (lap) laplace_ard_launch(s, p, a.d, w);
        else switch (a.family) {
            case 0: grad_ard_launch<0>(s, p, a.d, w); break;
            case 1: grad_ard_launch<1>(s, p, a.d, w); break;
            case 2: grad_ard_launch<2>(s, p, a.d, w); break;
            default: grad_ard_launch<3>(s, p, a.d, w); break;
        }
        hipError_t e = hipGetLastError();
        if (e != hipSuccess) return e;
        hipLaunchKernelGGL(ard_reduce_kernel, dim3((unsigned)(w + 3)), dim3(256), 0, s, a.partial, p.nblk, a.sums + q * (w + 3));
        if ((e = hipGetLastError()) != hipSuccess) return e;
    }
    return hipSuccess;
}

int64_t grad_co2_blocks(const GradCo2Args& a) {
    const int64_t T = (a.n + RT - 1) / RT;
    return T * (T + 1) / 2;
}

hipError_t launch_grad_co2(hipStream_t s, const GradCo2Args& a) {
    if (a.n <= 0 || a.d <= 0) return hipSuccess;
    Co2Dev p;
    p.Z = a.Z; p.n = a.n; p.d = (int)a.d; p.alpha = a.alpha; p.Kn = a.Kn; p.ld = a.ld;
    p.n1 = a.n1; p.n4 = a.n4; p.n5 = a.n5; p.cu = a.cu; p.n8 = a.n8; p.n10 = a.n10;
    p.partial = a.partial; p.nblk = grad_co2_blocks(a);
    const dim3 grid((unsigned)p.nblk), block(256);
    if (a.d <= GRAD_MAXD) hipLaunchKernelGGL(grad_co2_kernel<true>, grid, block, (size_t)2 * RT * a.d * sizeof(double), s, p);
    else hipLaunchKernelGGL(grad_co2_kernel<false>, grid, block, 0, s, p);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(ard_reduce_kernel, dim3(CO2_NS), dim3(256), 0, s, a.partial, p.nblk, a.sums);
    return hipGetLastError();
}

int64_t grad_trace_blocks(const GradArgs& a) {
    const int64_t Tm = (a.nrows + RT - 1) / RT, Tn = (a.nB + RT - 1) / RT;
    return a.tri ? Tm * (Tm + 1) / 2 : Tm * Tn;
}

hipError_t launch_grad_trace(hipStream_t s, const GradArgs& a) {
    if (a.nrows <= 0 || a.nB <= 0) return hipSuccess;
    GradDev p;
    p.A = a.A; p.B = a.B; p.nA = a.nA; p.nB = a.nB; p.d = (int)a.d; p.row0 = a.row0;
    p.rend = std::min(a.row0 + a.nrows, a.nA);
    p.Tm = (int)((a.nrows + RT - 1) / RT); p.Tn = (int)((a.nB + RT - 1) / RT);
    p.alpha_r = a.alpha_r; p.alpha_c = a.alpha_c;
    p.Kinv = a.Kinv; p.ld = a.ld; p.kinv_sign = a.kinv_sign;
    p.coef = a.coef; p.sig2 = a.sig2; p.two_sigma = a.two_sigma; p.inv_l3 = a.inv_l3;
    p.tri = a.tri; p.partial = a.partial;
    if (a.family < 0 || a.family > 3) return hipErrorInvalidValue;
    const dim3 grid((unsigned)grad_trace_blocks(a)), block(256);
    const size_t lds = (size_t)2 * RT * a.d * sizeof(double);
#define GRAD_TRACE_FAMILY(FF)                                                                                          \
    if (a.d <= GRAD_MAXD) hipLaunchKernelGGL((grad_trace_kernel<true, FF>), grid, block, lds, s, p);                   \
    else hipLaunchKernelGGL((grad_trace_kernel<false, FF>), grid, block, 0, s, p)
    switch (a.family) {
        case 0: GRAD_TRACE_FAMILY(0); break;
        case 1: GRAD_TRACE_FAMILY(1); break;
        case 2: GRAD_TRACE_FAMILY(2); break;
        default: GRAD_TRACE_FAMILY(3); break;
    }
#undef GRAD_TRACE_FAMILY
    return hipGetLastError();
}

hipError_t launch_loo_kappa(hipStream_t s, const double* U, int64_t ld, int64_t n, double* kappa) {
    if (n <= 0) return hipSuccess;
    hipLaunchKernelGGL(loo_kappa_kernel, dim3((unsigned)((n + 3) / 4)), dim3(256), 0, s, U, ld, n, kappa);
    return hipGetLastError();
}

hipError_t launch_loo_points(hipStream_t s, const double* y, const double* alpha, const double* kappa, int64_t n,
                             double* mu, double* var, double* logp, double* sum) {
    if (n <= 0) return hipSuccess;
    hipLaunchKernelGGL(loo_points_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, y, alpha, kappa, n, mu, var, logp);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(ard_reduce_kernel, dim3(1), dim3(256), 0, s, logp, n, sum);
    return hipGetLastError();
}

hipError_t launch_mirror_lower(hipStream_t s, double* A, int64_t ld, int64_t np) {
    if (np <= 0) return hipSuccess;
    const unsigned T = (unsigned)(np / 64);
    hipLaunchKernelGGL(mirror_lower_kernel, dim3(T, T), dim3(256), 0, s, A, ld);
    return hipGetLastError();
}

hipError_t launch_loo_dmat(hipStream_t s, const double* Z, int64_t n, int64_t d, double coef, double sig2, int family,
                           double* D, int64_t ld, int64_t np) {
    if (np <= 0 || d <= 0) return hipSuccess;
    if (family < 0 || family > 3) return hipErrorInvalidValue;
    DmatDev p;
    p.Z = Z; p.n = n; p.d = (int)d; p.coef = coef; p.sig2 = sig2; p.D = D; p.ld = ld;
    const unsigned T = (unsigned)(np / RT);
#define LOO_DMAT_FAMILY(FF)                                                                                            \
    if (d <= GRAD_MAXD) hipLaunchKernelGGL((loo_dmat_kernel<true, FF>), dim3(T, T), dim3(256), (size_t)2 * RT * d * sizeof(double), s, p); \
    else hipLaunchKernelGGL((loo_dmat_kernel<false, FF>), dim3(T, T), dim3(256), 0, s, p)
    switch (family) {
        case 0: LOO_DMAT_FAMILY(0); break;
        case 1: LOO_DMAT_FAMILY(1); break;
        case 2: LOO_DMAT_FAMILY(2); break;
        default: LOO_DMAT_FAMILY(3); break;
    }
#undef LOO_DMAT_FAMILY
    return hipGetLastError();
}

hipError_t launch_row_pass(hipStream_t s, const double* M, int64_t ld, int64_t n, const double* x0, const double* x1,
                           double* sq, double* d0, double* d1) {
    if (n <= 0) return hipSuccess;
    const dim3 grid((unsigned)((n + 3) / 4)), block(256);
    if (x1) hipLaunchKernelGGL(row_pass_kernel<true>, grid, block, 0, s, M, ld, n, x0, x1, sq, d0, d1);
    else hipLaunchKernelGGL(row_pass_kernel<false>, grid, block, 0, s, M, ld, n, x0, x1, sq, d0, d1);
    return hipGetLastError();
}

hipError_t launch_row_dot2(hipStream_t s, const double* C, int64_t ldc, const double* B, int64_t ldb, int64_t nrows,
                           int64_t n, double* out) {
    if (nrows <= 0 || n <= 0) return hipSuccess;
    hipLaunchKernelGGL(row_dot2_kernel, dim3((unsigned)((nrows + 3) / 4)), dim3(256), 0, s, C, ldc, B, ldb, nrows, n, out);
    return hipGetLastError();
}

hipError_t launch_loo_grad_sums(hipStream_t s, const LooGradArgs& a) {
    if (a.n <= 0) return hipSuccess;
    hipLaunchKernelGGL(loo_grad_sums_kernel, dim3(3), dim3(256), 0, s, a);
    return hipGetLastError();
}

}  // namespace gpmi
