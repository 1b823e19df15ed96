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
// Every tile kernel here (grad_trace_kernel, grad_ard_kernel, grad_co2_kernel, loo_dmat_kernel) recomputes the kernel
// element from X and multiplies it by a weight: one 128 x 128 tile per block, two columns x 32 rows per thread.  What
// they share exists once, below:
//   rbf_tri_tile (gpmi_kroute.h) the lower tiles of a symmetric matrix from the block index
//   stage_edges               both tile edges of X into LDS (d <= 32), zero past the end; beyond, X comes from global memory
//   sqdist2 / sqdist1         the squared distance, s = fma(e, e, s) over k ascending, from LDS or global memory
//   wave_sum64, block_tree256, block_partials   the reductions, each in ONE fixed order: results are bitwise reproducible
//   lower_tile_sums           the body of the weighted sums over the lower tiles of Kn = -K_y^-1 (ARD, Laplace, CO2)
// A kernel's own comment says only what is particular to it: its weight, its terms, its column layout.
// pgrad_kernel (the gradients of the prediction at the test inputs) is no tile kernel: test rows against chunks of training
// columns, the kernel element from both input sets, the same families, wave_sum64 and a fixed-order sum over the chunks.
//
// The per-element function is a compile-time family F (cov_family: 0 squared exponential, 1 / 2 / 3 Matern nu = 1/2,
// 3/2, 5/2).  For a Matern, with t = a sqrt(sq), a = -coef:
//     K / sigma^2 = P(t) e^-t,   dK/dl = sigma^2 a^2 H(t) sq / l,   dK/dz-scale_k likewise with (z_ik - z_jk)^2,
//     H(t) = -(1/t) d(P e^-t)/dt = e^-t / t,  e^-t,  (1 + t) e^-t / 3
// H_1/2 is singular at t = 0 but always multiplied by a squared difference <= sq: it is SELECTED to 0 there (duplicate
// training points), never divided.
#include <algorithm>
#include <type_traits>

#include "exp_dev.h"
#include "gpmi_internal.h"

namespace gpmi {

namespace {

constexpr int RT = 128;
constexpr int GRAD_MAXD = 32;

// ---- the shared pieces ------------------------------------------------------------------------------------------------
// As[r][k] = A[arow0 + r][k] and Bs[k][r] = B[bcol0 + r][k] for the RT rows behind either origin, zero past nA / nB.
// DC == 0: LDS rows are d wide.  DC > 0 (the ARD kernel): they are DC >= d wide and zero from d on.
template <int DC>
__device__ __forceinline__ void stage_edges(double* As, double* Bs, const double* A, const double* B, int64_t arow0,
                                            int64_t bcol0, int64_t nA, int64_t nB, int d, int tid) {
    const int w = DC ? DC : d;
    for (int e = tid; e < RT * w; e += 256) {
        const int r = e / w, k = e - r * w;
        const int64_t ga = arow0 + r, gb = bcol0 + r;
        const bool ink = DC == 0 || k < d;
        As[r * w + k] = (ink && ga < nA) ? A[ga * d + k] : 0.0;
        Bs[k * RT + r] = (ink && gb < nB) ? B[gb * d + k] : 0.0;
    }
    __syncthreads();
}

// Squared distances of row a to the columns b0 and b1, whose dimension k lies at [k * sb] (LDS: sb = RT, b1 = b0 + 1;
// global memory: sb = 1)
__device__ __forceinline__ void sqdist2(const double* a, const double* b0, const double* b1, int sb, int d, double& s0,
                                        double& s1) {
    for (int k = 0; k < d; ++k) {
        const double ak = a[k];
        const double e0 = ak - b0[k * sb], e1 = ak - b1[k * sb];
        s0 = fma(e0, e0, s0);
        s1 = fma(e1, e1, s1);
    }
}

// ... and to the one column b
__device__ __forceinline__ double sqdist1(const double* a, const double* b, int sb, int d) {
    double sq = 0.0;
    for (int k = 0; k < d; ++k) {
        const double e = a[k] - b[k * sb];
        sq = fma(e, e, sq);
    }
    return sq;
}

// The ARD kernel's distance is other arithmetic: the squares e2[k] of the launch's DC dimensions k0 .. k0 + DC are kept
// and ADDED in order (zero beyond d); from global memory the dimensions outside that window follow by FMA.
template <int DC, bool LDS>
__device__ __forceinline__ double ard_sqdist(const double* a, const double* b, int d, int k0, double (&e2)[DC]) {
    double sq = 0.0;
#pragma unroll
    for (int k = 0; k < DC; ++k) {
        const int kk = k0 + k;
        const double e = LDS ? a[k] - b[k * RT] : (kk < d) ? a[kk] - b[kk] : 0.0;
        e2[k] = e * e;
        sq += e2[k];
    }
    if (!LDS) {
        for (int kk = 0; kk < k0; ++kk) {
            const double e = a[kk] - b[kk];
            sq = fma(e, e, sq);
        }
        for (int kk = k0 + DC; kk < d; ++kk) {
            const double e = a[kk] - b[kk];
            sq = fma(e, e, sq);
        }
    }
    return sq;
}

// 64 lanes by a butterfly
__device__ __forceinline__ double wave_sum64(double v) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off, 64);
    return v;
}

// NV values per thread of a 256-thread block by a binary tree in shared memory; sum j ends in sh[j][0], for thread 0 to read
template <int NV>
__device__ __forceinline__ void block_tree256(double (&sh)[NV][256], const double (&v)[NV], int tid) {
#pragma unroll
    for (int j = 0; j < NV; ++j) sh[j][tid] = v[j];
    __syncthreads();
    for (int off = 128; off > 0; off >>= 1) {
        if (tid < off) {
#pragma unroll
            for (int j = 0; j < NV; ++j) sh[j][tid] += sh[j][tid + off];
        }
        __syncthreads();
    }
}

// NS accumulators per thread to the block's partials, component-major (partial[j * nblk + block]): 64 lanes by the
// butterfly, then the four waves in order.  ard_reduce_kernel adds the blocks.
template <int NS>
__device__ __forceinline__ void block_partials(double (&red)[4][NS], const double (&acc)[NS], int tid, double* partial,
                                               int64_t nblk) {
#pragma unroll
    for (int k = 0; k < NS; ++k) {
        const double v = wave_sum64(acc[k]);
        if ((tid & 63) == 0) red[tid >> 6][k] = v;
    }
    __syncthreads();
    if (tid < NS)
        partial[(int64_t)tid * nblk + blockIdx.x] = ((red[0][tid] + red[1][tid]) + red[2][tid]) + red[3][tid];
}

// ---- two traces: l and sigma ------------------------------------------------------------------------------------------
// The thread's columns are the adjacent pair 2 cp, 2 cp + 1.  Any row range of a rectangular matrix (tri == 0: the
// partitioned path) or the lower tiles of the symmetric one; two partials per block, added by the host in block order.
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
        rbf_tri_tile((int)blockIdx.x, ti, tj);
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
    if (LDS) stage_edges<0>(As, Bs, p.A, p.B, grow0, gcol0, p.nA, p.nB, d, tid);
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
        if (LDS) sqdist2(&As[lr * d], &Bs[2 * cp], &Bs[2 * cp + 1], RT, d, s0, s1);
        else sqdist2(p.A + gr * d, p.B + ((gc < p.nB) ? gc : 0) * d, p.B + ((gc + 1 < p.nB) ? gc + 1 : 0) * d, 1, d, s0, s1);
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
    const double acc[2] = {acc_l, acc_s};
    block_tree256(red, acc, tid);
    if (tid == 0) {
        p.partial[2 * (size_t)blockIdx.x] = red[0][0];
        p.partial[2 * (size_t)blockIdx.x + 1] = red[1][0];
    }
}

// ---- weighted sums over the lower tiles of Kn = -K_y^-1 ---------------------------------------------------------------
// lower_tile_sums is the one body of grad_ard_kernel (regression and Laplace weights) and grad_co2_kernel.  The thread's
// two columns lie 64 apart (gc and gc + 64), so that a wave reads both tile edges and Kn densely.  Per element it forms the
// weight w, zero above the diagonal (Kn is valid on and below it only) and doubled strictly below it, then adds the
// terms of a compile-time terms type T to NS accumulators.  They are indexed by compile-time constants only (every loop
// over them is unrolled), so they live in registers; block_partials and ard_reduce_kernel sum them.  T supplies:
//   Dev, NS      the argument block and the number of sums; the last one is the noise slot
//   DC           LDS row width (0: d)
//   Weight       the row's share of the weight, loaded once per row, and the element's weight from it
//   Dist, dist   what the terms need of the squared distance, and its form
//   add          the terms
// Nothing here is selected at run time: every difference between the callers is a type or a template parameter.

// w = alpha_i alpha_j + Kn_ij; the diagonal's w goes to the noise sum
struct RegWeight {
    double ar;
    template <class Dev>
    __device__ __forceinline__ RegWeight(const Dev& p, int64_t gr) : ar(p.alpha[gr]) {}
    template <class Dev>
    __device__ __forceinline__ double operator()(const Dev& p, int64_t g, int64_t gr, bool in, const double* kn,
                                                 double& acc_n) const {
        double w = (in && g <= gr) ? fma(ar, p.alpha[g], *kn) : 0.0;
        if (g == gr) acc_n += w;
        else w += w;
        return w;
    }
};

template <class T, bool LDS>
__device__ __forceinline__ void lower_tile_sums(const typename T::Dev& p) {
    extern __shared__ __attribute__((aligned(16))) double lds[];
    __shared__ double red[4][T::NS];
    int ti, tj;
    rbf_tri_tile((int)blockIdx.x, ti, tj);
    const int d = p.d, w = T::DC ? T::DC : d;
    const int64_t grow0 = (int64_t)ti * RT, gcol0 = (int64_t)tj * RT;
    const int tid = threadIdx.x;
    double* As = lds;               // [RT][w]
    double* Bs = lds + RT * w;      // [w][RT]
    if (LDS) stage_edges<T::DC>(As, Bs, p.Z, p.Z, grow0, gcol0, p.n, p.n, d, tid);
    const int cp = tid & 63, rg = tid >> 6;
    const int64_t gc = gcol0 + cp;
    double acc[T::NS], acc_n = 0.0;                              // acc_n: the noise sum, the last slot
#pragma unroll
    for (int k = 0; k < T::NS; ++k) acc[k] = 0.0;
    for (int r = 0; r < 32; ++r) {
        const int lr = 32 * rg + r;
        const int64_t gr = grow0 + lr;
        if (gr >= p.n) break;                                    // wave-uniform
        const typename T::Weight weight(p, gr);
        const double* kp = p.Kn + gr * p.ld + gc;
#pragma unroll
        for (int c = 0; c < 2; ++c) {                            // the thread's two columns, one after the other
            const int64_t g = gc + 64 * c;
            const bool in = g < p.n;
            typename T::Dist x;
            if (LDS) T::template dist<true>(p, &As[lr * w], &Bs[cp + 64 * c], x);
            else T::template dist<false>(p, p.Z + gr * d, p.Z + (in ? g : 0) * d, x);
            const double wt = weight(p, g, gr, in, kp + 64 * c, acc_n);
            T::add(p, wt, x, acc);
        }
    }
    acc[T::NS - 1] = acc_n;
    block_partials(red, acc, tid, p.partial, p.nblk);
}

// ---- d + 3 traces: per-dimension lengthscales (ARD), l, sigma, noise ---------------------------------------------
// Per element: e_k^2 = (z_ik - z_jk)^2 for the DC dimensions of this launch (zero beyond d), x = exp(coef * sum over
// ALL d of e_k^2), then
//     acc_k += w x e_k^2,   acc_l += w x sq,   acc_s += w x,   acc_n += w on the diagonal
// with w = alpha_i alpha_j - K_y^-1_ij (a Matern family: x = H(t) in acc_k and acc_l, x = P(t) e^-t in acc_s).
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
// (its slot is written 0).  The LAP instantiations (family 0 only) take their own argument block.
struct ArdLapDev : ArdDev {
    const double* s;
    const double* z;
    const double* g;
};
template <bool LAP> struct ArdDevOf { typedef ArdDev type; };
template <> struct ArdDevOf<true> { typedef ArdLapDev type; };

struct LapWeight {
    double ar, sr, zr, gr_;
    __device__ __forceinline__ LapWeight(const ArdLapDev& p, int64_t gr)
        : ar(p.alpha[gr]), sr(p.s[gr]), zr(p.z[gr]), gr_(p.g[gr]) {}
    __device__ __forceinline__ double operator()(const ArdLapDev& p, int64_t g, int64_t gr, bool in, const double* kn,
                                                 double&) const {
        double w = 0.0;
        if (in && g <= gr) {
            w = fma(ar, p.alpha[g], (sr * p.s[g]) * *kn);
            w = fma(zr, p.g[g], w);
            w = fma(p.z[g], gr_, w);
        }
        if (g != gr) w += w;
        return w;
    }
};

template <int DC_, int F, bool LAP>
struct ArdTerms {
    typedef typename ArdDevOf<LAP>::type Dev;
    typedef typename std::conditional<LAP, LapWeight, RegWeight>::type Weight;
    static constexpr int DC = DC_, NS = DC_ + 3;
    struct Dist {
        double sq, e2[DC_];
    };
    template <bool LDS>
    static __device__ __forceinline__ void dist(const Dev& p, const double* a, const double* b, Dist& x) {
        x.sq = ard_sqdist<DC_, LDS>(a, b, p.d, p.k0, x.e2);
    }
    static __device__ __forceinline__ void add(const Dev& p, double w, const Dist& x, double (&acc)[NS]) {
        double wx, ws;                                           // the weight of the lengthscale sums and of sigma's
        if constexpr (F == 0) {
            wx = ws = w * exp(p.coef * x.sq);
        } else {
            double kk, hh;
            matern_kh<F>(p.coef, x.sq, kk, hh);
            wx = w * hh;
            ws = w * kk;
        }
#pragma unroll
        for (int k = 0; k < DC_; ++k) acc[k] = fma(wx, x.e2[k], acc[k]);
        acc[DC_] = fma(wx, x.sq, acc[DC_]);
        acc[DC_ + 1] += ws;
    }
};

// LDS: d <= DC and k0 == 0, dimensions d .. DC are zero on both staged edges
template <int DC, bool LDS, int F, bool LAP = false>
__global__ __launch_bounds__(256) void grad_ard_kernel(const typename ArdDevOf<LAP>::type p) {
    lower_tile_sums<ArdTerms<DC, F, LAP>, LDS>(p);
}

// out[j] = sum over the blocks of partial[j * nblk + b]: thread t adds blocks t, t + 256, ... in order, then a fixed tree
__global__ __launch_bounds__(256) void ard_reduce_kernel(const double* partial, int64_t nblk, double* out) {
    __shared__ double sh[1][256];
    const double* in = partial + (int64_t)blockIdx.x * nblk;
    double v[1] = {0.0};
    for (int64_t b = threadIdx.x; b < nblk; b += 256) v[0] += in[b];
    block_tree256(sh, v, (int)threadIdx.x);
    if (threadIdx.x == 0) out[blockIdx.x] = sh[0][0];
}

// ---- 11 basis sums of the CO2 composite kernel (kind 3; CO2_example.py:9-64) ----------------------------------------
// The regression weight w = alpha_i alpha_j + Kn_ij.  Per element, with sq the squared distance and r = sqrt(sq):
//     e1 = exp(n1 sq)   s2 = sin^2(pi r)   q2 = exp(n4 sq + n5 s2)   u = cu sq   p3 = exp(n8 log1p(u))   e4 = exp(n10 sq)
//     S1 += w e1   S2 += w e1 sq   S3 += w q2   S4 += w q2 sq   S5 += w q2 s2
//     S6 += w p3   S7 += w p3 sq / (1 + u)   S8 += w p3 (u / (1 + u) - log1p(u))   S9 += w e4   S10 += w e4 sq
//     S11 += w on the diagonal
// The six constants come from the host (regress.hip: lml_grad_co2_impl), which also turns the sums into the twelve
// derivatives.  Every term is regular at sq == 0 (e1 = 1, s2 = 0, u = 0): nothing is selected on the diagonal or for
// duplicate points.  LDS rows are d wide (d <= GRAD_MAXD).
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

struct Co2Terms {
    typedef Co2Dev Dev;
    typedef RegWeight Weight;
    static constexpr int DC = 0, NS = CO2_NS;
    struct Dist {
        double sq;
    };
    template <bool LDS>
    static __device__ __forceinline__ void dist(const Dev& p, const double* a, const double* b, Dist& x) {
        x.sq = sqdist1(a, b, LDS ? RT : 1, p.d);
    }
    static __device__ __forceinline__ void add(const Dev& p, double w, const Dist& x, double (&acc)[NS]) {
        const double sq = x.sq;
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
};

template <bool LDS>
__global__ __launch_bounds__(256) void grad_co2_kernel(const Co2Dev p) {
    lower_tile_sums<Co2Terms, LDS>(p);
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
// dK/dl = a^2 D / l, with the library exp), zero on padded rows and columns.  Every tile
// of a square grid, the adjacent column pair; exp by the K build's polynomial while every lane of
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
    if (LDS) stage_edges<0>(As, Bs, p.Z, p.Z, grow0, gcol0, p.n, p.n, d, tid);
    const int cp = tid & 63, rg = tid >> 6;
    const int64_t gc = gcol0 + 2 * cp;
    const bool in0 = gc < p.n, in1 = gc + 1 < p.n;
    for (int r = 0; r < 32; ++r) {
        const int lr = 32 * rg + r;
        const int64_t gr = grow0 + lr;
        const bool inr = gr < p.n;                               // wave-uniform
        double s0 = 0.0, s1 = 0.0;
        if (LDS) sqdist2(&As[lr * d], &Bs[2 * cp], &Bs[2 * cp + 1], RT, d, s0, s1);
        else sqdist2(p.Z + (inr ? gr : 0) * d, p.Z + (in0 ? gc : 0) * d, p.Z + (in1 ? gc + 1 : 0) * d, 1, d, s0, s1);
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
    __shared__ double sh[1][256];
    const int comp = blockIdx.x;
    double acc[1] = {0.0};
    for (int64_t i = threadIdx.x; i < p.n; i += 256) {
        const double a = p.alpha[i], k = p.kappa[i];
        double r, s;
        if (comp == 0) { r = -p.un[i]; s = -p.sn[i]; }
        else if (comp == 1) { r = a + p.noise * p.qn[i]; s = k - p.noise * p.cn[i]; }
        else { r = -p.qn[i]; s = p.cn[i]; }
        acc[0] += (a * r - .5 * (1.0 + a * a / k) * s) / k;
    }
    block_tree256(sh, acc, (int)threadIdx.x);
    if (threadIdx.x == 0) p.out3[comp] = sh[0][0];
}

// ---- gradients of the predictive mean and variance at the test inputs --------------------------------------------------
// Per pair (test row i, training column j): e_k = z*_ik - z_jk, sq = sum_k e_k^2 (FMA over k ascending), g = exp(coef sq)
// (a Matern family: g = H(t), selected to 0 at sq == 0 for nu = 1/2 by matern_kh) once, then for the row's d dimensions
//     am_k += alpha_j g e_k        and, HW:   aw_k += W_ij g e_k
// K(X*, X) is never stored; W is read once.  A block takes RB test rows (RB * DC <= 32: a row's 2 DC sums stay in
// registers) against PG_CHUNK training columns, a thread four of them 256 apart, so that a training point's coordinates
// are loaded once for the RB rows.  The sums of a (row, chunk) go to the workspace -- 64 lanes by the butterfly, then the
// four waves in order -- and launch_sum_fixed adds the chunks in index order: no atomics, the same bits every run.
constexpr int PG_CHUNK = 1024;
struct PgradDev {
    const double* Zs;       // scaled test inputs n x d
    const double* Z;        // scaled training inputs N x d
    int64_t n, N;
    int d;
    const double* alpha;    // length N
    const double* W;        // n x ldw (HW only)
    int64_t ldw;
    double coef;
    double* partial;        // [chunk][row][ncomp]
    int ncomp;              // d, or 2 d with W
};

template <int F, int DC, int RB, bool HW>
__global__ __launch_bounds__(256) void pgrad_kernel(const PgradDev p) {
    constexpr int NC = HW ? 2 * DC : DC;
    __shared__ double zs[RB][DC];
    __shared__ double red[4][RB * NC];
    const int tid = threadIdx.x, d = p.d;
    const int64_t i0 = (int64_t)blockIdx.x * RB;
    if (tid < RB * DC) {
        const int r = tid / DC, k = tid - r * DC;
        const int64_t i = (i0 + r < p.n) ? i0 + r : p.n - 1;
        zs[r][k] = (k < d) ? p.Zs[i * d + k] : 0.0;
    }
    __syncthreads();
    double am[RB][DC], aw[HW ? RB : 1][DC];
#pragma unroll
    for (int r = 0; r < RB; ++r)
#pragma unroll
        for (int k = 0; k < DC; ++k) {
            am[r][k] = 0.0;
            if constexpr (HW) aw[r][k] = 0.0;
        }
    for (int q = 0; q < PG_CHUNK / 256; ++q) {
        const int64_t j = (int64_t)blockIdx.y * PG_CHUNK + q * 256 + tid;
        if (j >= p.N) continue;
        double z[DC];
#pragma unroll
        for (int k = 0; k < DC; ++k) z[k] = (k < d) ? p.Z[j * d + k] : 0.0;
        const double aj = p.alpha[j];
#pragma unroll
        for (int r = 0; r < RB; ++r) {
            const int64_t i = (i0 + r < p.n) ? i0 + r : p.n - 1;
            double e[DC], sq = 0.0;
#pragma unroll
            for (int k = 0; k < DC; ++k) {
                e[k] = zs[r][k] - z[k];
                sq = fma(e[k], e[k], sq);
            }
            double g;
            if constexpr (F == 0) {
                g = exp(p.coef * sq);
            } else {
                double kk;
                matern_kh<F>(p.coef, sq, kk, g);
            }
            const double ga = aj * g;
#pragma unroll
            for (int k = 0; k < DC; ++k) am[r][k] = fma(ga, e[k], am[r][k]);
            if constexpr (HW) {
                const double gw = p.W[i * p.ldw + j] * g;
#pragma unroll
                for (int k = 0; k < DC; ++k) aw[r][k] = fma(gw, e[k], aw[r][k]);
            }
        }
    }
#pragma unroll
    for (int r = 0; r < RB; ++r)
#pragma unroll
        for (int k = 0; k < DC; ++k) {
            const double v = wave_sum64(am[r][k]);
            if ((tid & 63) == 0) red[tid >> 6][r * NC + k] = v;
            if constexpr (HW) {
                const double u = wave_sum64(aw[r][k]);
                if ((tid & 63) == 0) red[tid >> 6][r * NC + DC + k] = u;
            }
        }
    __syncthreads();
    if (tid < RB * NC) {
        const int r = tid / NC, cq = tid - r * NC;
        const int half = cq / DC, k = cq - half * DC;
        const int64_t i = i0 + r;
        if (i < p.n && k < d)
            p.partial[((int64_t)blockIdx.y * p.n + i) * p.ncomp + half * d + k] =
                ((red[0][tid] + red[1][tid]) + red[2][tid]) + red[3][tid];
    }
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

// lower 128 x 128 tiles of an n x n matrix
int64_t tri_tile_count(int64_t n) {
    const int64_t T = (n + RT - 1) / RT;
    return T * (T + 1) / 2;
}
// dimensions per launch: the narrowest of 4 / 8 / 16 / 32 that holds d, 32 beyond
int64_t grad_ard_width(const GradArdArgs& a) { return a.d <= 4 ? 4 : a.d <= 8 ? 8 : a.d <= 16 ? 16 : 32; }
int64_t grad_ard_launches(const GradArdArgs& a) { return a.d <= GRAD_MAXD ? 1 : (a.d + GRAD_MAXD - 1) / GRAD_MAXD; }

// f(std::integral_constant<int, family>()): the runtime family (0 .. 3, checked by the caller) as a compile-time constant
template <class Fn>
static void with_family(int family, Fn&& f) {
    switch (family) {
        case 0: f(std::integral_constant<int, 0>()); break;
        case 1: f(std::integral_constant<int, 1>()); break;
        case 2: f(std::integral_constant<int, 2>()); break;
        default: f(std::integral_constant<int, 3>()); break;
    }
}

// the width ladder of both weights: d <= 32 from LDS at width w = grad_ard_width, beyond from global memory at 32
template <int F, bool LAP>
static void grad_ard_launch(hipStream_t s, const typename ArdDevOf<LAP>::type& p, int64_t d, int w) {
    const dim3 grid((unsigned)p.nblk), block(256);
    auto go = [&](auto dc) {
        constexpr int DC = decltype(dc)::value;
        hipLaunchKernelGGL((grad_ard_kernel<DC, true, F, LAP>), grid, block, (size_t)2 * RT * DC * sizeof(double), s, p);
    };
    if (d > GRAD_MAXD) hipLaunchKernelGGL((grad_ard_kernel<32, false, F, LAP>), grid, block, 0, s, p);
    else if (w == 4) go(std::integral_constant<int, 4>());
    else if (w == 8) go(std::integral_constant<int, 8>());
    else if (w == 16) go(std::integral_constant<int, 16>());
    else go(std::integral_constant<int, 32>());
}

hipError_t launch_grad_ard(hipStream_t s, const GradArdArgs& a) {
    if (a.n <= 0 || a.d <= 0) return hipSuccess;
    if (a.family < 0 || a.family > 3) return hipErrorInvalidValue;
    const bool lap = a.lap_s != nullptr;
    if (lap && (a.family != 0 || !a.lap_z || !a.lap_g)) return hipErrorInvalidValue;
    ArdLapDev p;
    p.Z = a.Z; p.n = a.n; p.d = (int)a.d; p.alpha = a.alpha; p.Kn = a.Kn; p.ld = a.ld; p.coef = a.coef;
    p.partial = a.partial; p.nblk = tri_tile_count(a.n);
    p.s = a.lap_s; p.z = a.lap_z; p.g = a.lap_g;
    const int w = (int)grad_ard_width(a);
    const int64_t nl = grad_ard_launches(a);
    for (int64_t q = 0; q < nl; ++q) {       // d > 32: every launch recomputes the whole squared distance and reads Kn again
        p.k0 = (int)(q * GRAD_MAXD);
        if (lap) grad_ard_launch<0, true>(s, p, a.d, w);
        else with_family(a.family, [&](auto f) { grad_ard_launch<decltype(f)::value, false>(s, p, a.d, w); });
        hipError_t e = hipGetLastError();
        if (e != hipSuccess) return e;
        hipLaunchKernelGGL(ard_reduce_kernel, dim3((unsigned)(w + 3)), dim3(256), 0, s, a.partial, p.nblk, a.sums + q * (w + 3));
        if ((e = hipGetLastError()) != hipSuccess) return e;
    }
    return hipSuccess;
}

hipError_t launch_grad_co2(hipStream_t s, const GradCo2Args& a) {
    if (a.n <= 0 || a.d <= 0) return hipSuccess;
    Co2Dev p;
    p.Z = a.Z; p.n = a.n; p.d = (int)a.d; p.alpha = a.alpha; p.Kn = a.Kn; p.ld = a.ld;
    p.n1 = a.n1; p.n4 = a.n4; p.n5 = a.n5; p.cu = a.cu; p.n8 = a.n8; p.n10 = a.n10;
    p.partial = a.partial; p.nblk = tri_tile_count(a.n);
    const dim3 grid((unsigned)p.nblk), block(256);
    if (a.d <= GRAD_MAXD) hipLaunchKernelGGL(grad_co2_kernel<true>, grid, block, (size_t)2 * RT * a.d * sizeof(double), s, p);
    else hipLaunchKernelGGL(grad_co2_kernel<false>, grid, block, 0, s, p);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(ard_reduce_kernel, dim3(CO2_NS), dim3(256), 0, s, a.partial, p.nblk, a.sums);
    return hipGetLastError();
}

int64_t grad_trace_blocks(const GradArgs& a) {
    return a.tri ? tri_tile_count(a.nrows) : ((a.nrows + RT - 1) / RT) * ((a.nB + RT - 1) / RT);
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
    with_family(a.family, [&](auto f) {
        constexpr int F = decltype(f)::value;
        if (a.d <= GRAD_MAXD) hipLaunchKernelGGL((grad_trace_kernel<true, F>), grid, block, lds, s, p);
        else hipLaunchKernelGGL((grad_trace_kernel<false, F>), grid, block, 0, s, p);
    });
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
    const dim3 grid(T, T), block(256);
    with_family(family, [&](auto f) {
        constexpr int F = decltype(f)::value;
        if (d <= GRAD_MAXD) hipLaunchKernelGGL((loo_dmat_kernel<true, F>), grid, block, (size_t)2 * RT * d * sizeof(double), s, p);
        else hipLaunchKernelGGL((loo_dmat_kernel<false, F>), grid, block, 0, s, p);
    });
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

int64_t pgrad_chunks(int64_t N) { return (N + PG_CHUNK - 1) / PG_CHUNK; }

hipError_t launch_pgrad(hipStream_t s, const PgradArgs& a) {
    if (a.n <= 0 || a.N <= 0) return hipSuccess;
    if (a.d <= 0 || a.d > GRAD_MAXD || a.family < 0 || a.family > 3) return hipErrorInvalidValue;
    PgradDev p;
    p.Zs = a.Zs; p.Z = a.Z; p.n = a.n; p.N = a.N; p.d = (int)a.d; p.alpha = a.alpha; p.W = a.W; p.ldw = a.ldw;
    p.coef = a.coef; p.partial = a.partial; p.ncomp = (int)(a.W ? 2 * a.d : a.d);
    const int64_t nch = pgrad_chunks(a.N);
    auto go = [&](auto f, auto dc, auto rb) {
        constexpr int F = decltype(f)::value, DC = decltype(dc)::value, RB = decltype(rb)::value;
        const dim3 grid((unsigned)((a.n + RB - 1) / RB), (unsigned)nch), block(256);      // chunks <= 65535: N < 2^26
        if (a.W) hipLaunchKernelGGL((pgrad_kernel<F, DC, RB, true>), grid, block, 0, s, p);
        else hipLaunchKernelGGL((pgrad_kernel<F, DC, RB, false>), grid, block, 0, s, p);
    };
    using std::integral_constant;
    if (nch > 65535) return hipErrorInvalidValue;
    with_family(a.family, [&](auto f) {
        if (a.d <= 4) go(f, integral_constant<int, 4>(), integral_constant<int, 4>());
        else if (a.d <= 8) go(f, integral_constant<int, 8>(), integral_constant<int, 4>());
        else if (a.d <= 16) go(f, integral_constant<int, 16>(), integral_constant<int, 2>());
        else go(f, integral_constant<int, 32>(), integral_constant<int, 1>());
    });
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
    const int64_t len = a.n * p.ncomp;
    return launch_sum_fixed(s, a.partial, nch, len, len, nullptr, 1.0, a.sums);
}

}  // namespace gpmi
