// Internal declarations shared by the translation units of libgpmi355x.so.
// gfx950 (MI355X / CDNA4) only: 64-lane wavefronts, v_mfma_f64_16x16x4_f64.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <cmath>
#include <mutex>

#include "gpmi_kroute.h"
#include "gpmi_route.h"

namespace gpmi {

constexpr int TILE = 128;   // row / column padding granule of every matrix
constexpr int IB = 64;      // inner (register-resident) panel width

// Kernel-selection options (gpmi_set_option).  They live in the context; a C-ABI call installs its
// context's set for the calling thread (TuneScope), so two contexts driven from two threads (the lanes
// of gpmi_lml_batch) never see each other's settings.  The context-free gpmi_dev_* primitives run with
// the defaults.
struct Tuning : GemmTuning {    // gpmi_route.h: the options that select a GEMM kernel
    int trsm_wave = 1;          // 1: wave-per-row substitution kernel for short panels, 0: lane-per-row always
    int rbf_blocks = 16384;     // persistent blocks of the register-path K build
    int trsv_vinv = 2;          // backward solve: 2 one launch, column blocks chained through the solution vector (inverted 128 x 128 diagonal blocks); 1 one launch per 128 unknowns with the same inverses; 0 the 16 x 16 rounds
    int panel_fused = 1;        // 1: fused multi-column panel kernels, 0: first-generation potf2 + substitution leaves
    unsigned long long* gemm_stamps = nullptr;   // diagnostic stamp buffer (gpmi_probe_gemm variant bit 16)
    unsigned long long* panel_stamps = nullptr;  // diagnostic: s_memtime stamps of the panel kernels (gpmi_probe_panel)
};
const Tuning& tuning();         // options of the C-ABI call running on this thread
struct TuneScope {
    const Tuning* prev;
    explicit TuneScope(const Tuning* t);
    ~TuneScope();
};
// What else runs on the chip beside the launches of this thread (gpmi_route.h: Sharing): read by gemm_route and by
// launch_trsm128; a driver that puts work on a second stream or lane says so for the length of a scope.
Sharing& sharing();
struct SharingScope {
    const Sharing prev;
    explicit SharingScope(Sharing s) : prev(sharing()) { sharing() = s; }
    ~SharingScope() { sharing() = prev; }
};

// One-time, per-device opt-in (hipFuncSetAttribute for > 64 KiB of dynamic LDS): thread-safe, keyed by
// the current device, and the error is returned instead of dropped.
struct PerDeviceOnce {
    std::mutex mu;
    uint64_t done = 0;
    template <class F> hipError_t run(F fn) {
        int dev = 0;
        hipError_t e = hipGetDevice(&dev);
        if (e != hipSuccess) return e;
        std::lock_guard<std::mutex> lock(mu);
        if (dev < 64 && ((done >> dev) & 1)) return hipSuccess;
        e = fn();
        if (e == hipSuccess && dev < 64) done |= (uint64_t)1 << dev;
        return e;
    }
};

// ---- gemm_nt.hip ----------------------------------------------------------
// C (M x N) op= A (M x K) * B (N x K)^T, all row-major.  M multiple of 128,
// N multiple of 64, K multiple of 16.  mode 0: C -= A*B^T; mode 1: C = A*B^T.
// lower != 0: skip tiles lying entirely above {col <= row + diag_off}.
struct GemmArgs {
    double* C;
    const double* A;
    const double* B;
    int64_t ldc, lda, ldb;
    int64_t M, N, K;
    int mode = 0;
    int lower = 0;
    int64_t diag_off = 0;
    // optional: row_ncols[ti / row_block_tiles] = number of leading columns of C that
    // the 128-row tile band ti updates (row-block cyclic storage: a rank's stacked
    // row blocks reach different distances to the right); device pointer or null
    const int32_t* row_ncols = nullptr;
    int row_block_tiles = 1;
    // optional host copy of row_ncols (row_bands entries): lets the launcher enumerate only the
    // supertiles that hold live tiles instead of the whole rectangle
    const int32_t* row_ncols_host = nullptr;
    int row_bands = 0;
    int role = 0;   // 1: Cholesky trailing update (launched under its own kernel symbol)
    // optional: B is not one matrix but a sequence of b_block_rows-row blocks (each b_block_rows x K, leading
    // dimension ldb) at B + b_block_off[i] doubles -- the panel column exactly as an all-gather leaves it, one
    // contiguous chunk per rank, read in natural block order through this table (device pointer); LDS-DMA kernel only
    const int64_t* b_block_off = nullptr;
    int64_t b_block_rows = 0;
};
// C -= A B^T over the whole rectangle; a launch with a row map, a block table or a role adds its fields to this
inline GemmArgs gemm_minus(double* C, int64_t ldc, const double* A, int64_t lda, const double* B, int64_t ldb, int64_t M,
                           int64_t N, int64_t K) {
    GemmArgs g;
    g.C = C; g.A = A; g.B = B;
    g.ldc = ldc; g.lda = lda; g.ldb = ldb;
    g.M = M; g.N = N; g.K = K;
    return g;
}
// ... on the tiles that reach {col <= row + diag_off} only
inline GemmArgs gemm_minus_lower(double* C, int64_t ldc, const double* A, int64_t lda, const double* B, int64_t ldb,
                                 int64_t M, int64_t N, int64_t K, int64_t diag_off) {
    GemmArgs g = gemm_minus(C, ldc, A, lda, B, ldb, M, N, K);
    g.lower = 1; g.diag_off = diag_off;
    return g;
}
// The route of a launch (gpmi_route.h: gemm_route; a launch that wants a resident form creates the device's counter
// pool here), and the launch of a route -- for a caller that accounts by the kernel family it reaches.
GemmRoute gemm_nt_route(const GemmArgs& a);
hipError_t launch_gemm_nt(hipStream_t s, const GemmArgs& a, const GemmRoute& r);
inline hipError_t launch_gemm_nt(hipStream_t s, const GemmArgs& a) { return launch_gemm_nt(s, a, gemm_nt_route(a)); }
double gemm_nt_algorithmic_flops(const GemmArgs& a, int64_t real_rows);   // 2K per needed element (lower: on/below the diagonal)
// gemm_dma.hip: the launches of the LDS-DMA kernels of a route (128 x 128 tiles and their forms; 64 x 64 tiles for
// launches with few tiles), and the resident workgroups a launch of this device may use (0: no counter pool)
hipError_t launch_gemm_nt_dma(hipStream_t s, const GemmArgs& a, const GemmRoute& r);
hipError_t launch_gemm_nt_small(hipStream_t s, const GemmArgs& a, const GemmRoute& r);
int gemm_resident_groups();
// number of tiles the launch actually computes (for flop accounting)
double gemm_nt_flops(const GemmArgs& a);

// ---- panel.hip -------------------------------------------------------------
// Cholesky of one 64x64 diagonal block in place (lower), one wavefront.
hipError_t launch_potf2_64(hipStream_t s, double* A, int64_t ld, int64_t col_offset,
                           int64_t* info_dev);
// X (m x 64) <- X * L^-T, L 64x64 lower; m multiple of 64.
hipError_t launch_trsm_rlt64(hipStream_t s, const double* L, int64_t ldl, double* X, int64_t ldx,
                             int64_t m);

// ---- panel_mfma.hip --------------------------------------------------------
// Cholesky of one 128 x 128 diagonal block in place (lower), one workgroup, MFMA updates.
hipError_t launch_potrf128(hipStream_t s, double* A, int64_t ld, int64_t col_offset, int64_t* info_dev);

// X (m x 128) <- X * L^-T, L 128 x 128 lower; m multiple of 128; on the matrix pipe.
hipError_t launch_trsm128(hipStream_t s, const double* L, int64_t ldl, double* X, int64_t ldx, int64_t m);

// X (rows <= 16, ncols) <- X * L^-T for a fused factor L (ncols x ncols, ncols a multiple of 128): the forward sweep for
// a few rows, one launch per 128 columns, L streamed once.  Rows of X from `rows` on and columns from ncols on are neither
// read nor written; of L it reads what trsm128 reads, block by block.
hipError_t launch_border_sweep(hipStream_t s, const double* L, int64_t ldl, int64_t ncols, double* X, int64_t ldx,
                               int64_t rows);
// X (rows, ncols) <- X * L^-1 for the same kind of factor (row i becomes L^-T x_i): the backward sweep, one launch per 128
// columns from the last block to the first whatever `rows` is (16-row groups ride in a second grid dimension), L streamed
// once per row group.  It reads and leaves alone what launch_border_sweep does.
hipError_t launch_back_sweep(hipStream_t s, const double* L, int64_t ldl, int64_t ncols, double* X, int64_t ldx,
                             int64_t rows);

// ---- rbf.hip ---------------------------------------------------------------
struct RbfArgs {
    const double* A;   // rows of the output: nA x d (row-major, device)
    const double* B;   // cols of the output: nB x d
    int64_t nA, nB, d;
    int64_t row0;      // first output row (index into A)
    int64_t nrows;     // rows to produce (multiple of 128 incl. padding)
    int64_t ncols;     // cols to produce (multiple of 128 incl. padding)
    double coef;       // -.5 * (1 / l^2); the Matern kinds: -a = -sqrt(2 nu) / |l| (cov_coef below)
    double sig2;       // sigma^2
    double diag_add;   // + s on global row == col (symmetric build only)
    int symmetric;     // 1: A==B, lower tiles only, identity padding
    double* out;       // nrows x ld, out(0,0) is element (row0, 0)
    int64_t ld;
    // covariance function: 0 squared-exponential (coef, sig2 above);
    // 1 linear  sum_k (a_k - c)(b_k - c), c = kp0            (GP_regression.py:22-33)
    // 2 periodic exp(-2 sin^2(pi |a-b| / p) / l^2), p = kp0, l = kp1, d == 1 (GP_regression.py:36-50)
    // 3 CO2 composite: kernel_1 + kernel_2 + kernel_3 + kernel_4 with theta_1..11 = kpv (CO2_example.py:9-94)
    // 4 / 5 / 6 Matern nu = 1/2, 3/2, 5/2: sig2 P(t) exp(-t), t = -coef sqrt(sq) (include/gpmi.h: the evaluation order)
    int kind = 0;
    double kp0 = 0., kp1 = 0.;
    double kpv[11] = {0., 0., 0., 0., 0., 0., 0., 0., 0., 0., 0.};
    int delta_square = 0;     // kind 3: the reference's output is square -> kernel_4 adds theta_11^2 * eye (:58-59)
    int64_t delta_col0 = 0;   // ... at row == col + delta_col0 (B is a window of the column inputs starting there)
    // upper bound of |a_i - b_j|^2 over the whole launch (from the inputs' bounding boxes), or < 0
    // when unknown: lets the squared-exponential and Matern builds skip their per-wave exp domain test
    double max_sq = -1.0;
};
hipError_t launch_rbf(hipStream_t s, const RbfArgs& a);
// The stationary kinds share the register-path K build and the gradient kernels, which take the per-element function
// as a compile-time family: 0 squared exponential, 1 / 2 / 3 Matern nu = 1/2, 3/2, 5/2 (kinds 4 / 5 / 6).
inline int cov_family(int kind) { return rbf_family(kind); }                   // gpmi_kroute.h
inline bool cov_stationary(int kind) { return rbf_stationary(kind); }
// what multiplies sq (family 0: GP_regression.py:19 evaluation order) or sqrt(sq) (Matern: -a) in the exp argument
inline double cov_coef(int kind, double ell) {
    static const double two_nu[4] = {0.0, 1.0, 3.0, 5.0};
    const int f = cov_family(kind);
    return f ? -(std::sqrt(two_nu[f]) / std::fabs(ell)) : -.5 * (1 / (ell * ell));
}
// what the gradients' plain sums are scaled by where the squared exponential has 1 / l^2: a^2 for a Matern kind
inline double cov_inv_l2(int kind, double ell, double coef) { return cov_family(kind) ? coef * coef : 1.0 / (ell * ell); }

// ---- grad.hip --------------------------------------------------------------
// sum_ij (alpha_i alpha_j - K_y^-1_ij) dK_ij/dtheta over a block of rows (tune_hyperparms_regression.py:54-57)
struct GradArgs {
    const double* A;          // row inputs  nA x d (device)
    const double* B;          // col inputs  nB x d
    int64_t nA, nB, d;
    int64_t row0, nrows;      // rows row0 .. row0+nrows of the full matrix in this launch
    const double* alpha_r;    // alpha indexed by global row
    const double* alpha_c;    // alpha indexed by column
    const double* Kinv;       // (row0 + r, c) at Kinv[r*ld + c]; holds kinv_sign * K_y^-1
    int64_t ld;
    double kinv_sign;
    double coef, sig2, two_sigma, inv_l3;   // family > 0: inv_l3 holds a^2 / l
    int family = 0;           // cov_family of the kernel
    int tri;                  // 1: symmetric case, lower tiles only (needs row0 == 0, nrows == nB)
    double* partial;          // 2 doubles per block (grad_trace_blocks of them)
};
// the lower 128 x 128 tiles of an n x n matrix: the blocks of a tri launch and of the ARD and CO2 sums
int64_t tri_tile_count(int64_t n);
int64_t grad_trace_blocks(const GradArgs& a);
hipError_t launch_grad_trace(hipStream_t s, const GradArgs& a);
// The same W against d + 3 derivatives (per-dimension lengthscales, l, sigma, noise) over the lower 128 x 128 tiles of
// Kn = -K_y^-1: per launch `width` dimensions (4 / 8 / 16 / 32, zero differences beyond d) and, in the first launch, the
// three others; d > 32 takes ceil(d / 32) launches.  sums[q * (width + 3) + j]: launch q's plain sums, without the
// factors sigma^2 / (l^2 r_k) etc. (the caller's), each the fixed-order sum of the per-block partials.
struct GradArdArgs {
    const double* Z;          // scaled inputs n x d (device)
    int64_t n, d;
    const double* alpha;      // length n
    const double* Kn;         // -K_y^-1, lower tiles valid, leading dimension ld
    int64_t ld;
    double coef;              // -1 / (2 l^2); family > 0: -a
    int family = 0;           // cov_family of the kernel: the "x" of the sums is then H(t) and sums[width + 1] takes K / sigma^2
    double* partial;          // (width + 3) * tri_tile_count(n) doubles, component-major
    double* sums;             // (width + 3) * grad_ard_launches doubles
    // The binary classifier's gradient (gpmi_laplace_grad; family 0 only): with lap_s set, alpha is a, Kn is -B^-1 and
    // the weight is a_i a_j + s_i s_j Kn_ij + z_i g_j + z_j g_i; there is no noise sum (its slot holds 0)
    const double* lap_s = nullptr;
    const double* lap_z = nullptr;
    const double* lap_g = nullptr;
};
int64_t grad_ard_width(const GradArdArgs& a);
int64_t grad_ard_launches(const GradArdArgs& a);
hipError_t launch_grad_ard(hipStream_t s, const GradArdArgs& a);
// The same W against the eleven basis sums of the CO2 composite kernel (kind 3) over the lower 128 x 128 tiles of Kn:
//   sums[0..10] = S1 .. S11 of grad.hip's grad_co2_kernel, plain (the caller scales them into the twelve derivatives),
// each the fixed-order sum of the per-block partials.  The constants multiply sq, sin^2(pi r) and log1p(u) inside the four
// exponentials: n1 = -1 / (2 theta_2^2), n4 = -1 / (2 theta_4^2), n5 = -2 / theta_5^2, cu = 1 / (2 theta_8 theta_7^2),
// n8 = -theta_8, n10 = -1 / (2 theta_10^2).
struct GradCo2Args {
    const double* Z;          // inputs n x d (device)
    int64_t n, d;
    const double* alpha;      // length n
    const double* Kn;         // -K_y^-1, lower tiles valid, leading dimension ld
    int64_t ld;
    double n1, n4, n5, cu, n8, n10;
    double* partial;          // 11 * tri_tile_count(n) doubles, component-major
    double* sums;             // 11 doubles
};
hipError_t launch_grad_co2(hipStream_t s, const GradCo2Args& a);
// The gradients of the predictive mean and variance at the test inputs (gpmi_predict_grad_resident), without their
// factors: with e_k = z*_ik - z_jk and g_ij = exp(coef sq_ij) (a Matern family: H(t_ij), 0 where sq_ij == 0 for nu = 1/2)
//   sums[i * ncomp + k]     = sum_j alpha_j g_ij e_k                     k < d
//   sums[i * ncomp + d + k] = sum_j W_ij g_ij e_k                        (W not null; ncomp = 2 d, else d)
// One fused pass, K(X*, X) never stored, W read once, d <= 32; per-(row, column chunk) partials, added in chunk order.
struct PgradArgs {
    const double* Zs;         // scaled test inputs n x d (device)
    const double* Z;          // scaled training inputs N x d
    int64_t n, N, d;
    const double* alpha;      // length N
    const double* W;          // n x ldw, or null: the mean's sums only
    int64_t ldw;
    double coef;              // -1 / (2 l^2); family > 0: -a
    int family = 0;
    double* partial;          // pgrad_chunks(N) * n * ncomp doubles
    double* sums;             // n * ncomp doubles
};
int64_t pgrad_chunks(int64_t N);
hipError_t launch_pgrad(hipStream_t s, const PgradArgs& a);
// Z[i][k] = X[i][k] / r[k]: one IEEE division per element
hipError_t launch_scale_inputs(hipStream_t s, const double* X, const double* r, int64_t n, int64_t d, double* Z);
hipError_t launch_set_identity_diag(hipStream_t s, double* V, int64_t ld, int64_t n);
// ---- leave-one-out cross-validation (GPML 5.4.2), grad.hip ----
// Every kernel reads rows and columns < n only (the identity padding contributes nothing), reads matrices with 16-byte
// loads (ld even, base 16-byte aligned, n < the padded size when n is odd) and adds in a fixed order.
// kappa[i] = sum_{i <= j < n} U[i][j]^2, the diagonal of K_y^-1 = U U^T from the upper triangular U = L^-T
hipError_t launch_loo_kappa(hipStream_t s, const double* U, int64_t ld, int64_t n, double* kappa);
// mu = y - alpha / kappa, var = 1 / kappa, logp = -.5 log var - (y - mu)^2 / (2 var) - .5 log 2 pi (n doubles each), and
// *sum = sum_i logp[i]
hipError_t launch_loo_points(hipStream_t s, const double* y, const double* alpha, const double* kappa, int64_t n,
                             double* mu, double* var, double* logp, double* sum);
// upper(i < j) <- lower(j, i) over the np x np matrix (np a multiple of 64)
hipError_t launch_mirror_lower(hipStream_t s, double* A, int64_t ld, int64_t np);
// D[a][b] = sig2 exp(coef sq_ab) sq_ab (family > 0: sig2 H(t_ab) sq_ab, t = -coef sqrt(sq)) for a, b < n and 0 on the
// padding, np x np in full (np a multiple of 128)
hipError_t launch_loo_dmat(hipStream_t s, const double* Z, int64_t n, int64_t d, double coef, double sig2, int family,
                           double* D, int64_t ld, int64_t np);
// per row i < n of M: sq[i] = sum_j M_ij^2 (sq may be null), d0[i] = sum_j M_ij x0[j], d1[i] = sum_j M_ij x1[j] (x1, d1
// may be null); x0, x1 hold at least n + 1 doubles
hipError_t launch_row_pass(hipStream_t s, const double* M, int64_t ld, int64_t n, const double* x0, const double* x1,
                           double* sq, double* d0, double* d1);
// out[i] = sum_{j < n} C[i][j] * B[i][j] for i < nrows
hipError_t launch_row_dot2(hipStream_t s, const double* C, int64_t ldc, const double* B, int64_t ldb, int64_t nrows,
                           int64_t n, double* out);
// GPML eq. 5.13 without its per-parameter factors.  With Kn = -K_y^-1: cn = row sums of Kn^2, qn = Kn alpha,
// un = Kn (D alpha), sn[i] = -[K_y^-1 D K_y^-1]_ii.  out3[0] (l): r = -un, s = -sn; out3[1] (sigma): r = alpha + noise qn,
// s = kappa - noise cn; out3[2] (noise): r = -qn, s = cn; each sum_i (alpha_i r_i - .5 (1 + alpha_i^2 / kappa_i) s_i) / kappa_i
struct LooGradArgs {
    const double *alpha, *kappa, *cn, *qn, *un, *sn;
    int64_t n;
    double noise;
    double* out3;
};
hipError_t launch_loo_grad_sums(hipStream_t s, const LooGradArgs& a);

// ---- solve.hip -------------------------------------------------------------
// dot[i] = sum_j V[i][j]*m[j], sq[i] = sum_j V[i][j]^2, j < ncols (fixed order)
// out (n x nf row-major) = tril(L) @ Z (n x nf row-major), L n x n with leading dimension ld: reads j <= i only
hipError_t launch_tri_mul(hipStream_t s, const double* L, int64_t ld, const double* Z, int64_t n, int64_t nf, double* out);
hipError_t launch_row_dots(hipStream_t s, const double* V, int64_t ld, int64_t nrows,
                           int64_t ncols, const double* m, double* dot, double* sq);
// out[0] = sum_{i<n} log(A[i*(ld+1)]), out[1] = sum_{i<n} m[i]^2 (deterministic)
hipError_t launch_lml_reduce(hipStream_t s, const double* A, int64_t ld, const double* m,
                             int64_t n, double* out2);
// out2[0] = sum_{i<n} log(A[i*(ld+1)]) (0 if A null), out2[1] = sum_{i<nx} x[i]^2 (0 if x null)
hipError_t launch_logdiag_sumsq(hipStream_t s, const double* A, int64_t ld, int64_t n, const double* x,
                                int64_t nx, double* out2);
// backward substitution  L^T x = b  (x overwrites b); n multiple of 64
hipError_t launch_trsv_lt(hipStream_t s, const double* L, int64_t ld, double* b, int64_t n);
// the same for a factor left by the fused panel kernels (inverses in the diagonal tiles), 128 unknowns per
// launch; n multiple of 128; b is destroyed, the solution goes to xout (must not alias b)
hipError_t launch_trsv_lt_fused(hipStream_t s, const double* L, int64_t ld, double* b, double* xout, int64_t n);
// full inverses of the 128 x 128 diagonal blocks into their upper triangles, and the backward solve that uses them
// vside (optional, n * 128 doubles): V = L_kk^-1 itself, row-major 128 x 128 per block, for launch_trsv_lt_chain
hipError_t launch_vinv128(hipStream_t s, double* A, int64_t ld, int64_t n, double* vside = nullptr);
hipError_t launch_trsv_lt_vinv(hipStream_t s, const double* L, int64_t ld, double* b, double* xout, int64_t n);
// the same in ONE launch (column blocks chained through the solution vector itself); m is only read; err_dev: one int,
// set if a poll gave up
// skip / max_wait_ms: gpmi_probe_trsv_giveup only (bottom blocks left unsolved, a shorter bound on every wait; 0: 10 s)
hipError_t launch_trsv_lt_chain(hipStream_t s, const double* L, int64_t ld, const double* vside, const double* m,
                                double* xout, int64_t n, int* err_dev, int skip = 0, double max_wait_ms = 0.0);
// y[c] = sum_r A[r][c] * x[r]; scratch: ceil(nrows/64) * ncols doubles
hipError_t launch_gemv_t(hipStream_t s, const double* A, int64_t ld, int64_t nrows, int64_t ncols,
                         const double* x, double* y, double* scratch);
// out2[0..1] += the sums of the even / odd entries of part (n pairs), fixed order
hipError_t launch_sum_pairs(hipStream_t s, const double* part, int64_t n, double* out2);
// out[i] = (base ? base[i] : 0) + scale * sum_{q < count} in[q * stride + i], i < n; the sum runs in index order
hipError_t launch_sum_fixed(hipStream_t s, const double* in, int64_t count, int64_t stride, int64_t n,
                            const double* base, double scale, double* out);
// Y (rows x cols) += a * X
hipError_t launch_axpy2d(hipStream_t s, double* Y, int64_t ldy, const double* X, int64_t ldx, int64_t rows,
                         int64_t cols, double a);
// fill helpers
hipError_t launch_fill_rows(hipStream_t s, double* A, int64_t ld, int64_t nrows, int64_t ncols,
                            double value);
hipError_t launch_set_yrow(hipStream_t s, double* row, const double* y, int64_t N, int64_t ncols);
// C = diag_val*I + Kss - G on the lower tiles (post-covariance assembly)
hipError_t launch_extract(hipStream_t s, const double* A, int64_t ld, int64_t r0, int64_t r1,
                          int64_t c0, int64_t c1, double* out, int lower_only);

// ---- probes ----------------------------------------------------------------
hipError_t launch_probe_mfma(hipStream_t s, double* sink, int iters, int cus, int waves_per_simd, int nacc,
                             unsigned long long* clk);
hipError_t launch_probe_write(hipStream_t s, double* buf, int64_t n_doubles, int mode, int blocks, double* sink);

}  // namespace gpmi
