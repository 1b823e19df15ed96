// Internal to libgpmi355x.so: the context object behind the opaque gpmi_ctx handle, the error
// helpers every translation unit of the C-ABI shares (HIP_TRY, LAUNCH_TRY), the single-GPU drivers (driver.hip) and the
// host-side pieces the fits, predictions and gradients share: regress.hip's backward solves, predict_front and ARD trace
// ending, laplace.hip's classifier skeleton.
#pragma once
#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstring>
#include <limits>
#include <string>
#include <thread>
#include <vector>

#include "../../include/gpmi.h"
#include "gpmi_internal.h"
#include "gpmi_pgrad_plan.h"
#include "gpmi_state.h"

namespace gpmi {

extern thread_local std::string g_err;      // text behind gpmi_last_error() (gpmi_api.hip)

inline int fail_runtime(hipError_t e, const char* what) {
    char buf[512];
    snprintf(buf, sizeof buf, "%s: %s (hipError %d)", what, hipGetErrorString(e), (int)e);
    g_err = buf;
    return GPMI_ERR_RUNTIME;
}
inline int fail_arg(const char* what) {
    g_err = what;
    return GPMI_ERR_BAD_ARG;
}

#define HIP_TRY(expr)                                             \
    do {                                                          \
        hipError_t _e = (expr);                                   \
        if (_e != hipSuccess) return fail_runtime(_e, #expr);     \
    } while (0)

// a kernel launch that returns through fail_runtime if the launch was refused
#define LAUNCH_TRY(kernel, grid, block, lds, stream, ...)                     \
    do {                                                                      \
        hipLaunchKernelGGL(kernel, grid, block, lds, stream, __VA_ARGS__);    \
        HIP_TRY(hipGetLastError());                                           \
    } while (0)

inline int64_t round_up(int64_t x, int64_t m) { return (x + m - 1) / m * m; }

struct DevBuf {
    void* p = nullptr;
    size_t cap = 0;
    hipError_t ensure(size_t bytes) {
        if (bytes <= cap) return hipSuccess;
        if (p) { hipError_t e = hipFree(p); if (e != hipSuccess) return e; p = nullptr; cap = 0; }
        hipError_t e = hipMalloc(&p, bytes);
        if (e == hipSuccess) cap = bytes;
        return e;
    }
    void release() { if (p) (void)hipFree(p); p = nullptr; cap = 0; }
    template <class T> T* as() const { return reinterpret_cast<T*>(p); }
};

struct TimedSpan { hipEvent_t a, b; int slot; };

// Per-dimension bounding box of a point set (host side, at upload time).  Two boxes bound every
// squared distance of a kernel-matrix launch, which lets the squared-exponential build drop its
// per-wave exp domain test (RbfArgs::max_sq).  Non-finite inputs make the box invalid.
struct Box {
    std::vector<double> lo, hi;
    bool valid = false;
    void assign(const double* X, int64_t n, int64_t d) {
        lo.assign((size_t)d, std::numeric_limits<double>::infinity());
        hi.assign((size_t)d, -std::numeric_limits<double>::infinity());
        bool finite = n > 0;
        for (int64_t i = 0; i < n; ++i)
            for (int64_t k = 0; k < d; ++k) {
                const double v = X[i * d + k];
                finite &= std::isfinite(v);
                lo[(size_t)k] = std::min(lo[(size_t)k], v);
                hi[(size_t)k] = std::max(hi[(size_t)k], v);
            }
        valid = finite;
    }
    // the box of the set with n more points (gpmi_append)
    void extend(const double* X, int64_t n, int64_t d) {
        if ((int64_t)lo.size() != d) { assign(X, n, d); return; }
        bool finite = valid;
        for (int64_t i = 0; i < n; ++i)
            for (int64_t k = 0; k < d; ++k) {
                const double v = X[i * d + k];
                finite &= std::isfinite(v);
                lo[(size_t)k] = std::min(lo[(size_t)k], v);
                hi[(size_t)k] = std::max(hi[(size_t)k], v);
            }
        valid = finite;
    }
};
// The box of z = x / r from the box of x: division by a positive number is monotone under rounding, so the same
// division the device performs on every element gives exact bounds of the scaled set.
inline void box_scale(const Box& raw, const std::vector<double>& r, Box& out) {
    out = raw;
    if (raw.lo.size() != r.size()) { out.valid = false; return; }
    for (size_t k = 0; k < r.size(); ++k) {
        out.lo[k] = raw.lo[k] / r[k];
        out.hi[k] = raw.hi[k] / r[k];
    }
}
inline double box_max_sq(const Box& a, const Box& b) {
    if (!a.valid || !b.valid || a.lo.size() != b.lo.size()) return -1.0;
    double s = 0.0;
    for (size_t k = 0; k < a.lo.size(); ++k) {
        const double w = std::max(a.hi[k] - b.lo[k], b.hi[k] - a.lo[k]);
        s += w * w;
    }
    return std::isfinite(s) ? s : -1.0;
}

}  // namespace gpmi

// the handle type of include/gpmi.h lives at global scope
using gpmi::Box;
using gpmi::DevBuf;
using gpmi::TimedSpan;

struct gpmi_ctx {
    int device = 0;
    hipStream_t stream = nullptr;    // main stream: K build, trailing updates, reductions
    hipStream_t pstream = nullptr;   // high-priority stream: panel factorisations (lookahead)
    // options
    int64_t nb = 0;         // outer block width of the Cholesky (multiple of 128); 0 = by size
    int64_t block(int64_t ncols) const { return nb ? nb : (ncols >= 32768 ? 2048 : ncols >= 12288 ? 1024 : 512); }
    int64_t ld_pad = 544;   // doubles added to every leading dimension
    int timing = 1;
    int lookahead = 1;      // factor panel k+1 while the rest of trailing update k runs
    int64_t la_min = 6144;  // ... from this many columns on (below, the two-stream choreography costs more than the panel it hides:
                            // profiles/r04_la_min_sweep.txt -- one pass / two calls / fit alone at N = 4096: 3.06 -> 2.96 / 3.82 -> 3.86 /
                            // 2.56 -> 2.59 ms, 6144: 5.41 -> 5.20 / 6.69 -> 6.50 / 4.67 -> 4.48, 10240: 13.8 -> 12.6 / 15.9 -> 14.7; same bits)
    int64_t shallow_min = 6144; // under lookahead, panels with fewer columns left than this use the one-launch panel kernels (0: never)
    // the blocked sweeps (cholesky_inplace, solve_sweep_factor) run their panel chain on pstream beside the update
    bool lookahead_for(int64_t ncols) const { return lookahead && pstream && ncols > block(ncols) && ncols >= la_min; }
    int lanes = 0;          // gpmi_lml_batch: factorisations in flight (0 = by size)
    std::vector<gpmi_ctx*> lane_ctx;   // the extra lanes (own streams and workspaces), created on demand
    int64_t reserve = 0;    // ensure_train_buffers sizes A for N + reserve points, so that gpmi_append stays in place
    int append_route = -1;  // the route the last gpmi_append took: 1 skinny, 0 padded (gpmi_get_layout)
    int append_skinny = -1; // gpmi_append, k <= 16 on a fused factor: -1 by size, 0 the padded 128-row sweep, 1 the <= 16-row kernel
    gpmi::Tuning tune;      // kernel-selection options of this context (installed per call: gpmi::TuneScope)
    // training set / factor
    int64_t N = 0, d = 0, Np = 0, ldA = 0, Mp = 0;
    int64_t rows_cap = 0;    // rows A is laid out for (>= Mp, the rows in use: option "reserve", or what an append left)
    gpmi::Resident res;      // what is resident and what was derived from it: gpmi_state.h, the only place that changes it
    double sig2 = 1.0, coef = -0.5;
    int kind = 0;            // covariance function: 0 rbf, 1 linear, 2 periodic, 3 CO2 composite, 4 / 5 / 6 Matern nu = 1/2, 3/2, 5/2 (gpmi_set_kernel*)
    double kp0 = 0., kp1 = 0.;
    double kpv[11] = {0., 0., 0., 0., 0., 0., 0., 0., 0., 0., 0.};
    DevBuf X, y, A, info, red;
    // test set
    int64_t n = 0, np_ = 0, ldV = 0, ldP = 0;
    int64_t v_row0 = 0;      // v^T in rows of A (gpmi_fit_predict_resident, res.v_in_A) starts at this row
    double* v_rows() { return res.v_in_A ? A.as<double>() + v_row0 * ldA : V.as<double>(); }
    // the y rows: row Np of A -- or, when the posterior factor rides as well (gpmi_fit_predict_sample_resident), behind the
    // test rows, whose own n_p columns then follow the training columns
    int64_t yrow = 0;
    double* m_row() { return A.as<double>() + yrow * ldA; }
    std::vector<double> hXs; // host copy of the test inputs (diag(K_ss) of the linear kernel)
    Box boxX, boxXs;         // bounding boxes of the training / test inputs
    // Per-dimension relative lengthscales r_k (gpmi_set_lengthscales; empty: isotropic).  X and Xs keep the raw inputs;
    // Xz and Xsz hold z = x / r, one IEEE division per element on the device, with boxZ / boxZs their boxes.  Every
    // kernel-matrix build and the gradient read the inputs through x_train() / x_test() / box_train() / box_test(), so
    // an isotropic context reads the buffers it always read.
    std::vector<double> ard_r;
    DevBuf Xz, Xsz, ard_rdev;
    Box boxZ, boxZs;
    bool ard() const { return !ard_r.empty(); }
    const double* x_train() const { return ard() ? Xz.as<double>() : X.as<double>(); }
    const double* x_test() const { return ard() ? Xsz.as<double>() : Xs.as<double>(); }
    const Box& box_train() const { return ard() ? boxZ : boxX; }
    const Box& box_test() const { return ard() ? boxZs : boxXs; }
    DevBuf Xs, V, P, vec, dense;
    DevBuf flag;             // one int the single-launch backward solve sets if a poll gave up
    DevBuf vside;            // Np x 128: the inverses of the 128 x 128 diagonal blocks, row-major (launch_vinv128's side buffer)
    DevBuf cov_a, cov_b, cov_out;   // gpmi_rbf / gpmi_cov staging, kept across calls (the BO loops call them hundreds of times)
    DevBuf U, Kn, gpart;     // f2: L^-T, -(K+sI)^-1, per-tile partial sums of the gradient trace
    DevBuf gsum;             // gpmi_lml_grad_ard: the d + 3 sums, reduced on the device
    double sigma = 1.0, ell = 1.0;   // hyper-parameters of the resident factorisation
    double noise = 0.0;              // ... and its noise variance (regression factorisations only)
    DevBuf app;              // gpmi_append, skinny route: the new points (aligned copy) and their 128 x N0 rows of K
    // gpmi_remove (remove.hip): the buffer a removal leaves behind, kept as the target of the next one under option
    // "remove_keep_spare" (any fit drops it); the sweep's workspace (side vectors, rotations, the gather map)
    int remove_keep_spare = 0;
    DevBuf spareA, rem;
    // gpmi_predict_grad_resident (predgrad.hip): W = V L^-1 (n_p x (Np + ld_pad), grown on demand, released by the next
    // fit into A), the per-chunk partial sums and the sums
    int pgrad_sweep = -1;                // option "pgrad_sweep": -1 by size, 0 the inverse route, 1 the sweep route whenever allowed
    int64_t pgrad_sweep_max = gpmi::PGRAD_SWEEP_MAX_DEFAULT;   // option "pgrad_sweep_max" (gpmi_pgrad_plan.h: PGRAD_SWEEP_MAX_DEFAULT, measured)
    DevBuf pgW, pgpart, pgsum;
    DevBuf loov, loow;       // gpmi_loo / gpmi_loo_grad: the per-point vectors; the NB x ld row block of K_y^-1 D
    // binary classification (laplace.hip): A holds the factor of B = I + W^1/2 K W^1/2 at the mode f^, lap holds f^,
    // grad log p(y|f^) and W^1/2 (with the Newton iterates), lap_part the tile partials of the matrix-vector products.
    DevBuf lap, lap_part, lap_out;
    // multi-class classification (softmax.hip): A holds M = chol(sum_c E_c) at the mode, sm_E the C matrices -E_c (full,
    // symmetric), sm the C x Np vectors (Y - P among them).  K and V = S_c L_c^-T are scratch of the fit and live in Kn
    // and U (the scratch of gpmi_lml_grad).
    int sm_classes = 0;
    DevBuf sm, sm_part, sm_E, sm_B, sm_out;
    // sparse regression with inducing points (sparse.hip): sp_L holds L = chol(K_uu + jitter I) (sp_mp x sp_ld), sp_B the
    // factor L_B of B = I + A~ A~^T with c = L_B^-1 A~ y~ in its row sp_mp, sp_Z the (scaled) inducing inputs, sp_q the N
    // values q_i, sp_W the slab workspace (sp_wrows x sp_ld) that prediction reuses for its chunks of test rows.  A is
    // not touched.
    int sp_method = 0, sp_fused = 1;
    int64_t sparse_slab = 0;     // option "sparse_slab": training rows per slab (0 = by size), rounded up to 128
    int64_t sp_m = 0, sp_mp = 0, sp_ld = 0, sp_wrows = 0;
    Box boxU;                    // bounding box of the (scaled) inducing inputs
    DevBuf sp_Zraw, sp_Z, sp_L, sp_B, sp_W, sp_q, sp_vec, sp_part, sp_scr, sp_info, sp_pred;
    // gpmi_sparse_grad: three sp_mp x sp_ld matrices, the slab-sized E, the chunks' partial sums and the vectors -- workspaces
    // of its own, made at the first call, so that the resident fit above is only ever read.  They hold no state and go
    // when something other than a sparse fit takes the sparse fit's place: a regression factorisation, a classifier's
    // fit, a new training set (a sparse fit after a sparse fit, the tuner's step, keeps them).
    DevBuf sp_g0, sp_g1, sp_g2, sp_gE, sp_gpart, sp_gvec;
    void release_sparse_grad() {
        for (DevBuf* b : {&sp_g0, &sp_g1, &sp_g2, &sp_gE, &sp_gpart, &sp_gvec}) b->release();
    }
    // timers
    std::vector<hipEvent_t> ev_pool;
    size_t ev_used = 0;
    std::vector<TimedSpan> spans;
    double stage_ms[GPMI_T_COUNT] = {0};

    // nullptr (and ev_error set) if the runtime cannot create another event
    hipError_t ev_error = hipSuccess;
    hipEvent_t new_event() {
        if (ev_used == ev_pool.size()) {
            hipEvent_t e = nullptr;
            const hipError_t r = hipEventCreateWithFlags(&e, hipEventDefault);
            if (r != hipSuccess) { ev_error = r; return nullptr; }
            ev_pool.push_back(e);
        }
        return ev_pool[ev_used++];
    }
    static constexpr size_t NO_SPAN = (size_t)-1;
    // a span that cannot get its events is dropped (timers are diagnostics); ordering events are not optional
    size_t span_begin(int slot, hipStream_t st = nullptr) {
        if (!timing) return NO_SPAN;
        TimedSpan s{new_event(), new_event(), slot};
        if (!s.a || !s.b) return NO_SPAN;
        if (hipEventRecord(s.a, st ? st : stream) != hipSuccess) return NO_SPAN;
        spans.push_back(s);
        return spans.size() - 1;
    }
    void span_end(size_t idx, hipStream_t st = nullptr) {
        if (!timing || idx == NO_SPAN) return;
        if (hipEventRecord(spans[idx].b, st ? st : stream) != hipSuccess) spans[idx].slot = GPMI_T_COUNT - 1;
    }
    // make stream `waiter` wait for everything queued so far on `signaller`
    hipError_t order(hipStream_t signaller, hipStream_t waiter) {
        hipEvent_t e = new_event();
        if (!e) return ev_error;
        hipError_t r = hipEventRecord(e, signaller);
        if (r != hipSuccess) return r;
        return hipStreamWaitEvent(waiter, e, 0);
    }
    void timers_reset(std::initializer_list<int> slots) {
        for (int s : slots) stage_ms[s] = 0.;
    }
    // call after the stream has been synchronised
    void timers_collect() {
        for (auto& s : spans) {
            float ms = 0.f;
            if (hipEventElapsedTime(&ms, s.a, s.b) == hipSuccess) stage_ms[s.slot] += ms;
        }
        spans.clear();
        ev_used = 0;
    }
};


namespace gpmi {

// driver.hip
hipError_t panel_factor(hipStream_t s, double* A, int64_t ld, int64_t nb, int64_t mrows, int64_t col_offset,
                        int64_t* info);
hipError_t trsm_block(hipStream_t s, const double* L, int64_t ldl, double* X, int64_t ldx, int64_t m, int64_t nb);
hipError_t cholesky_inplace(gpmi_ctx* c, double* A, int64_t ld, int64_t ncols, int64_t nrows, int64_t* info,
                            bool account, int64_t carried_rows = 0);
hipError_t solve_sweep(gpmi_ctx* c, double* V, int64_t ldv, int64_t m, bool tri = false);
// the same sweep through any resident lower factor (ncols x ncols, leading dimension ld), not only the one in c->A
hipError_t solve_sweep_factor(gpmi_ctx* c, const double* L, int64_t ld, int64_t ncols, double* V, int64_t ldv, int64_t m,
                              bool tri = false);
// V = F^-T (upper triangular, n x n) for a resident lower factor F by that sweep on the identity, and Out = -V V^T on the
// lower tiles for such a V, one launch per row block of c->block(n) rows
hipError_t inverse_transposed(gpmi_ctx* c, const double* F, int64_t ldf, int64_t n, double* V, int64_t ldv);
hipError_t neg_gram_lower(gpmi_ctx* c, const double* V, double* Out, int64_t ld, int64_t n);
// Out -= V V^T on the lower tiles for a dense V (the caller zeroes Out before the first of a sum), the same row blocks
hipError_t neg_gram_lower_dense(gpmi_ctx* c, const double* V, double* Out, int64_t ld, int64_t n);
// The kernel-matrix launches of a context, ready for launch_rbf.  rbf_cross: rows row0 .. row0 + nrows of K(A, B) for point
// sets of nA and nB points with boxes ba and bb, ncols columns, nothing on the diagonal; the delta term of the composite
// kernel counts as on a square matrix only for the test set against a training set of the same size.  rbf_sym: the lower
// tiles of K(X, X) + diag_add I, npad x npad.
RbfArgs rbf_cross(const gpmi_ctx* c, const double* A, int64_t nA, const Box& ba, const double* B, int64_t nB, const Box& bb,
                  int64_t row0, int64_t nrows, int64_t ncols, double* out, int64_t ld);
RbfArgs rbf_sym(const gpmi_ctx* c, const double* X, int64_t n, const Box& box, double diag_add, int64_t npad, double* out,
                int64_t ld);
RbfArgs rbf_test_train(const gpmi_ctx* c, double* out, int64_t ld);      // K(X*, X), n_p x Np
int ensure_train_buffers(gpmi_ctx* c, int64_t test_rows = 0, bool test_cols = false);
// append.hip: k more observations into the resident regression factorisation (include/gpmi.h: gpmi_append)
int append_impl(gpmi_ctx* c, const double* Xnew, int64_t k, const double* ynew, double* lml, int64_t* bad_pivot);
// remove.hip: k observations out of the resident regression factorisation (include/gpmi.h: gpmi_remove)
int remove_impl(gpmi_ctx* c, const int64_t* idx, int64_t k, double* lml);
// with_test: the test set's rows K(X*, X) ride below the y rows (they come out as v^T = K_s^T L^-T, a7 inside a3) and
// mean / variance (a6, a8) are read off them behind the LML
// with_post (needs with_test): the test rows also get their own columns K_ss + jitter I, i.e. ONE Cholesky of
//   [[K + sI, .], [K_s^T, K_ss + jitter I]]  (N + n columns)  --  its last n columns are cholesky(K_ss + jitter I - v^T v), f1
int factorize_impl(gpmi_ctx* c, double sigma, double ell, double noise_var, double* lml, int64_t* bad_pivot,
                   bool with_test = false, double* mu = nullptr, double* out2 = nullptr, int want_sd = 1,
                   bool with_post = false, double jitter = 0.0);
// gpmi_api.hip: regenerate the scaled copy of the training / test inputs and its box (no-ops on an isotropic context)
int ard_rescale_train(gpmi_ctx* c);
int ard_rescale_test(gpmi_ctx* c);
void meanvar_to_host(gpmi_ctx* c, const std::vector<double>& h, double* mu, double* out2, int want_sd);
// regress.hip: L^T x = b on the resident fused factor (a5; the first call after a factorisation inverts its diagonal blocks)
hipError_t backward_solve_fused(gpmi_ctx* c, double* b, double* xout);
// x = L^-T m for the m of the y row, through the fused solve or the plain one as the resident factor asks: x2 holds 2 Np
// doubles, *x_out says where in it the solution lies; fail_gave_up: the status of a one-launch solve whose give-up word is set
hipError_t backward_solve_resident(gpmi_ctx* c, double* x2, double** x_out);
// the same for a right-hand side the caller has put into x2[0 .. Np) (zero past N), which leaves the y row alone
hipError_t backward_solve_rhs(gpmi_ctx* c, double* x2, double** x_out);
int fail_gave_up(const char* api);
// The end of a call that ran a backward solve, behind the caller's own device-to-host copies: the read of the one-launch
// solve's give-up word where that solve ran, the call's one synchronisation, the timers, the word's status under `api`
int solve_epilogue(gpmi_ctx* c, const char* api);
// predgrad.hip: the gradients of the predictive mean and variance at the resident test inputs
int predict_grad_impl(gpmi_ctx* c, double* mu, double* var, double* dmu, double* dvar);
// regress.hip: the regression calls of include/gpmi.h on the resident factorisation, behind the shims' pointer checks
int alpha_impl(gpmi_ctx* c, double* alpha_out);
// The body of the regression gradients' front, for any factor resident in A: the slot's timer reset, U, (want_kn) Kn and
// vec made large enough, then inside a span of that slot, which it opens: (alpha_out not null) alpha = L^-T m,
// U = L^-T by the TRSM sweep on the identity and (want_kn) Kn = -U U^T on the lower tiles
int factor_inverse_front(gpmi_ctx* c, int slot, bool want_kn, double** alpha_out, size_t* span);
// The ending of the three ARD traces (gpmi_lml_grad_ard, gpmi_laplace_grad, gpmi_softmax_grad; regress.hip's
// tile_sums_finish, in which gpmi_lml_grad_co2 ends too).  grad_ard_finish, given
// the arguments with the caller's inputs: gpart and gsum sized, the trace, the span's end, the launches' plain sums on the
// host behind the call's one synchronisation, timers collected; solve_api not null: a backward solve ran in this call and
// its give-up word is read and reported under that name.  grad_ard_scale: the derivatives asked for (null: skipped) from
// the sums, d_r[k] = sig2 sum_k / (2 l2 r_k), d_ell, d_sigma and the noise slot; l2 is l^2 (a Matern family's 1 / a^2).
int grad_ard_finish(gpmi_ctx* c, GradArdArgs& a, size_t span, const char* solve_api, std::vector<double>* sums);
void grad_ard_scale(const gpmi_ctx* c, const GradArdArgs& a, const std::vector<double>& sums, double l2, double* d_r,
                    double* d_ell, double* d_sigma, double* d_noise);
// the front of the three predictions: whatever v was kept goes, V is made n_p x (Np + ld_pad) and K(X*, X) is built
// into it, inside a span of ks_slot where that is not negative
int predict_front(gpmi_ctx* c, int ks_slot);
int predict_resident_impl(gpmi_ctx* c, double* mu, double* out2, int want_sd);
int lml_grad_impl(gpmi_ctx* c, double* d_ell, double* d_sigma);
int lml_grad_ard_impl(gpmi_ctx* c, double* d_r, double* d_ell, double* d_sigma, double* d_noise);
int lml_grad_co2_impl(gpmi_ctx* c, double* d_theta, double* d_noise);
int loo_impl(gpmi_ctx* c, double* mu, double* var, double* logp, double* loo);
int loo_grad_impl(gpmi_ctx* c, double* d_ell, double* d_sigma, double* d_noise);
int grad_trace_impl(gpmi_ctx* c, const double* a_in, const double* b_in, int64_t N, int64_t d, double sigma, double ell,
                    const double* alpha_in, const double* Kinv_in, double* d_ell, double* d_sigma);
int post_chol_impl(gpmi_ctx* c, double jitter, double* L_out, int64_t* bad_pivot);
int post_sample_impl(gpmi_ctx* c, double jitter, const double* Z, int64_t num_fun, double* LZ_out, int64_t* bad_pivot);
// the context's options with the panel kind of the resident factor: solve with the kind of leaves that produced it
inline Tuning resident_tuning(const gpmi_ctx* c) {
    Tuning tn = c->tune;
    tn.panel_fused = c->res.factor_fused;
    return tn;
}

// laplace.hip: GPML Algorithms 3.1 (Newton iteration for the mode, logistic likelihood) and 3.2 (prediction)
int laplace_fit_impl(gpmi_ctx* c, double sigma, double ell, double tol, int max_iter, double* log_q, int* iters,
                     int* converged, double* f_hat);
int laplace_predict_impl(gpmi_ctx* c, double* f_mean, double* f_var, double* prob);
int laplace_grad_impl(gpmi_ctx* c, double* d_r, double* d_ell, double* d_sigma);
// The Newton skeleton of both classifiers (laplace.hip); the loop itself is newton_iterate of gpmi_state.h, which each fit
// gives a problem object.  classifier_fit_check: the arguments both take, under the caller's API name; `own` is the text of
// a failed check of the caller's own arguments (or null), reported at its place behind the kernel check.
// classifier_labels_check: y on the host (one synchronisation) and `text`, behind the API name, for a label that fails ok(label, n_classes).
// classifier_fit_begin: the resident fit goes, A and the hyper-parameters are set up, the backward solve's give-up word
// (*chain: it is read from the first iteration on) and the pivot word are reset.  newton_readback, behind the caller's
// per-point kernel: Psi from its partials with the pivot and give-up words in one record, h = {Psi, pivot word, give-up
// word}, the iteration's one synchronisation, and the record's status under the caller's API name and pivot text.
constexpr int64_t NO_BAD_PIVOT = std::numeric_limits<int64_t>::max();
int classifier_fit_check(const gpmi_ctx* c, const char* api, const char* own, double sigma, double ell, double tol,
                         int max_iter);
int classifier_labels_check(gpmi_ctx* c, const char* api, bool (*ok)(double label, int n_classes), int n_classes,
                            const char* text);
int classifier_fit_begin(gpmi_ctx* c, double sigma, double ell, bool* chain);
hipError_t launch_newton_psi(hipStream_t st, const double* psi_part, int64_t nblk, const int64_t* info, const int* flag,
                             double* out);
int newton_readback(gpmi_ctx* c, const double* psi_part, int64_t nblk, bool chain, double* rec, double (&h)[3],
                    const char* api, const char* pivot_text);
void laplace_quad_nodes(double sig2, int* M, double* T, double* h);

// softmax.hip: GPML Algorithms 3.3 (Newton iteration for the mode, softmax likelihood, C latent functions with one shared
// prior) and 3.4 (prediction)
int softmax_fit_impl(gpmi_ctx* c, int n_classes, double sigma, double ell, double tol, int max_iter, double* log_q,
                     int* iters, int* converged, double* f_hat);
int softmax_predict_impl(gpmi_ctx* c, double* mu, double* cov, int64_t n_samples, const double* normals, double* prob);
int softmax_grad_impl(gpmi_ctx* c, double* d_r, double* d_ell, double* d_sigma);

// sparse.hip: sparse regression with m inducing inputs (VFE / FITC) in the whitened form, and its prediction
int sparse_fit_impl(gpmi_ctx* c, const double* Z, int64_t m, double sigma, double ell, double noise_var, double jitter,
                    int method, double* value, int64_t* bad_pivot);
int sparse_predict_impl(gpmi_ctx* c, double* mu, double* out2, int want_sd);
int sparse_get_impl(gpmi_ctx* c, double* c_out, double* q_out);
int sparse_grad_impl(gpmi_ctx* c, double* d_ell, double* d_sigma, double* d_noise, double* d_r, double* d_Z);
// B_lower (mp x mp, leading dimension ldb) += V^T V for the row-major slab V (rows x mp, leading dimension ldv; rows and
// mp multiples of 128) on the matrix pipe; part: gram_part_doubles(rows, mp) doubles of workspace
int64_t gram_part_doubles(int64_t rows, int64_t mp);
hipError_t launch_gram_tn(hipStream_t s, const double* V, int64_t ldv, int64_t rows, int64_t mp, double* part, double* B,
                          int64_t ldb);

}  // namespace gpmi
