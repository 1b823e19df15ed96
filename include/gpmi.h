/*
 * gpmi.h -- C-ABI of libgpmi355x.so, the MI355X (gfx950) implementation of the
 * GP-regression hot path of happyjin/Gaussian_process.
 *
 * The reference has no FFI/plugin interface: its boundary is a set of plain
 * Python functions other scripts import.  Each entry point
 * below names the reference statement(s) it replaces; the Python shim in
 * gaussian_process_amd/ binds them with ctypes and keeps the reference's
 * function signatures.  All matrices are float64, row-major, caller-owned host
 * buffers unless the name says `_dev` (device pointers for the multi-GPU
 * driver).  No torch types cross this boundary.
 *
 * Every function returns an int status:
 *   GPMI_OK            0
 *   GPMI_ERR_NOT_PD    1  Cholesky met a non-positive pivot (reference:
 *                         numpy.linalg.LinAlgError from np.linalg.cholesky,
 *                         GP_regression.py:138,154); *bad_pivot = 1-based index
 *   GPMI_ERR_BAD_ARG   2  -> ValueError in the shim
 *   GPMI_ERR_RUNTIME   3  HIP runtime failure -> RuntimeError; text in
 *                         gpmi_last_error()
 * Nothing aborts the process.  A context is not thread-safe (one per thread).
 */
#ifndef GPMI_H
#define GPMI_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define GPMI_OK 0
#define GPMI_ERR_NOT_PD 1
#define GPMI_ERR_BAD_ARG 2
#define GPMI_ERR_RUNTIME 3

#define GPMI_ABI_VERSION 4

/* stage timer slots filled by gpmi_get_timers (milliseconds, hipEvent-timed on
 * the context's compute stream; 0 when the stage did not run in the last call) */
enum {
    GPMI_T_KBUILD = 0,    /* a1+a2: K(X,X)+s*I lower tiles                */
    GPMI_T_CHOL = 1,      /* a3 (+a4 folded in): blocked Cholesky, total   */
    GPMI_T_CHOL_PANEL = 2,/*    of which: diagonal block + panel TRSM      */
    GPMI_T_CHOL_TRAIL = 3,/*    of which: trailing SYRK/GEMM updates       */
    GPMI_T_LML = 4,       /* a10: reductions for the log-marginal-likelihood */
    GPMI_T_KS = 5,        /* a1 for K(X*,X) (transposed K_s)               */
    GPMI_T_SOLVE_V = 6,   /* a7: v = L^-1 K_s (TRSM sweep), total          */
    GPMI_T_MEANVAR = 7,   /* a6+a8: mean / variance reductions             */
    GPMI_T_ALPHA = 8,     /* a5: backward solve L^T alpha = m              */
    GPMI_T_POSTCHOL = 9,  /* f1: v^T v, K** + jitter*I - v^T v, its Cholesky */
    GPMI_T_TRAIL_LAUNCHES = 10, /* number of trailing-update launches in last fit */
    GPMI_T_TRAIL_FLOPS = 11,    /* algorithmic flops of those launches: 2K per element on or below the diagonal, real rows + the y row */
    GPMI_T_GRAD = 12,     /* f2: L^-T, K_y^-1 and the fused gradient trace */
    GPMI_T_LOO = 13,      /* gpmi_loo / gpmi_loo_grad: the whole device span of the last of the two */
    GPMI_T_SPARSE = 14,   /* gpmi_sparse_fit: the whole device span of the last sparse fit */
    GPMI_T_COUNT = 16
};

typedef struct gpmi_ctx gpmi_ctx;

int gpmi_abi_version(void);
/* text of the last GPMI_ERR_RUNTIME / GPMI_ERR_BAD_ARG on this thread */
const char* gpmi_last_error(void);
int gpmi_device_count(int* count);

/* one context = one GPU (device ordinal) + its streams and workspaces */
int gpmi_ctx_create(int device, gpmi_ctx** out);
int gpmi_ctx_destroy(gpmi_ctx* ctx);
/* tuning knobs; unknown names -> GPMI_ERR_BAD_ARG.
 * per context:  "nb" (outer Cholesky block, 0 = by size), "ld_pad" (doubles added to leading dimensions),
 *               "timing" (0/1: hipEvent stage timers), "lookahead" (0/1), "la_min" (columns from which lookahead is used,
 *               default 12288), "lanes" (factorisations in flight in gpmi_lml_batch, 0 = by size),
 *               "sparse_slab" (gpmi_sparse_fit: training rows per slab, rounded up to 128; 0 = by size (16384).  It bounds
 *               the slab workspace to that many rows of m + "ld_pad" doubles whatever N is; same results to rounding),
 *               "shallow_min" (under lookahead, panels with fewer columns left than this use the one-launch panel
 *               kernels: the update they would run beside is over long before they are; default 6144, 0 = never);
 *               kernel selection (for measurements; also per context -- the lanes of gpmi_lml_batch inherit them):
 *               "panel_fused" (0/1: 128-column MFMA panel kernels / first-generation 64-column leaves),
 *               "gemm_dma" (0/1), "gemm_dma_waves" (4/8), "gemm_small_tiles" (0/1), "gemm_small_dma" (0/1),
 *               "gemm_persist" (0/1: resident workgroups for update GEMMs that have the chip to themselves),
 *               "gemm_tall" (0/1: 256 x 128 blocks for per-tile update launches of at least "tall_min_tiles" live
 *               128 x 128 tiles, default 12288 -- "tall_min_tiles_slack", default 1024, in a Cholesky of 49152 columns
 *               and more under lookahead, whose panel chain is far off the critical path),
 *               "trsv_vinv" (backward solve: 2 ONE launch, column blocks chained through the solution vector, with the
 *               inverted 128 x 128 diagonal blocks -- the default; 1 one launch per block with the same inverses; 0 the
 *               16 x 16 rounds),
 *               "trsm_wave" (0/1), "rbf_blocks" (persistent blocks of the K build);
 *               gpmi_append: "reserve" (default 0: from the next fit on A is sized for N + reserve points, so that appends
 *               up to that size stay in place; setting it drops nothing), "append_skinny" (k <= 16 on a fused factor:
 *               -1 by size -- the default --, 0 the padded 128-row sweep, 1 the <= 16-row sweep kernel whenever allowed);
 *               gpmi_remove: "remove_keep_spare" (default 0: the buffer a removal leaves behind is freed; 1: it is kept
 *               as the target of the next removal, so a remove / append cycle allocates nothing; any fit drops it, and
 *               so does setting the option back to 0);
 *               gpmi_predict_grad_resident: "pgrad_sweep" (-1 by size -- the default --, 0 the inverse route, 1 the
 *               backward sweep whenever the factor is fused), "pgrad_sweep_max" (default 4096: the largest n
 *               that takes the sweep under "by size"; profiles/r17_predgrad_rate.txt).
 * The context-free gpmi_dev_* primitives run with the defaults. */
int gpmi_set_option(gpmi_ctx* ctx, const char* name, int64_t value);

/* RBF_kernel(a, b, sigma, l)                         GP_regression.py:8-19
 *   out[i*M + j] = sigma^2 * exp(-.5 * (1/l^2) * sum_k (a[i,k]-b[j,k])^2)
 * a: N x d, b: M x d, out: N x M. */
int gpmi_rbf(gpmi_ctx* ctx, const double* a, int64_t N, const double* b, int64_t M,
             int64_t d, double sigma, double ell, double* out);

/* The reference's other covariance functions, same layout as gpmi_rbf:
 *   kind 0: RBF_kernel (p0 = sigma, p1 = l)                               GP_regression.py:8-19
 *   kind 1: lin_kernel(a, b, c): np.dot(a - c, b.T - c), p0 = c            GP_regression.py:22-33
 *   kind 2: per_kernel(a, b, (p, l)): exp(-2 sin(pi|a-b|/p)^2 / l^2), d = 1, p0 = p, p1 = l   :36-50
 * and the Matern family (Rasmussen & Williams, GPML, section 4.2.1), which the reference does not have:
 *   kind 4: nu = 1/2,  kind 5: nu = 3/2,  kind 6: nu = 5/2      (p0 = sigma, p1 = l, any d)
 *   K_ij = sigma^2 P(t) exp(-t),  t = a sqrt(sq_ij),  a = sqrt(2 nu) / |l|,  sq_ij = sum_k (z_ik - z_jk)^2
 *   P = 1 (nu = 1/2),  1 + t (3/2),  1 + t + t^2 / 3 (5/2)
 * z = x, or x / r with lengthscales set (gpmi_set_lengthscales).  l == 0 and NaN are refused as for kind 0; a negative
 * l means |l|.  Evaluation order (only exp itself may differ from a NumPy float64 evaluation in this order):
 *   1. sq in the pairwise order of kind 0 (NumPy's add.reduce over the middle axis of the (N, d, M) differences);
 *   2. r = sqrt(sq), correctly rounded;
 *   3. t = a * r, a = sqrt(2 nu) / |l| computed once on the host in double (sqrt(1.0), sqrt(3.0), sqrt(5.0));
 *   4. P = 1 + t, or (1 + t) + (t * t) * c3 with c3 the double nearest 1/3 -- one rounding per operation, no FMA;
 *   5. e = exp(-t), K = sigma^2 * (P * e).
 * At sq == 0 every factor is exactly 1: the diagonal of K is sigma^2 exactly. */
int gpmi_cov(gpmi_ctx* ctx, int kind, const double* a, int64_t N, const double* b, int64_t M,
             int64_t d, double p0, double p1, double* out);
/* Covariance function used by gpmi_factorize / gpmi_predict / gpmi_post_chol from now on
 * (kernel_choice of prediction(), GP_regression.py:125-136).  kind 0 (default) takes sigma and l
 * from gpmi_factorize; kinds 1, 2 take (p0, p1) as above and ignore them.  Kinds 4, 5, 6 (Matern nu = 1/2, 3/2, 5/2)
 * take sigma and l from gpmi_factorize and its siblings exactly as kind 0 does, and ignore p0 and p1. */
int gpmi_set_kernel(gpmi_ctx* ctx, int kind, double p0, double p1);
/* The composite covariance of the CO2 example (second half):
 *   kind 3: covariance_function(a, b, hyperparms) = kernel_1 + kernel_2 + kernel_3 + kernel_4,
 *           hyperparms = theta_1..theta_11, any d                            CO2_example.py:9-94
 * kernel_4 adds theta_11^2 on row == col whenever the matrix is square (N == M), as the reference
 * does (:58-59).  The *_params forms take the parameters as an array; kinds 0-2 and 4-6 accept
 * nparams == 2 with (p0, p1) as above. */
int gpmi_cov_params(gpmi_ctx* ctx, int kind, const double* a, int64_t N, const double* b, int64_t M,
                    int64_t d, const double* params, int nparams, double* out);
int gpmi_set_kernel_params(gpmi_ctx* ctx, int kind, const double* params, int nparams);

/* Copy the training set to the device (X: N x d, y: N).  Replaces nothing in
 * the reference (it has no device); separates PCIe from the timed path. */
int gpmi_set_train(gpmi_ctx* ctx, const double* X, int64_t N, int64_t d, const double* y);

/* K = RBF_kernel(X,X,sigma,l); L = cholesky(K + s*I); m = solve(L, y)
 *                    GP_regression.py:126,138-139; tune_hyperparms_regression.py:306-308
 * and the log-marginal-likelihood of tune_hyperparms_regression.py:312:
 *   lml = -.5*y^T alpha - sum(log(diag L)) - N/2*log(2*pi)   (y^T alpha = m^T m)
 * Leaves L and m resident in the context.  lml/bad_pivot may be NULL. */
int gpmi_factorize(gpmi_ctx* ctx, double sigma, double ell, double noise_var,
                   double* lml, int64_t* bad_pivot);

/* gpmi_set_train + gpmi_factorize in one call (host buffers in). */
int gpmi_fit(gpmi_ctx* ctx, const double* X, int64_t N, int64_t d, const double* y,
             double sigma, double ell, double noise_var, double* lml, int64_t* bad_pivot);

/* k more observations (Xnew: k x d, ynew: k) into the resident REGRESSION factorisation, in O(N^2 k): afterwards the
 * context is what gpmi_fit on [X; Xnew], [y; ynew] with the resident kernel, lengthscales, sigma, ell and noise_var would
 * have left -- N + k points, L, m = L^-1 y, and in *lml the LML of the N + k points -- to rounding (the factor's leading
 * floor(N / 128) 128 rows are the resident ones bit for bit).  Every consumer of a regression fit works on it unchanged;
 * v of a resident test set is dropped (gpmi_predict_resident recomputes it; gpmi_post_* ask for that first).
 * With N0 = floor(N / 128) 128 only the border, rows [N0, ceil((N + k) / 128) 128), is built: its rows of K against the
 * first N0 points swept through the resident factor (k <= 16 on a fused factor: the k new rows alone, by the kernel
 * behind gpmi_dev_border_sweep; otherwise all border rows by the 128-row TRSM sweep; option "append_skinny"), one
 * rank-N0 update of the border block and the y row, and the Cholesky of that block.  It works in place while the
 * padded size fits the resident allocation (always inside the padding; beyond it with option "reserve"), and otherwise
 * moves the leading N0 x N0 square into an allocation of the size a fresh fit would choose; if that allocation fails the
 * call returns GPMI_ERR_RUNTIME with the old fit intact.  A runtime error behind the allocations (a copy, a launch)
 * also returns GPMI_ERR_RUNTIME, but then as a failed pivot does: no fit resident, the training set the extended one
 * (gpmi_get_layout tells N), gpmi_factorize works on it.
 * Refused (GPMI_ERR_BAD_ARG, nothing changed): no regression factorisation resident ("no factorisation resident"),
 * k < 1, NaN in Xnew or ynew, the composite kernel (kind 3).  Kinds 0, 1, 2, 4, 5, 6 and per-dimension lengthscales are
 * supported.  A failed pivot of the border returns GPMI_ERR_NOT_PD with *bad_pivot its 1-based index among the N + k
 * points and *lml NaN: the fit is dropped, the EXTENDED training set stays resident (gpmi_factorize works on it).
 * Timers: GPMI_T_KS the row builds, GPMI_T_SOLVE_V the sweep, GPMI_T_CHOL the border update and factorisation,
 * GPMI_T_LML.  lml / bad_pivot may be NULL. */
int gpmi_append(gpmi_ctx* ctx, const double* Xnew, int64_t k, const double* ynew, double* lml, int64_t* bad_pivot);
/* The k observations at the distinct 0-based positions idx (any order) of the resident ordering out of the resident
 * REGRESSION factorisation, in O(N^2 k): afterwards the context is what gpmi_fit on the surviving points, in their
 * relative order, with the resident kernel, lengthscales, sigma, ell and noise_var would have left -- N - k points, L,
 * m = L^-1 y, and in *lml the LML of the N - k points -- to rounding.  With J0 = floor(min(idx) / 128) 128 the leading
 * J0 x J0 block of the factor is the resident one bit for bit.  Every consumer of a regression fit works on the result
 * unchanged (gpmi_append included); v of a resident test set is dropped (gpmi_predict_resident recomputes it; gpmi_post_*
 * ask for that first).  No element of K is evaluated: every covariance kind is served, the composite kind 3 included.
 * The rows S of L that survive satisfy L_S L_S^T = K_y[S, S]; plane rotations of the surviving columns against the
 * removed ones, left to right, make L_S triangular again -- a POSITIVE rank-k update of the trailing factor, so no
 * pivot can fail.  One sweep carries up to 16 removed columns; more go in descending groups of 16 (the largest first).
 * Each sweep is one launch per 128-column block from its J0 on and one more for the y row, reads the old trailing
 * trapezoid once and writes the new one once, out of place, into a second buffer of the resident shape (leading
 * dimension and rows stay: a removal never shrinks the allocation; the y row moves to row ceil((N - k) / 128) 128);
 * rows and columns below J0 move with one 2-D copy.  Afterwards the old buffer is freed, or kept for the next removal
 * under option "remove_keep_spare".  A fused factor (option "panel_fused" 1 at fit time) gets the inverses of its new
 * 16 x 16 diagonal tiles from tile J0 / 16 on; a first-generation factor has none and stays of its kind.  The same
 * removal from the same fit gives the same bits every run.
 * The training set is compacted on the device (X, y, the scaled inputs); the lanes of gpmi_lml_batch forget their copy.
 * Refused (GPMI_ERR_BAD_ARG, nothing changed): no regression factorisation resident ("no factorisation resident"), a
 * null idx, k < 1, k >= N, an index outside [0, N), a duplicate index.  Every allocation happens before anything of the
 * resident fit changes: if one fails the call returns GPMI_ERR_RUNTIME with the old fit intact.  A runtime error behind
 * the allocations (a copy, a launch) also returns GPMI_ERR_RUNTIME, but then as in gpmi_append: no fit resident, the
 * training set the REDUCED one (gpmi_get_layout tells N), gpmi_factorize works on it.
 * Timers: GPMI_T_SOLVE_V the sweeps, GPMI_T_CHOL the tile inverses, GPMI_T_LML; GPMI_T_KS holds what only moves (the
 * 2-D copy, the rows' columns below J0, the new padding).  lml may be NULL. */
int gpmi_remove(gpmi_ctx* ctx, const int64_t* idx, int64_t k, double* lml);
/* The layout of the resident training set and factor, for tests and the rate script: out5 = {N, Np (N padded to 128),
 * the leading dimension of A, the rows A is laid out for, the route of the last gpmi_append that got as far as its sweep: 1 skinny,
 * 0 padded, -1 none yet}.  The leading dimension and the rows are 0 until a fit has sized A. */
int gpmi_get_layout(gpmi_ctx* ctx, int64_t* out5);

/* alpha = solve(L.T, m)                               GP_regression.py:140
 * out: N doubles. */
int gpmi_get_alpha(gpmi_ctx* ctx, double* alpha_out);
/* m = solve(L, y) (GP_regression.py:139) and diag(L); each N doubles. */
int gpmi_get_m(gpmi_ctx* ctx, double* m_out);
int gpmi_get_diag(gpmi_ctx* ctx, double* diag_out);
/* rows [r0,r1) x cols [c0,c1) of the resident factor, lower part, zeros above
 * the diagonal (np.linalg.cholesky convention); for tests and small N. */
int gpmi_get_factor_block(gpmi_ctx* ctx, int64_t r0, int64_t r1, int64_t c0, int64_t c1,
                          double* out);

/* Copy test inputs to the device (Xs: n x d, d as in set_train). */
int gpmi_set_test(gpmi_ctx* ctx, const double* Xs, int64_t n);

/* K_s = RBF_kernel(X, Xs); mu = K_s.T @ alpha; v = solve(L, K_s);
 * var = diag(K_ss) - sum(v**2, 0); sd = sqrt(var)     GP_regression.py:127,143-148
 * mu, out2: n doubles each; out2 = sd if want_sd else var.  A negative var
 * gives NaN sd, as np.sqrt does in the reference (no clamp).  Either output
 * may be NULL.  v stays resident (transposed, n x N) for gpmi_post_chol. */
int gpmi_predict_resident(gpmi_ctx* ctx, double* mu, double* out2, int want_sd);
int gpmi_predict(gpmi_ctx* ctx, const double* Xs, int64_t n, double* mu, double* out2,
                 int want_sd);

/* prediction() in one pass: gpmi_factorize + gpmi_predict_resident for a training and a test set that are both
 * resident (gpmi_set_train, gpmi_set_test), GP_regression.py:109-156 (a1-a8).  K(X*, X) rides below the y row through
 * the Cholesky, so a7 (v = L^-1 K_s) has no launches of its own.  lml / bad_pivot as gpmi_factorize, mu / out2 / want_sd
 * as gpmi_predict_resident; alpha, post_chol and lml_grad work on the result as after the two calls.  Results agree with
 * the two-call form to rounding (not bit for bit: the two sweeps' block widths differ). */
int gpmi_fit_predict_resident(gpmi_ctx* ctx, double sigma, double ell, double noise_var, double* lml, int64_t* bad_pivot,
                              double* mu, double* out2, int want_sd);

/* ... and with the posterior-sample factor of GP_regression.py:154 in the same pass: one Cholesky of the augmented matrix
 *   [[K + sI, .], [K(X*, X), K_ss + jitter I]]   (N + n columns, the y rows below): its last n columns are
 *   L_ = cholesky(K_ss + jitter I - v.T @ v), the Schur complement the trailing updates leave there.  Arguments as
 * gpmi_fit_predict_resident plus jitter and L_out (n x n row-major, zeros above the diagonal; may be NULL -- gpmi_post_chol
 * with the same jitter then only downloads it).  GPMI_ERR_NOT_PD for a pivot of K + sI (:138) or of the posterior covariance
 * (:154; bad_pivot then counts from the posterior's own first column).  LML, alpha, mean and variance as the other forms to
 * rounding (the leading dimension and the block boundaries differ); L_ as gpmi_post_chol to rounding. */
int gpmi_fit_predict_sample_resident(gpmi_ctx* ctx, double sigma, double ell, double noise_var, double jitter, double* lml,
                                     int64_t* bad_pivot, double* mu, double* out2, int want_sd, double* L_out);

/* L_ = cholesky(K_ss + jitter*I - v.T @ v)            GP_regression.py:154
 * for the test set of the last predict; L_out: n x n row-major, zeros above the
 * diagonal.   */
int gpmi_post_chol(gpmi_ctx* ctx, double jitter, double* L_out, int64_t* bad_pivot);

/* L_ @ Z for f_post = mu + L_ @ normals (GP_regression.py:155) without bringing L_ (n x n) to the host: Z (n x num_fun
 * row-major; the caller's normals, drawn on the host so that np.random's order stays the reference's) goes up, LZ_out
 * (n x num_fun) comes down.  L_ is the factor gpmi_post_chol(jitter) returns -- the resident one when it rode through
 * gpmi_fit_predict_sample_resident or an earlier call formed it for this jitter, else formed now (status and bad_pivot as
 * gpmi_post_chol).  Row sums are added in a fixed order (bitwise reproducible); against np.dot they differ by rounding. */
int gpmi_post_sample(gpmi_ctx* ctx, double jitter, const double* Z, int64_t num_fun, double* LZ_out, int64_t* bad_pivot);

/* Gradients of the predictive mean and variance with respect to the test inputs, at the resident regression
 * factorisation and the resident test set (gpmi_set_test).  With z = x / r (r: gpmi_set_lengthscales, all 1 when none
 * are set), k_j = k(z*, z_j), alpha = K_y^-1 y and w = K_y^-1 k = L^-T v, v = L^-1 k:
 *   dmu/dx*_k  =      sum_j alpha_j D_jk            dvar/dx*_k = -2 sum_j w_j D_jk
 *   D_jk = dk_j/dx*_k = -k_j (z*_k - z_jk) / (l^2 r_k)                     kind 0
 *                      = -sigma^2 a^2 H(t_j) (z*_k - z_jk) / r_k            kinds 4, 5, 6 (a, t, H as at gpmi_lml_grad)
 * (the prior term sigma^2 of var does not depend on x* for these kinds).  An element with sq_j == 0 contributes 0; for
 * nu = 1/2 the kernel has no derivative there.  The derivatives are with respect to the raw, unscaled x* as the caller
 * passed it (gpmi_sparse_grad treats Z the same way).
 * mu, var: n doubles each, bit for bit what gpmi_predict_resident(want_sd = 0) computes from the same v.  dmu, dvar:
 * n x d row-major.  Every pointer may be NULL.  There is no want_sd: dsd = dvar / (2 sd) is the caller's.
 * v: formed exactly as gpmi_predict_resident forms it when it is not resident (and left resident); reused when it is,
 * wherever it lies (in V, or below the y row after the one-pass and augmented fits).  It is never written:
 * gpmi_post_chol, gpmi_post_sample and gpmi_predict_resident return the same bits before and after.
 * W (row i: w_i) goes to a buffer of the context's own (n_p x (N_p + ld_pad) doubles, grown on demand, released by the
 * next fit) by one of two routes, chosen by gpmi_pgrad_plan.h:
 *   sweep    a copy of v through gpmi_dev_back_sweep: O(N^2 n), no N^3 term; a fused factor only;
 *   inverse  U = L^-T by the forward sweep on the identity (N^3 / 3, the buffer of gpmi_lml_grad), W = V U^T by the routed
 *            GEMM; serves a first-generation factor ("panel_fused" 0 at fit time) and large n.
 * Options: "pgrad_sweep" -1 by size (the default), 0 always the inverse route, 1 the sweep route whenever allowed;
 * "pgrad_sweep_max" the largest n that takes the sweep route under "by size" (default 4096: the largest measured n at
 * which the sweep wins at N = 16384, d = 8 -- 62.2 against 62.7 ms there, 3.02 against 31.8 ms at n = 16;
 * profiles/r17_predgrad_rate.txt).  With
 * dvar == NULL nothing is swept backwards: the call costs alpha and one O(n N d) pass.
 * The pass regenerates K(X*, X) on the fly (never stored), reads W once and adds per-(row, 1024-column chunk) partial
 * sums in index order: no atomics, the same bits every run.
 * GPMI_ERR_BAD_ARG, nothing changed: no regression factorisation resident, no test set, a kernel kind other than 0, 4, 5,
 * 6, d > 32 (a test point's 2 d sums are kept in registers, as in gpmi_sparse_grad).  The single-launch backward solve's
 * give-up word is reported as by gpmi_get_alpha.  Timers: GPMI_T_ALPHA alpha, GPMI_T_KS and GPMI_T_SOLVE_V v and the
 * route to W, GPMI_T_MEANVAR the row dots and the pass. */
int gpmi_predict_grad_resident(gpmi_ctx* ctx, double* mu, double* var, double* dmu, double* dvar);

/* Gradient of the log marginal likelihood at the resident factorisation:
 *   d_ell   = .5 * trace((alpha alpha^T - K_y^-1) @ l_grad),     l_grad     = sigma^2 exp(-.5 sqdist/l^2) sqdist/l^3
 *                                                     tune_hyperparms_regression.py:54-57
 *   d_sigma = .5 * trace((alpha alpha^T - K_y^-1) @ sigma_grad), sigma_grad = 2 sigma exp(-.5 sqdist/l^2)
 *                                                     tune_hyperparms_regression.py:46-51 (commented out there)
 * with K_y^-1 = inv(L.T) @ inv(L) (:144) formed on the device from the resident L.
 * Kinds 0, 4, 5 and 6 (another kind -> GPMI_ERR_BAD_ARG).  For the Matern kinds, with H(t) = -(1/t) d(P e^-t)/dt =
 * e^-t / t (nu = 1/2), e^-t (3/2), (1 + t) e^-t / 3 (5/2):  dK_ij/dl = sigma^2 a^2 H(t_ij) sq_ij / l,  dK/dsigma = 2 K / sigma;
 * an element with sq_ij == 0 contributes 0 to d_ell (H(t) sq -> 0; duplicate training points are fine for nu = 1/2).
 * With lengthscales set (gpmi_set_lengthscales) sqdist is that of the scaled inputs and d_ell the derivative w.r.t. the
 * common multiplier l. */
int gpmi_lml_grad(gpmi_ctx* ctx, double* d_ell, double* d_sigma);
/* Per-dimension lengthscales (automatic relevance determination).  The context carries relative lengthscales r_k > 0,
 * k < d (default: all 1), and every squared-exponential covariance it builds becomes
 *   K_ij = sigma^2 exp(-.5 / l^2 * sum_k ((x_ik - x_jk) / r_k)^2)
 * (a Matern covariance, kinds 4-6, takes the same sum as its sq_ij)
 * -- the effective lengthscale of dimension k is l * r_k, with l the argument every call already takes.  The scaling is
 * done on the inputs: z = x / r, one IEEE division per element on the device, and factorisation, prediction, posterior
 * samples, gpmi_lml_batch, both Laplace classifiers and the gradients read z.  gpmi_rbf / gpmi_cov take their inputs as
 * arguments and are not affected.
 *   r == NULL or d == 0: back to the isotropic state (the context then reads the buffers it always read).
 *   otherwise every r_k must be finite and > 0 and d must equal the resident training set's d (GPMI_ERR_BAD_ARG).
 * May be called before or after gpmi_set_train / gpmi_set_test and repeatedly: the raw inputs stay on the device and the
 * scaled copies are regenerated there (d doubles go up).  Drops any resident regression factor, binary Laplace fit and
 * softmax fit, as a new gpmi_set_train does.  A later gpmi_set_train with another d clears the lengthscales; one with the
 * same d keeps them.  Squared-exponential and Matern kernels (kinds 0, 4, 5, 6): a fit with kind 1, 2 or 3 is refused while
 * they are set. */
int gpmi_set_lengthscales(gpmi_ctx* ctx, const double* r, int64_t d);
/* The gradient of the log marginal likelihood w.r.t. every hyper-parameter at the resident factorisation, with
 * W = alpha alpha^T - K_y^-1 and z = x / r (z = x when no lengthscales are set):
 *   d_r[k]  = .5 * sum_ij W_ij K_ij (z_ik - z_jk)^2 / (l^2 r_k)     (d doubles; d LML / d r_k)
 *             Matern kinds: .5 * sum_ij W_ij sigma^2 a^2 H(t_ij) (z_ik - z_jk)^2 / r_k, H as at gpmi_lml_grad
 *   d_ell, d_sigma as gpmi_lml_grad (to rounding: another kernel adds them up)
 *   d_noise = .5 * (alpha^T alpha - trace(K_y^-1))                   (d LML / d noise_var)
 * Any output may be NULL.  sum_k r_k d_r[k] == l * d_ell (K depends on l * r_k only).  Refuses what gpmi_lml_grad
 * refuses.  One fused pass over K_y^-1 per 32 dimensions; the sums are bitwise reproducible from run to run. */
int gpmi_lml_grad_ard(gpmi_ctx* ctx, double* d_r, double* d_ell, double* d_sigma, double* d_noise);
/* The gradient of the log marginal likelihood of the CO2 composite kernel (kind 3, gpmi_set_kernel_params) w.r.t. its
 * 11 hyper-parameters and the noise variance at the resident factorisation (GPML section 5.4.3).  With
 * W = alpha alpha^T - K_y^-1, sq_ij the squared distance, r = sqrt(sq) and
 *   e1 = exp(-sq / (2 theta_2^2))                                    K = theta_1^2 e1 + theta_3^2 q2 + theta_6^2 p3
 *   q2 = exp(-sq / (2 theta_4^2) - 2 sin^2(pi r) / theta_5^2)            + theta_9^2 e4 + theta_11^2 delta_ij
 *   p3 = (1 + u)^-theta_8,  u = sq / (2 theta_8 theta_7^2)
 *   e4 = exp(-sq / (2 theta_10^2))
 * d_theta[m] = .5 * sum_ij W_ij dK_ij/dtheta_(m+1)  (11 doubles):
 *   dK/dtheta_1 = 2 theta_1 e1               dK/dtheta_2 = theta_1^2 e1 sq / theta_2^3
 *   dK/dtheta_3 = 2 theta_3 q2               dK/dtheta_4 = theta_3^2 q2 sq / theta_4^3
 *   dK/dtheta_5 = 4 theta_3^2 q2 sin^2(pi r) / theta_5^3
 *   dK/dtheta_6 = 2 theta_6 p3               dK/dtheta_7 = theta_6^2 p3 sq / (theta_7^3 (1 + u))
 *   dK/dtheta_8 = theta_6^2 p3 (u / (1 + u) - log(1 + u))
 *   dK/dtheta_9 = 2 theta_9 e4               dK/dtheta_10 = theta_9^2 e4 sq / theta_10^3
 *   dK/dtheta_11 = 2 theta_11 delta_ij
 * *d_noise = .5 * (alpha^T alpha - trace(K_y^-1)) = d_theta[10] / (2 theta_11).  Either output may be NULL.
 * GPMI_ERR_BAD_ARG when no regression factorisation is resident or the context's kernel is not kind 3.  Reads the
 * resident fit only: alpha, prediction, posterior samples and leave-one-out work afterwards as before (gpmi_append
 * refuses kind 3 before and after).  Costs what gpmi_lml_grad costs plus one fused pass over K_y^-1; the sums are bitwise
 * reproducible from run to run.  The derivatives assume 1 + u > 0 (theta_8 > 0). */
int gpmi_lml_grad_co2(gpmi_ctx* ctx, double* d_theta, double* d_noise);
/* Leave-one-out cross-validation at the resident regression factorisation (Rasmussen & Williams, GPML, section 5.4.2,
 * eqs. 5.10-5.12).  With K_y = K + noise_var I, alpha = K_y^-1 y and kappa_i = [K_y^-1]_ii:
 *   mu[i]   = y_i - alpha_i / kappa_i,  var[i] = 1 / kappa_i      (mean and variance of y_i predicted from the other
 *                                                                  N - 1 points, noise included)
 *   logp[i] = -.5 log var_i - (y_i - mu_i)^2 / (2 var_i) - .5 log(2 pi)
 *   *loo    = sum_i logp[i]                                       (added on the device in a fixed order)
 * mu, var, logp: N doubles each; every output may be NULL.  Needs a resident regression factor: refused without one, and
 * after a Laplace or softmax fit by the rule stated at gpmi_laplace_fit.  Every kernel kind (only L, m and y are read);
 * with lengthscales set the factor is that of the scaled inputs, as everywhere.  The factor, m and any resident test
 * state are left untouched.  Costs N^3/3 beyond the fit (U = L^-T; kappa_i = sum_j U_ij^2), half of gpmi_lml_grad. */
int gpmi_loo(gpmi_ctx* ctx, double* mu, double* var, double* logp, double* loo);
/* The derivatives of *loo (GPML eq. 5.13) w.r.t. l, sigma and noise_var at the resident factorisation:
 *   d/dtheta = sum_i (alpha_i r_i - .5 (1 + alpha_i^2 / kappa_i) s_i) / kappa_i,
 *   Z = K_y^-1 dK_y/dtheta,  r = Z alpha,  s_i = [Z K_y^-1]_ii
 * with dK_y/dl = K o sqdist / l^3 (Matern kinds: sigma^2 a^2 H(t) o sqdist / l), dK_y/dsigma = 2 K / sigma,
 * dK_y/dnoise_var = I.  Any output may be NULL.  Refuses what gpmi_lml_grad refuses; state rules as gpmi_loo.  With lengthscales set, sqdist is
 * that of the scaled inputs and d_ell the derivative w.r.t. the common multiplier l.  The l component takes the diagonal
 * of K_y^-1 (K o sqdist) K_y^-1, a full N x N x N product (2 N^3 flops beside the 2 N^3 / 3 of gpmi_lml_grad), formed
 * NB rows at a time; bitwise reproducible from run to run.  Device memory: DESIGN.md section 4c. */
int gpmi_loo_grad(gpmi_ctx* ctx, double* d_ell, double* d_sigma, double* d_noise);
/* The same two traces from the arguments gradient_ascent(a, b, sigma, l, alpha, K_y) receives
 * (tune_hyperparms_regression.py:31): a, b: N x d; alpha: N; K_y_inv: N x N row-major (host).
 * One fused N^2 pass instead of the reference's two N x N products (:55). */
int gpmi_grad_trace(gpmi_ctx* ctx, const double* a, const double* b, int64_t N, int64_t d, double sigma,
                    double ell, const double* alpha, const double* K_y_inv, double* d_ell, double* d_sigma);

/* compute_mar_likelihood for T hyper-parameter triples on one training set
 *                    tune_hyperparms_regression.py:292-313 called in the loops at :368-369,:385-386
 * triples: T x 3 = (ell, sigma_f, noise_var).  lml_out: T doubles (NaN where the
 * factorisation failed), status_out: T ints (GPMI_OK / GPMI_ERR_NOT_PD), may be
 * NULL.  Uses the training set of gpmi_set_train.  Up to "lanes" factorisations are in flight at once
 * (extra lanes = internal contexts with their own streams and workspaces; by size: 2 up to N = 32768,
 * else 1): the latency-bound panel steps of one fill with the MFMA work of another.
 * Each triple is factored by the same launches whatever the lane count, so the results are bitwise
 * independent of it; the factor left resident is that of the last triple. */
int gpmi_lml_batch(gpmi_ctx* ctx, const double* triples, int64_t T, double* lml_out,
                   int* status_out);

/* Binary GP classification by the Laplace approximation: Rasmussen & Williams, GPML, Algorithm 3.1 (Newton iteration
 * for the posterior mode, logistic likelihood) and 3.2 (prediction), with the labels +-1 of GP_binary_classification.py.
 * On the resident training set (gpmi_set_train; y exactly -1 or +1, else GPMI_ERR_BAD_ARG), squared-exponential kernel
 * only (a kind other than 0 -> GPMI_ERR_BAD_ARG), K = sigma^2 exp(-.5 / l^2 sqdist) without noise.  From a = f = 0 each
 * iteration forms f = K a, pi = expit(f), W = pi (1 - pi), grad = (y + 1) / 2 - pi, b = W f + grad and the objective
 * Psi = -a^T f / 2 + sum log p(y|f); it has converged when |Psi - Psi_prev| <= tol max(1, |Psi|), a drop of more than that
 * halves the step (a <- (a + a_prev) / 2, at most 20 times); otherwise B = I + W^1/2 K W^1/2 is factored and
 * a = b - W^1/2 B^-1 W^1/2 K b.  At most max_iter steps; *iters = steps taken, *converged = 0 / 1.
 *   log_q = Psi(f^) - sum log diag(chol B(f^))          (GPML eq. 3.32 at the mode f^)
 * f_hat: N doubles or NULL.  f^, grad(f^), W^1/2(f^) and the factor of B(f^) stay resident in place of any regression
 * factor: gpmi_predict*, gpmi_get_alpha, gpmi_post_* and gpmi_lml_grad then refuse (GPMI_ERR_BAD_ARG) until the next
 * regression factorisation, which in turn drops the Laplace state. */
int gpmi_laplace_fit(gpmi_ctx* ctx, double sigma, double ell, double tol, int max_iter, double* log_q, int* iters,
                     int* converged, double* f_hat);
/* Prediction on the resident test set (gpmi_set_test) from the resident Laplace fit (Algorithm 3.2):
 *   f_mean = K(X*, X) grad(f^),  f_var = sigma^2 - |B^-1/2 W^1/2 K(X, X*)|^2 per test point,
 *   prob = int expit(z) N(z | f_mean, f_var) dz     (composite trapezoid rule, error below 1e-12)
 * each n doubles or NULL. */
int gpmi_laplace_predict_resident(gpmi_ctx* ctx, double* f_mean, double* f_var, double* prob);
/* Gradient of log_q at the resident Laplace fit (GPML Algorithm 5.1, logistic likelihood) w.r.t. the relative
 * lengthscales of gpmi_set_lengthscales (d_r: d doubles, all r_k = 1 when none are set), the common lengthscale and
 * sigma, with the conventions of gpmi_lml_grad_ard; any pointer may be NULL (K has no noise term).  With pi = expit(f^),
 * W = pi (1 - pi), s = W^1/2, g = grad(f^), a = K^-1 f^ (the fit's last iterate; = g at the mode), B = L L^T:
 *   dlog_q/dtheta = sum_ik dK_ik/dtheta [ (a_i a_k - R_ik) / 2 + (z_i g_k + z_k g_i) / 2 ],   R = diag(s) B^-1 diag(s),
 *   z = s2 - R K s2,   s2_i = -(1 - [B^-1]_ii) (1 - 2 pi_i) / 2
 * (z^T dK g is the implicit term s2^T (I - K R) dK g of Algorithm 5.1).  The formula holds AT the mode: the result
 * carries the fit's distance from it, so fit with tol = 1e-13 (the default 1e-10 leaves up to a few 1e-9 relative).
 * U = L^-T, -B^-1 = -U U^T and [B^-1]_ii as in gpmi_lml_grad / gpmi_loo, K rebuilt into U's buffer, then one fused
 * pass over the lower tiles for all d + 2 derivatives.  Only reads the fit: it stays resident and
 * gpmi_laplace_predict_resident returns the same bits afterwards.  GPMI_ERR_BAD_ARG ("no Laplace fit resident") without
 * one.  The call runs no backward solve, so there is no give-up word to report.  Time: the GPMI_T_GRAD slot. */
int gpmi_laplace_grad(gpmi_ctx* ctx, double* d_r, double* d_ell, double* d_sigma);

/* Multi-class GP classification by the Laplace approximation: GPML Algorithm 3.3 (Newton iteration for the mode, softmax
 * likelihood, one latent function per class, all with the same squared-exponential prior K = sigma^2 exp(-.5 / l^2
 * sqdist), no noise) and 3.4 (prediction), the working form of GP_multi_classification.py.  The labels are the y of
 * gpmi_set_train: each an integer in [0, n_classes), else GPMI_ERR_BAD_ARG; 2 <= n_classes <= GPMI_SOFTMAX_MAX_CLASSES;
 * kernel kind 0 only.  With Y the 0/1 encoding and F, A, P of shape C x N (latent values, a = K^-1 f, softmax
 * probabilities), from A = 0 each iteration forms F = A K, P and
 *   Psi = -1/2 sum(A o F) + sum(Y o F) - sum_i logsumexp_c F_ci,
 * stops or halves the step by the rule of gpmi_laplace_fit, and otherwise factors L_c = chol(I + s_c s_c^T o K),
 * s_c = sqrt(P_c), forms E_c = S_c L_c^-T L_c^-1 S_c and M = chol(sum_c E_c), and steps to
 *   A <- B - [E_c K b_c]_c + [E_c M^-T M^-1 sum_c E_c K b_c]_c,   B = P o F - P o sum_c(P o F) + Y - P.
 *   log_q = Psi - sum_c sum log diag L_c - sum log diag M   at the last iterate
 * (the last term is missing from the printed Algorithm 3.3: 1/2 log|I + K W| = sum_c sum log diag L_c + sum log diag M).
 * f_hat: C x N doubles (row c = latent values of class c) or NULL.  Y - P, the E_c and M stay resident in place of any
 * regression factor or binary Laplace fit, under the rule stated at gpmi_laplace_fit.  Device memory: DESIGN.md. */
#define GPMI_SOFTMAX_MAX_CLASSES 10
int gpmi_softmax_fit(gpmi_ctx* ctx, int n_classes, double sigma, double ell, double tol, int max_iter, double* log_q,
                     int* iters, int* converged, double* f_hat);
/* Prediction on the resident test set (gpmi_set_test) from the resident softmax fit (Algorithm 3.4 with the shared
 * kernel), R = K(X*, X):
 *   mu (n x C) = R (Y - P)^T;  B_c = R E_c;  U_c = M^-1 B_c^T;
 *   cov (n x C x C, or NULL): cov[i][c][c'] = U_c[:, i] . U_c'[:, i], plus sigma^2 - B_c[i] . R[i] where c == c'
 *   prob (n x C): (1 / S) sum_s softmax(mu_i + chol(cov_i) z_s), with the S = n_samples rows of `normals` (S x C standard
 *   normals supplied by the caller, the same for every test point: the result is a function of its inputs).  A pivot
 *   <= 0 of the C x C Cholesky is set to 0 with its column.  n_samples 0: normals and prob NULL, no sampling. */
int gpmi_softmax_predict_resident(gpmi_ctx* ctx, double* mu, double* cov, int64_t n_samples, const double* normals,
                                  double* prob);
/* Gradient of log_q at the resident softmax fit w.r.t. the relative lengthscales of gpmi_set_lengthscales (d_r: d
 * doubles, all r_k = 1 when none are set), the common lengthscale and sigma of the kernel all classes share, with the
 * conventions of gpmi_laplace_grad; any pointer may be NULL (K has no noise term).  GPML prints no algorithm for the
 * multi-class case (Algorithm 5.1 is binary); DESIGN.md section 4g derives this one.  With G = Y - P at the mode:
 *   dlog_q/dtheta = 1/2 sum_ik dK_ik/dtheta Wm_ik
 *   Wm    = -sum_c E_c + Gamma + sum_c (g_c g_c^T + z_c g_c^T + g_c z_c^T)
 *   Gamma = sum_c E_c (M M^T)^-1 E_c = sum_c T_c^T T_c,   T_c^T = E_c M^-T
 * (-sum_c E_c + Gamma is minus the sum of the diagonal blocks of R = (K_blk + W^-1)^-1, GPML eq. 3.47: the classes share
 * one K, so only those blocks meet dK).  The implicit term: with Sigma_i the C x C posterior covariance of the latent
 * values at training point i -- the cov of gpmi_softmax_predict_resident with the training set as test set -- and pi_i
 * column i of P,
 *   q_i = diag(Sigma_i) - 2 Sigma_i pi_i,   s2_ci = -1/2 pi_ci (q_ci - pi_i . q_i)    (= -1/2 sum_pq Sigma_i[p,q] dW_i[p,q]/df_ci)
 *   z = s2 - R K_blk s2:   v_c = E_c (K s2_c),  t = M^-T M^-1 sum_c v_c,  z_c = s2_c - v_c + E_c t.
 * The formula holds AT the mode: fit with tol = 1e-13, as for gpmi_laplace_grad.  About 5 C N^3 flops (per class the
 * product K E_c, two triangular sweeps and a lower-tile product).  Only reads the fit (M, the E_c, F^, Y - P; the kept K
 * has its lower triangle mirrored into its upper one): it stays resident and gpmi_softmax_predict_resident returns the
 * same bits afterwards.  Device memory: C more N x N matrices; if they do not fit, GPMI_ERR_RUNTIME and the
 * fit is still resident.  GPMI_ERR_BAD_ARG ("no softmax fit resident (call gpmi_softmax_fit)") without one.  The
 * single-launch backward solve's give-up word is reported as by gpmi_softmax_fit.  Time: the GPMI_T_GRAD slot. */
int gpmi_softmax_grad(gpmi_ctx* ctx, double* d_r, double* d_ell, double* d_sigma);

/* Sparse GP regression with m inducing inputs Z (m x d, d as in gpmi_set_train) on the resident training set, for N far
 * beyond an N x N covariance: O(N m^2) flops, O(m^2 + N d) device memory.  GPML chapter 8; the
 * collapsed bound of Titsias (2009) -- method GPMI_SPARSE_VFE -- and FITC of Snelson & Ghahramani (2006).  Squared-
 * exponential kernel only (kind 0; sigma, ell as gpmi_factorize, the context's lengthscales apply to X, Z and the test
 * set alike), s = noise_var > 0, jitter >= 0 added to the diagonal of K_uu.  In the whitened form
 *   L = chol(K_uu + jitter I),  A = L^-1 K_uf (m x N),  q_i = |A[:, i]|^2,
 *   Lambda_i = s (VFE)  or  s + sigma^2 - q_i (FITC),  A~ = A Lambda^-1/2,  y~ = Lambda^-1/2 y,
 *   B = I + A~ A~^T,  L_B = chol(B),  c = L_B^-1 A~ y~,
 *   *value = -N/2 log 2 pi - sum log diag L_B - 1/2 sum_i log Lambda_i - 1/2 y~^T y~ + 1/2 c^T c
 *            [VFE only: - sum_i (sigma^2 - q_i) / (2 s)]
 * which for VFE is a lower bound of the log marginal likelihood gpmi_factorize returns and for FITC is
 * log N(y | 0, Q_ff + Lambda), Q_ff = K_fu K_uu^-1 K_uf.  K_uf is never held: the training rows pass in slabs (option
 * "sparse_slab") through the cross-covariance build, the sweep through L, one row pass and the accumulation of B; every
 * sum runs in a fixed order (bitwise reproducible from run to run at one slab size).
 *   GPMI_ERR_BAD_ARG: m < 1, m > N, noise_var <= 0, jitter < 0, an unknown method, a kernel kind other than 0.
 *   GPMI_ERR_NOT_PD:  a pivot of K_uu + jitter I (*bad_pivot = its 1-based index), a Lambda_i of FITC that is not a
 *                     positive finite number (*bad_pivot = the 1-based training row), a pivot of B (*bad_pivot = m + its
 *                     1-based index).
 * L, L_B, c, Z and the hyper-parameters stay resident.  A sparse fit is not a regression factor: it takes the place of a
 * resident regression factor, Laplace or softmax fit under the rule stated at gpmi_laplace_fit -- gpmi_predict*,
 * gpmi_get_alpha, gpmi_post_*, gpmi_lml_grad* and gpmi_loo* refuse (GPMI_ERR_BAD_ARG) until the next regression
 * factorisation; that, a Laplace or softmax fit, gpmi_set_train and gpmi_set_lengthscales drop it.  value / bad_pivot may
 * be NULL.  Timers: GPMI_T_SPARSE the whole span, of which GPMI_T_KS the cross-covariance builds, GPMI_T_SOLVE_V the
 * sweeps through L, GPMI_T_MEANVAR the row pass with g = A~ y~, GPMI_T_POSTCHOL the accumulation of A~ A~^T and
 * GPMI_T_CHOL the two factorisations. */
#define GPMI_SPARSE_VFE 0
#define GPMI_SPARSE_FITC 1
int gpmi_sparse_fit(gpmi_ctx* ctx, const double* Z, int64_t m, double sigma, double ell, double noise_var, double jitter,
                    int method, double* value, int64_t* bad_pivot);
/* Prediction on the resident test set (gpmi_set_test) from the resident sparse fit:
 *   v1 = L^-1 k_u*,  v2 = L_B^-1 v1,  mu = v2^T c,  var = sigma^2 - |v1|^2 + |v2|^2
 * -- the variance of the latent f, the convention of gpmi_predict_resident; out2 = sqrt(var) if want_sd (NaN where var is
 * negative) else var.  mu, out2: n doubles each, either may be NULL.  The test rows pass in chunks of the fit's slab size.
 * Refused (GPMI_ERR_BAD_ARG) without a sparse fit or a test set. */
int gpmi_sparse_predict_resident(gpmi_ctx* ctx, double* mu, double* out2, int want_sd);
/* c (m doubles) and q (N doubles) of the resident sparse fit; either may be NULL.  For tests and small N. */
int gpmi_sparse_get(gpmi_ctx* ctx, double* c_out, double* q_out);
/* Gradient of the VFE bound F that gpmi_sparse_fit returned, at the resident fit, w.r.t. ell, sigma, noise_var, the
 * context's lengthscales r (d doubles; without lengthscales the derivative at r = 1) and the inducing inputs Z as the
 * caller passed them (m x d, row-major, unscaled).  Every output may be NULL.  With s = noise_var, z = x / r, K0_uu = K_uu
 * without the jitter (a constant: the diagonal of K_uu contributes through sigma^2 only) and
 *   u = L_B^-T c,  p = L^-T u,  T = L^-T (I - B^-1) L^-1 / s,  beta = (y - K_fu p) / s,
 *   D_fu = K_fu T + beta p^T  (N x m, never held),  D_uu = -1/2 L^-T (B - 2 I + B^-1 + u u^T) L^-1,
 *   G_fu = D_fu o K_fu,  G_uu = D_uu o K0_uu:
 *   *d_sigma  = (2 / sigma) (sum G_fu + sum G_uu) - N sigma / s
 *   *d_ell    = (sum_ij G_fu,ij |z_i - z_j|^2 + sum_jj' G_uu,jj' |z_j - z_j'|^2) / ell^3
 *   d_r[k]    = (sum_ij G_fu,ij (z_ik - z_jk)^2 + sum_jj' G_uu,jj' (z_jk - z_j'k)^2) / (ell^2 r_k)
 *   *d_noise  = -(N - m + tr B^-1) / (2 s) + 1/2 beta^T beta + sum_i (sigma^2 - q_i) / (2 s^2)
 *   d_Z[j][k] = (sum_i G_fu,ij (z_ik - z_jk) + 2 sum_j' G_uu,jj' (z_j'k - z_jk)) / (ell^2 r_k)
 * so sum_k r_k d_r[k] = ell *d_ell.  Device schedule: L_B^-T and L^-T by the sweep on the identity, B^-1, B = L_B L_B^T, T
 * and D_uu by the routed GEMM (O(m^3)); then the training rows pass once more in slabs of the fit's size: K(X_slab, Z),
 * beta, E = W T on the routed GEMM (2 N m^2 flops) and one contraction kernel that reads every element of W and E once;
 * K_uu passes through the same kernel with E = D_uu.  Every sum runs in a fixed order without atomics: bitwise
 * reproducible from run to run at one slab size.  One host synchronisation.  O(N m^2), the order of the fit.
 *   GPMI_ERR_BAD_ARG: no sparse fit resident; the resident fit is FITC (its gradient is not implemented); d > 32 (the
 *                     contraction keeps a column's 2 d + 1 sums in registers; there is no pass loop over dimensions).
 * The resident fit is only read -- gpmi_sparse_predict_resident and gpmi_sparse_get return the same bits afterwards; the
 * slab workspace that prediction also overwrites is reused.  The m x m temporaries live in workspaces of the call's own,
 * 8 (max(S, m_p) ld + 3 m_p ld + chunks m_p (2 d + 1)) bytes with chunks = ceil(max(S, m_p) / 128), made at the first call
 * and freed when a regression factorisation, a Laplace or softmax fit or gpmi_set_train takes the sparse fit's place (a
 * sparse fit after a sparse fit keeps them: a tuner's step allocates nothing).  Timers: GPMI_T_SPARSE the whole span (it replaces the fit's), of which
 * GPMI_T_CHOL the m-sized part, GPMI_T_KS the covariance builds, GPMI_T_SOLVE_V beta, GPMI_T_POSTCHOL the products W T and
 * GPMI_T_MEANVAR the contractions. */
int gpmi_sparse_grad(gpmi_ctx* ctx, double* d_ell, double* d_sigma, double* d_noise, double* d_r, double* d_Z);

int gpmi_get_timers(gpmi_ctx* ctx, double* stage_ms, int count);
/* block the host until everything queued on the context has finished */
int gpmi_sync(gpmi_ctx* ctx);

/* ---- micro-benchmarks used by bench.py to re-read chip peaks on the box ---- */
/* fp64 MFMA issue rate: returns achieved TFLOP/s of a register-only
 * v_mfma_f64_16x16x4_f64 loop over the whole chip. */
int gpmi_probe_mfma_f64(gpmi_ctx* ctx, double* tflops);
/* same loop with one workgroup of 4 * blocks_per_cu waves on every CU (blocks_per_cu = waves per SIMD, 1 .. 4) and nacc
 * (4, 8, 16) independent accumulators per wave; out[0] = TFLOP/s, out[1] = shader clock in
 * GHz held during the loop, out[2] = shader cycles per MFMA per SIMD */
int gpmi_probe_mfma_f64_ex(gpmi_ctx* ctx, int blocks_per_cu, int nacc, int iters, double* out);
/* one launch shape of the trailing-update GEMM on scratch buffers; variant = timing-only
 * ablation bits (0 = the production kernel); out[0] = TFLOP/s, out[1] = ms per launch */
int gpmi_probe_gemm(gpmi_ctx* ctx, int64_t M, int64_t N, int64_t K, int lower, int variant, int reps,
                    double* out);
/* the Gram accumulation of gpmi_sparse_fit alone, B_lower (m x m) += V^T V for a random row-major slab V (S x m), split
 * launch and reduction together; out[0] = TFLOP/s on the 128 x 128 tiles it computes (2 S per element), out[1] = ms */
int gpmi_probe_gram(gpmi_ctx* ctx, int64_t S, int64_t m, int reps, double* out);
/* streaming-store bandwidth (GB/s) over `bytes` of device memory */
int gpmi_probe_hbm_write(gpmi_ctx* ctx, int64_t bytes, double* gbps);
/* streaming bandwidth with a chosen access form: mode 0 grid-stride 16-byte stores, 1 the same
 * non-temporal, 2 one contiguous span per workgroup, 3 span + non-temporal, 4 16-byte loads */
int gpmi_probe_hbm_ex(gpmi_ctx* ctx, int64_t bytes, int mode, int blocks, double* gbps);
/* what the device reports about itself: out[0] compute units, [1] shader clock kHz, [2] memory clock kHz,
 * [3] memory bus width (bits), [4] global memory bytes, [5] L2 bytes, [6] LDS per workgroup bytes, [7] wavefront size */
int gpmi_device_info(gpmi_ctx* ctx, double* out, int count);
/* the panel kernels alone on scratch data: kind 0 = Cholesky of one 128 x 128 block (potrf128), kind 1 = X L^-T on
 * m rows (trsm128); *out_us = microseconds per launch; stamps_out (64 entries or NULL) = in-kernel clock stamps
 * of one instrumented launch (layout: csrc/panel_mfma.hip) */
int gpmi_probe_panel(gpmi_ctx* ctx, int kind, int64_t m, int reps, double* out_us, uint64_t* stamps_out);
/* diagnostic: the give-up path of the one-launch backward solve.  An n x n identity system whose bottom block is
 * deliberately never solved: every wait runs into its bound (wait_ms here, 10 s in the product), the kernel must set
 * its error word (*err_out = 1), leave NaN in the entries it waited for (x_out, n doubles) and RETURN
 * (*elapsed_ms: about wait_ms per dependent block in flight). */
int gpmi_probe_trsv_giveup(gpmi_ctx* ctx, int64_t n, double wait_ms, int* err_out, double* elapsed_ms, double* x_out);

/* ---------------------------------------------------------------------------
 * Device-pointer block primitives for the multi-GPU (row-block cyclic) driver
 * in gaussian_process_amd/dist.py.  `stream` is a hipStream_t passed as void*
 * (torch.cuda.current_stream().cuda_stream).  All leading dimensions in
 * doubles.  Sizes must be multiples of 64 (panel width) / 128 (rows).
 * ------------------------------------------------------------------------- */
/* rows [row0,row0+nrows) of K(X,X)+s*I, columns [0, row0+nrows), into out
 * (nrows x ld); columns beyond N and rows beyond N are the identity padding. */
int gpmi_dev_rbf_rows(void* stream, const double* X_dev, int64_t N, int64_t d,
                      int64_t row0, int64_t nrows, int64_t ncols, double sigma, double ell,
                      double noise_var, double* out_dev, int64_t ld);
/* rows [row0,row0+nrows) of K(Xs,X): out[i][j] = k(Xs[row0+i], X[j]), j < ncols */
int gpmi_dev_rbf_cross(void* stream, const double* Xs_dev, int64_t n, const double* X_dev,
                       int64_t N, int64_t d, int64_t row0, int64_t nrows, int64_t ncols,
                       double sigma, double ell, double* out_dev, int64_t ld);
/* The same two builds for every covariance function the reference's prediction() serves (GP_regression.py:125-136:
 * 'rbf' / 'lin' / 'per') and for CO2_example.py:66-90's composite -- f4 on the row-block partitioned path.
 * kind / params as gpmi_set_kernel (0: sigma, l; 1: c; 2: period, l -- 1-D inputs) and gpmi_set_kernel_params (3: the
 * 11 hyper-parameters; kernel_4 adds theta_11^2 on the diagonal of a square matrix); kinds 4-6 (Matern) take (sigma, l)
 * as kind 0 does.  gpmi_dev_cov_cross takes a WINDOW
 * of the column inputs that starts at input col0 of the full set; square != 0: the full cross matrix is square (n == N),
 * so the composite kernel's delta term lands on row == col0 + column (CO2_example.py:58-62). */
int gpmi_dev_cov_rows(void* stream, int kind, const double* params, int nparams, const double* X_dev, int64_t N, int64_t d,
                      int64_t row0, int64_t nrows, int64_t ncols, double noise_var, double* out_dev, int64_t ld);
int gpmi_dev_cov_cross(void* stream, int kind, const double* params, int nparams, const double* Xs_dev, int64_t n,
                       const double* Xcols_dev, int64_t ncols_real, int64_t d, int64_t col0, int square, int64_t nrows,
                       int64_t ncols, double* out_dev, int64_t ld);
/* in-place Cholesky of the nb x nb diagonal block (nb multiple of 128, ld even, A_dev 16-byte aligned: a view that
 * starts on an odd column is refused before anything is launched).
 * Read: the 16 x 16 tiles on and below the block diagonal, the diagonal tiles whole (the symmetric values the K build
 * writes there).  The tiles strictly above the block diagonal are never read for the result and may hold anything, NaN
 * included; the updates inside a block wider than 128 may pass over those that lie inside a 128 x 128 diagonal block.
 * On return the lower triangle holds L, and the strict upper triangles of the 16 x 16 tiles on the diagonal are
 * OVERWRITTEN with W^T, W = the inverse of that tile of L (diag(W) = 1 / diag(L) implied), which gpmi_dev_trsm_block,
 * gpmi_dev_trsv_lt_fused and the vinv forms read back; a block of 128 columns leaves every other tile above the diagonal
 * as it was.  Under option "panel_fused" 0 (the first-generation 64-column leaves) nothing above the diagonal is the
 * factor's: such a factor carries NO inverses, and gpmi_dev_trsm_block takes it under the same option only.
 * info_dev: int64 on the device, atomically min-ed (as 64-bit unsigned) with col_offset + failing column, a pivot that
 * is negative, zero or NaN (initialise to INT64_MAX).  When several pivots fail, in one 16 x 16 tile or in different
 * launches of the call, it ends up holding the smallest failing global column; a value already below that stays.  Columns
 * left of the failing pivot's 16 x 16 tile are those of the clean factor; from that tile on the block is no factor. */
int gpmi_dev_potrf_block(void* stream, double* A_dev, int64_t ld, int64_t nb,
                         int64_t col_offset, int64_t* info_dev);
/* X (m x nb, ldx) <- X * L^-T with L the nb x nb lower factor (ldl) AS LEFT BY gpmi_dev_potrf_block / the
 * factorisation (m multiple of 128, nb of 64, ldl and ldx even, both pointers 16-byte aligned).  nb multiple of 128:
 * the 16 x 16 diagonal tiles carry their inverses above the diagonal, so a copy of the block must be a copy of the
 * whole nb x nb square.  Read of L: the tiles below the block diagonal and the diagonal tiles whole, nothing above
 * them.  nb an odd multiple of 64, or option "panel_fused" 0 (required for a factor made under it): the 64-column
 * substitution leaves, which read the lower triangle only.  L is not written.  One launch or two per 128 columns
 * (gpmi_dev_set_concurrent) give the same bits, and so do the wave-per-row and lane-per-row forms of the 64-column
 * leaves (option "trsm_wave"). */
int gpmi_dev_trsm_block(void* stream, const double* L_dev, int64_t ldl, double* X_dev,
                        int64_t ldx, int64_t m, int64_t nb);
/* X (rows x ncols, ldx) <- X * L^-T for 1 <= rows <= 16 and L the ncols x ncols lower factor (ldl) of a FUSED
 * factorisation (ncols a multiple of 128, ldl and ldx even and >= ncols, both pointers 16-byte aligned): the forward
 * sweep of gpmi_append for a few new points.  trsm128's recurrence on 16 x 16 tiles with the stored inverses; one launch
 * per 128 columns, L streamed once, a fixed summation order (the same bits every run).  Measured it is bound by its
 * chain of ncols / 128 dependent launches, not by memory: 0.35 of the streaming-read rate at ncols = 65536, 0.03 at 4096
 * (profiles/r14_append_rate.txt).  Read of L: the
 * tiles below the block diagonal, and of every 128 x 128 diagonal block its lower 16 x 16 tiles and its diagonal tiles
 * whole -- never the block-upper tiles, which hold L_kk^-T after a backward solve.  Rows of X from `rows` on and columns
 * from ncols on are neither read nor written; L is not written.  Anything else is refused with nothing launched. */
int gpmi_dev_border_sweep(void* stream, const double* L_dev, int64_t ldl, int64_t ncols, double* X_dev, int64_t ldx,
                          int64_t rows);
/* X (rows x ncols, ldx) <- X * L^-1 for rows >= 1 and L the ncols x ncols lower factor (ldl) of a FUSED factorisation: row
 * i becomes L^-T x_i, the backward counterpart of gpmi_dev_border_sweep with the same argument rules (ncols a multiple of
 * 128, ldl and ldx even and >= ncols, both pointers 16-byte aligned; ncols == 0 does nothing).  One launch per 128-column
 * block from the last to the first whatever `rows` is: rows beyond 16 are further 16-row groups in the same launches
 * (a second grid dimension), dead rows of the last group are fed as zeros and never stored.  In launch t the workgroup of
 * column block c <= t applies X_c -= X_(t+1) L_(t+1, c); the one with c == t then solves X_t <- X_t L_tt^-1 by the
 * backward recurrence over its eight 16 x 16 tiles with the stored tile inverses.  No workgroup waits for another, nothing
 * is added atomically, the sums run in a fixed order: the same bits every run.  L is streamed once per 16-row group.  Reads
 * of L: exactly those of gpmi_dev_border_sweep -- never the block-upper tiles.  Rows of X from `rows` on and columns from
 * ncols on are neither read nor written; L is not written.  Anything else is refused with nothing launched.  Measured
 * (profiles/r17_predgrad_rate.txt): with one row group the chain of launches bounds it, 15.7 us per launch at 4096 columns
 * and 20.4 us at 65536, where it reads L at 0.26 of the streaming-read rate; with 256 row groups a launch takes 134 us to
 * 1.8 ms and the groups read L, mostly out of L2, at 0.66 to 0.75 of that rate. */
int gpmi_dev_back_sweep(void* stream, const double* L_dev, int64_t ldl, int64_t ncols, double* X_dev, int64_t ldx,
                        int64_t rows);
/* C (M x N, ldc) -= A (M x K, lda) * B (N x K, ldb)^T.  lower != 0: only tiles
 * that intersect {col <= row + diag_off} are touched. */
int gpmi_dev_gemm_nt(void* stream, double* C_dev, int64_t ldc, const double* A_dev, int64_t lda,
                     const double* B_dev, int64_t ldb, int64_t M, int64_t N, int64_t K,
                     int lower, int64_t diag_off);
/* same, for a rank's STACKED row blocks (row-block cyclic storage): the 128-row tile
 * bands of row block q (row_block_rows rows each) update only the leading
 * row_ncols_dev[q] columns of C (int32 on the device) */
int gpmi_dev_gemm_nt_rowmap(void* stream, double* C_dev, int64_t ldc, const double* A_dev, int64_t lda,
                            const double* B_dev, int64_t ldb, int64_t M, int64_t N, int64_t K,
                            const int32_t* row_ncols_dev, int64_t row_block_rows);
/* the same with a host copy of the row map (row_bands entries covering M): only the supertiles that hold
 * live tiles are launched */
int gpmi_dev_gemm_nt_rowmap_host(void* stream, double* C_dev, int64_t ldc, const double* A_dev, int64_t lda,
                                 const double* B_dev, int64_t ldb, int64_t M, int64_t N, int64_t K,
                                 const int32_t* row_ncols_dev, const int32_t* row_ncols_host, int64_t row_bands,
                                 int64_t row_block_rows);
/* C (M x N) -= A (M x K) * B^T with B given as a TABLE of row blocks: block i (b_block_rows x K, leading dimension
 * ldb) starts at B_dev + b_block_off_dev[i] doubles (device array, ceil(N / b_block_rows) entries).  The
 * multi-rank driver reads the panel column this way straight from the all-gather's receive buffer (one
 * contiguous chunk per rank) in natural block order -- no re-ordering copy.  The row map is optional
 * (row_ncols_dev and row_ncols_host both NULL: plain rectangle). */
int gpmi_dev_gemm_nt_blocks(void* stream, double* C_dev, int64_t ldc, const double* A_dev, int64_t lda,
                            const double* B_dev, int64_t ldb, const int64_t* b_block_off_dev, int64_t b_block_rows,
                            int64_t M, int64_t N, int64_t K, const int32_t* row_ncols_dev,
                            const int32_t* row_ncols_host, int64_t row_bands, int64_t row_block_rows);
/* out2[0] = sum_{i<n} log(A[i][i]) (skipped if A_dev is NULL), out2[1] = sum_{i<nx} x[i]^2
 * (skipped if x_dev is NULL): the per-rank pieces of the log-marginal-likelihood */
int gpmi_dev_logdiag_sumsq(void* stream, const double* A_dev, int64_t ld, int64_t n, const double* x_dev,
                           int64_t nx, double* out2_dev);
/* y[c] = sum_r A[r][c] * x[r] for a row-major nrows x ncols block (fixed summation order);
 * scratch: ceil(nrows/64) * ncols doubles (ncols % 2 == 0 and ld % 2 == 0 take the 16-byte-load path, which uses
 * ceil(nrows/128) * ncols of them).  Piece of the distributed backward solve
 * (GP_regression.py:140): a rank's contribution L_jk^T alpha_j of its rows below block k. */
int gpmi_dev_gemv_t(void* stream, const double* A_dev, int64_t ld, int64_t nrows, int64_t ncols,
                    const double* x_dev, double* y_dev, double* scratch_dev);
/* backward substitution L^T x = b on an n x n lower block (x overwrites b), n % 64 == 0 */
int gpmi_dev_trsv_lt(void* stream, const double* L_dev, int64_t ld, double* b_dev, int64_t n);
/* the same for a block as gpmi_dev_potrf_block leaves it (inverses in its diagonal tiles), n % 128 == 0: 128 unknowns
 * per launch; b_dev is destroyed, the solution goes to x_dev (n doubles, must not alias b_dev) */
int gpmi_dev_trsv_lt_fused(void* stream, const double* L_dev, int64_t ld, double* b_dev, double* x_dev, int64_t n);
/* the same through the inverted 128 x 128 diagonal blocks: invert != 0 first writes L_kk^-T of every 128 x 128 diagonal
 * block into that block's upper triangle (storage nothing else reads; one launch), then -- and on every later call with
 * invert == 0 on the same factored block -- each step is one matrix-vector product with it.  a5 of the multi-rank driver
 * (GP_regression.py:140). */
int gpmi_dev_trsv_lt_vinv(void* stream, double* L_dev, int64_t ld, double* b_dev, double* x_dev, int64_t n, int invert);
/* the same in ONE launch: the 128-column blocks are chained through the solution vector itself (x_dev is filled with a
 * "not yet" NaN pattern, a block's consumers poll the entries they need), so no launch gap and no chip-wide update sits
 * between two blocks.  vside_dev: n * 128 doubles owned by the caller; invert != 0 first fills it with the inverses of the
 * 128 x 128 diagonal blocks (row-major, one launch; also written into the blocks' upper triangles as above), later calls
 * on the same factored block pass 0 and the same buffer.  m_dev is only read; x_dev must not alias it.  err_dev: one int
 * the kernel sets to 1 if a wait gave up (non-finite factor); zero it before the call.  L_dev and vside_dev must be
 * 16-byte aligned (the kernel reads both with 16-byte loads; an odd column offset of a view is refused).  The chain
 * advances only while the queue makes progress: workgroup b waits for workgroups < b, which the hardware dispatches
 * first; a wait is bounded by wall time (10 s), so a co-tenant that holds the card for a while reads as a slow solve,
 * never as a wrong one.  a5 (GP_regression.py:140). */
int gpmi_dev_trsv_lt_chain(void* stream, double* L_dev, int64_t ld, double* vside_dev, const double* m_dev, double* x_dev,
                           int64_t n, int invert, int* err_dev);
/* on != 0: the block primitives called from this thread run beside a trailing update on another stream (lookahead)
 * and use their small-LDS forms, which fit on a CU next to an update workgroup; same results.  2: the same, and no
 * panel chain waits for this thread's update launches either (the state of a Cholesky of 49152 columns and more: the
 * 256 x 128 form from "tall_min_tiles_slack" live tiles on); same results.  0 switches back. */
int gpmi_dev_set_concurrent(int on);
/* kernel-selection options (the gpmi_set_option names that choose between kernel forms: "gemm_ticket", "gemm_persist",
 * "gemm_tall", ...) for the context-free block primitives called from THIS thread; same results
 * whatever the choice.  The multi-rank driver switches its large update launches to the ticket form with it. */
int gpmi_dev_set_option(const char* name, int64_t value);
/* f2 on device pointers, one row chunk of the gradient trace (tune_hyperparms_regression.py:43-57):
 *   out2[0] += sum_ij W_ij dK_ij/dl,  out2[1] += sum_ij W_ij dK_ij/dsigma,
 *   W_ij = alpha_r[i] alpha_c[j] - kinv_sign * Kinv[(i - row0) * ld + j],  rows row0 .. row0 + nrows, all N columns.
 * partial_dev: 2 * ceil(nrows / 128) * ceil(N / 128) doubles of workspace.  The multi-rank driver feeds it
 * its own partial of -K_y^-1 row block by row block (DistGP.lml_grad). */
int gpmi_dev_grad_trace(void* stream, const double* X_dev, int64_t N, int64_t d, int64_t row0, int64_t nrows,
                        const double* alpha_r_dev, const double* alpha_c_dev, const double* Kinv_dev, int64_t ld,
                        double kinv_sign, double sigma, double ell, double* partial_dev, double* out2_dev);
/* out[i] = sum_j V[i][j]*m[j] ; out2[i] = sum_j V[i][j]^2  (partial sums over
 * the columns this rank owns), i < nrows, j < ncols */
int gpmi_dev_row_dots(void* stream, const double* V_dev, int64_t ld, int64_t nrows,
                      int64_t ncols, const double* m_dev, double* dot_out_dev,
                      double* sq_out_dev);

/* out[i] = (base_dev ? base_dev[i] : 0) + scale * (in[i] + in[stride + i] + ... + in[(count - 1) * stride + i]),
 * i < n, the contributions added one after the other in index order (no reduction tree): the partitioned path's sums
 * over gathered per-rank partials -- the right-hand side m_k - sum_r part_r of the distributed backward solve
 * (GP_regression.py:140), the log-determinant pieces (tune_hyperparms_regression.py:312) -- come out with the same
 * bits on every rank.  out_dev may alias base_dev. */
int gpmi_dev_sum_fixed(void* stream, const double* in_dev, int64_t count, int64_t stride, int64_t n,
                       const double* base_dev, double scale, double* out_dev);
/* Y (rows x cols, ldy) += a * X (rows x cols, ldx): K_ss + jitter * I - v^T v on the partitioned path
 * (GP_regression.py:154), the all-reduced -v^T v added onto the covariance rows */
int gpmi_dev_axpy2d(void* stream, double* Y_dev, int64_t ldy, const double* X_dev, int64_t ldx, int64_t rows,
                    int64_t cols, double a);

/* ---------------------------------------------------------------------------
 * RCCL behind the C-ABI: the collectives of the row-block partitioned path (broadcast of a
 * factored diagonal block, all-gather of a panel column over xGMI, the small all-reduces) issued on the CALLER'S stream,
 * straight into librccl -- opened at run time (dlopen), never linked, so the library loads on hosts without it and binds
 * the copy of RCCL a process already carries (PyTorch ships one next to its HIP runtime).  One communicator must not be
 * used from two streams at once; the multi-rank driver keeps one per stream (gaussian_process_amd/dist.py: RcclComm).
 * All sizes in bytes except gpmi_comm_all_reduce.
 * ------------------------------------------------------------------------- */
typedef struct gpmi_comm gpmi_comm;
/* optional: the librccl to bind (absolute path); without it the first call looks for a copy already in the process,
 * then for librccl.so.1 on the loader's path ($GPMI_RCCL_LIB overrides) */
int gpmi_comm_load(const char* librccl_path);
/* which library was bound (out: cap bytes) and its ncclGetVersion (may be NULL) */
int gpmi_comm_library(char* out, int64_t cap, int* version);
/* rank 0: a fresh ncclUniqueId (128 bytes) to hand to every rank by any side channel */
int gpmi_comm_unique_id(char* id128);
/* collective over the `size` ranks that hold the same id: ncclCommInitRank on `device` */
int gpmi_comm_create(const char* id128, int rank, int size, int device, gpmi_comm** out);
int gpmi_comm_destroy(gpmi_comm* comm);
/* every rank's buf_dev (nbytes) <- root's */
int gpmi_comm_broadcast(gpmi_comm* comm, void* stream, void* buf_dev, int64_t nbytes, int root);
/* recv_dev (size * nbytes_per_rank) <- every rank's send_dev (nbytes_per_rank), in rank order */
int gpmi_comm_all_gather(gpmi_comm* comm, void* stream, const void* send_dev, void* recv_dev, int64_t nbytes_per_rank);
/* in place over `count` elements; dtype 0 float64, 1 int64; op 0 sum, 1 min, 2 max */
int gpmi_comm_all_reduce(gpmi_comm* comm, void* stream, void* buf_dev, int64_t count, int dtype, int op);

#ifdef __cplusplus
}
#endif
#endif /* GPMI_H */
