// C-ABI of libgpmi355x.so (see include/gpmi.h): context lifetime, options, uploads, the covariance calls, the getters,
// the batch of LML evaluations, and the shims in front of the models' *_impl functions (driver.hip, regress.hip, predgrad.hip,
// laplace.hip, softmax.hip, sparse.hip) that keep the reference's call surface (GP_regression.py:109-156,
// tune_hyperparms_regression.py:292-313) reachable through plain C.
//
// Data layout in HBM (one context):
//   A   (Np + 128) x ldA   row-major, ldA = Np + ld_pad.  Rows/cols < N hold
//       K + s*I (lower tiles only) and, after gpmi_factorize, L.  Np = N rounded
//       up to 128; the padding is the identity, so every block operation works
//       on whole tiles.  Row Np carries y: the factorisation treats it as one
//       more row of the panel, so when it finishes that row holds
//       m = L^-1 y (forward substitution folded into the sweep, no extra pass).
//       Option "reserve" r sizes both dimensions for N + r points instead; gpmi_append then
//       grows the factor in place and moves the y row to the new Np (append.hip).
//   V   n_p x ldV          row-major, row i = K(x*_i, X) then (L^-1 K_s)[:, i]
//       (v transposed: both GEMM operands of the sweep stay K-contiguous).
//   P   n_p x ldP          posterior covariance / its factor (gpmi_post_chol).
#include "gpmi_ctx.h"

using namespace gpmi;

namespace gpmi {
thread_local std::string g_err;

// options of the context-free gpmi_dev_* primitives called from this thread (gpmi_dev_set_option); the defaults otherwise
static thread_local Tuning t_dev_tuning;
static thread_local const Tuning* t_tuning = nullptr;
const Tuning& tuning() { return t_tuning ? *t_tuning : t_dev_tuning; }
TuneScope::TuneScope(const Tuning* t) : prev(t_tuning) { t_tuning = t; }
TuneScope::~TuneScope() { t_tuning = prev; }
static thread_local Sharing t_sharing;
Sharing& sharing() { return t_sharing; }

// z = x / r for the training / test inputs of a context with per-dimension lengthscales (the raw inputs stay resident:
// a tuner that changes r every iteration uploads d doubles, not N d)
int ard_rescale_train(gpmi_ctx* c) {
    if (!c->ard()) return GPMI_OK;
    HIP_TRY(c->Xz.ensure((size_t)c->N * c->d * 8));
    HIP_TRY(launch_scale_inputs(c->stream, c->X.as<double>(), c->ard_rdev.as<double>(), c->N, c->d, c->Xz.as<double>()));
    HIP_TRY(hipStreamSynchronize(c->stream));
    box_scale(c->boxX, c->ard_r, c->boxZ);
    return GPMI_OK;
}
int ard_rescale_test(gpmi_ctx* c) {
    if (!c->ard()) return GPMI_OK;
    HIP_TRY(c->Xsz.ensure((size_t)c->n * c->d * 8));
    HIP_TRY(launch_scale_inputs(c->stream, c->Xs.as<double>(), c->ard_rdev.as<double>(), c->n, c->d, c->Xsz.as<double>()));
    HIP_TRY(hipStreamSynchronize(c->stream));
    box_scale(c->boxXs, c->ard_r, c->boxZs);
    return GPMI_OK;
}
}

extern "C" {

int gpmi_abi_version(void) { return GPMI_ABI_VERSION; }
const char* gpmi_last_error(void) { return g_err.c_str(); }

int gpmi_device_count(int* count) {
    if (!count) return fail_arg("gpmi_device_count: null pointer");
    int n = 0;
    hipError_t e = hipGetDeviceCount(&n);
    if (e != hipSuccess) { *count = 0; return fail_runtime(e, "hipGetDeviceCount"); }
    *count = n;
    return GPMI_OK;
}

int gpmi_ctx_create(int device, gpmi_ctx** out) {
    if (!out) return fail_arg("gpmi_ctx_create: null out pointer");
    *out = nullptr;
    int n = 0;
    HIP_TRY(hipGetDeviceCount(&n));
    if (device < 0 || device >= n) return fail_arg("gpmi_ctx_create: no such device");
    HIP_TRY(hipSetDevice(device));
    gpmi_ctx* c = new gpmi_ctx();
    c->device = device;
    int prio_lo = 0, prio_hi = 0;
    (void)hipDeviceGetStreamPriorityRange(&prio_lo, &prio_hi);
    hipError_t e = hipStreamCreateWithPriority(&c->stream, hipStreamNonBlocking, prio_lo);
    if (e != hipSuccess) { delete c; return fail_runtime(e, "hipStreamCreate"); }
    e = hipStreamCreateWithPriority(&c->pstream, hipStreamNonBlocking, prio_hi);
    if (e != hipSuccess) { (void)hipStreamDestroy(c->stream); delete c; return fail_runtime(e, "hipStreamCreate"); }
    const char* env;
    if ((env = getenv("GPMI_NB"))) c->nb = std::max<int64_t>(128, atoll(env) / 128 * 128);
    if ((env = getenv("GPMI_LD_PAD"))) c->ld_pad = std::max<int64_t>(0, atoll(env) / 2 * 2);
    if ((env = getenv("GPMI_LOOKAHEAD"))) c->lookahead = atoi(env) ? 1 : 0;
    *out = c;
    return GPMI_OK;
}

int gpmi_ctx_destroy(gpmi_ctx* c) {
    if (!c) return GPMI_OK;
    for (gpmi_ctx* l : c->lane_ctx) (void)gpmi_ctx_destroy(l);
    c->lane_ctx.clear();
    (void)hipSetDevice(c->device);
    (void)hipStreamSynchronize(c->stream);
    for (DevBuf* b : {&c->X, &c->y, &c->A, &c->info, &c->red, &c->Xs, &c->V, &c->P, &c->vec, &c->dense,
                       &c->U, &c->Kn, &c->gpart, &c->cov_a, &c->cov_b, &c->cov_out, &c->flag, &c->vside,
                       &c->Xz, &c->Xsz, &c->ard_rdev, &c->gsum, &c->app, &c->spareA, &c->rem, &c->lap, &c->lap_part, &c->lap_out, &c->sm, &c->sm_part, &c->sm_E, &c->sm_B, &c->sm_out, &c->loov, &c->loow, &c->pgW, &c->pgpart, &c->pgsum,
                       &c->sp_Zraw, &c->sp_Z, &c->sp_L, &c->sp_B, &c->sp_W, &c->sp_q, &c->sp_vec, &c->sp_part, &c->sp_scr, &c->sp_info, &c->sp_pred,
                       &c->sp_g0, &c->sp_g1, &c->sp_g2, &c->sp_gE, &c->sp_gpart, &c->sp_gvec})
        b->release();
    for (auto e : c->ev_pool) (void)hipEventDestroy(e);
    (void)hipStreamDestroy(c->stream);
    (void)hipStreamDestroy(c->pstream);
    delete c;
    return GPMI_OK;
}

// kernel-selection options (gpmi_internal.h: Tuning) by name; -1: no such option, else a status
static int set_tuning_option(Tuning& t, const char* name, int64_t value) {
    if (!strcmp(name, "gemm_small_tiles")) {
        t.gemm_small_tiles = value ? 1 : 0;
    } else if (!strcmp(name, "trsm_wave")) {
        t.trsm_wave = value ? 1 : 0;
    } else if (!strcmp(name, "gemm_small_dma")) {
        t.gemm_small_dma = value ? 1 : 0;
    } else if (!strcmp(name, "gemm_persist")) {
        t.gemm_persist = value ? 1 : 0;
    } else if (!strcmp(name, "gemm_ticket")) {
        if (value < 0 || value > 2) return fail_arg("gemm_ticket must be 0 (off), 1 (trailing updates under lookahead) or 2 (every launch)");
        t.gemm_ticket = (int)value;
    } else if (!strcmp(name, "gemm_balance")) {
        t.gemm_balance = value ? 1 : 0;
    } else if (!strcmp(name, "trsv_vinv")) {
        if (value < 0 || value > 2) return fail_arg("trsv_vinv must be 0 (16 x 16 rounds), 1 (one launch per block) or 2 (one launch)");
        t.trsv_vinv = (int)value;
    } else if (!strcmp(name, "panel_fused")) {
        t.panel_fused = value ? 1 : 0;
    } else if (!strcmp(name, "rbf_blocks")) {
        if (value < 1 || value > (1 << 24)) return fail_arg("rbf_blocks must be in 1..2^24");
        t.rbf_blocks = (int)value;
    } else if (!strcmp(name, "gemm_dma_waves")) {
        if (value != 4 && value != 8) return fail_arg("gemm_dma_waves must be 4 or 8");
        t.gemm_dma_waves = (int)value;
    } else if (!strcmp(name, "gemm_tall")) {
        if (value < 0 || value > 1) return fail_arg("gemm_tall must be 0 (128 x 128 blocks) or 1 (256 x 128 blocks for large launches)");
        t.gemm_tall = (int)value;
    } else if (!strcmp(name, "tall_min_tiles")) {
        if (value < 0 || value > (1 << 30)) return fail_arg("tall_min_tiles must be in 0..2^30");
        t.tall_min_tiles = (int)value;
    } else if (!strcmp(name, "tall_min_tiles_slack")) {
        if (value < 0 || value > (1 << 30)) return fail_arg("tall_min_tiles_slack must be in 0..2^30");
        t.tall_min_tiles_slack = (int)value;
    } else if (!strcmp(name, "gemm_dma")) {
        t.gemm_use_dma = value ? 1 : 0;
    } else {
        return -1;
    }
    return GPMI_OK;
}

int gpmi_set_option(gpmi_ctx* c, const char* name, int64_t value) {
    if (!c || !name) return fail_arg("gpmi_set_option: null argument");
    if (!strcmp(name, "nb")) {
        if (value != 0 && (value < 128 || value % 128)) return fail_arg("nb must be 0 (auto) or a positive multiple of 128");
        c->nb = value;
    } else if (!strcmp(name, "ld_pad")) {
        if (value < 0 || value % 2) return fail_arg("ld_pad must be even and >= 0");
        c->ld_pad = value;
        c->res.drop_fit();
    } else if (!strcmp(name, "timing")) {
        c->timing = value ? 1 : 0;
    } else if (!strcmp(name, "lookahead")) {
        c->lookahead = value ? 1 : 0;
    } else if (!strcmp(name, "la_min")) {
        if (value < 0) return fail_arg("la_min must be >= 0");
        c->la_min = value;
    } else if (!strcmp(name, "shallow_min")) {
        if (value < 0) return fail_arg("shallow_min must be >= 0");
        c->shallow_min = value;
    } else if (!strcmp(name, "sparse_slab")) {
        if (value < 0) return fail_arg("sparse_slab must be >= 0 (0: by size)");
        c->sparse_slab = value;
    } else if (!strcmp(name, "reserve")) {
        // takes effect with the next fit; a resident one keeps the layout it was made with
        if (value < 0) return fail_arg("reserve must be >= 0 (points that gpmi_append may add in place)");
        c->reserve = value;
    } else if (!strcmp(name, "append_skinny")) {
        if (value < -1 || value > 1) return fail_arg("append_skinny must be -1 (by size), 0 (never) or 1 (whenever allowed)");
        c->append_skinny = (int)value;
    } else if (!strcmp(name, "pgrad_sweep")) {
        if (value < -1 || value > 1) return fail_arg("pgrad_sweep must be -1 (by size), 0 (the inverse route) or 1 (the sweep route whenever allowed)");
        c->pgrad_sweep = (int)value;
    } else if (!strcmp(name, "pgrad_sweep_max")) {
        if (value < 0) return fail_arg("pgrad_sweep_max must be >= 0");
        c->pgrad_sweep_max = value;
    } else if (!strcmp(name, "remove_keep_spare")) {
        // 0 frees the buffer a removal leaves behind (and one kept earlier); 1 keeps it for the next removal
        c->remove_keep_spare = value ? 1 : 0;
        if (!c->remove_keep_spare) {
            HIP_TRY(hipSetDevice(c->device));
            c->spareA.release();
        }
    } else if (!strcmp(name, "lanes")) {
        if (value < 0 || value > 8) return fail_arg("lanes must be 0 (by size) .. 8");
        c->lanes = (int)value;
    } else {
        const int rc = set_tuning_option(c->tune, name, value);
        if (rc < 0) return fail_arg("gpmi_set_option: unknown option");
        return rc;
    }
    return GPMI_OK;
}

// The same kernel-selection options for the context-free gpmi_dev_* block primitives called from THIS thread (the
// multi-rank driver): e.g. "gemm_ticket" 2 around its large update launches.  Thread-local; the defaults otherwise.
int gpmi_dev_set_option(const char* name, int64_t value) {
    if (!name) return fail_arg("gpmi_dev_set_option: null argument");
    const int rc = set_tuning_option(t_dev_tuning, name, value);
    if (rc < 0) return fail_arg("gpmi_dev_set_option: unknown option");
    return rc;
}

int gpmi_set_kernel(gpmi_ctx* c, int kind, double p0, double p1) {
    if (!c) return fail_arg("gpmi_set_kernel: null context");
    if (kind < 0 || kind == 3 || kind > 6)
        return fail_arg("gpmi_set_kernel: kind must be 0 (rbf), 1 (linear), 2 (periodic) or 4, 5, 6 (Matern nu = 1/2, 3/2, 5/2)");
    if (kind == 2 && (!(p0 != 0.0) || !(p1 != 0.0))) return fail_arg("gpmi_set_kernel: period and lengthscale must be non-zero");
    c->kind = kind; c->kp0 = p0; c->kp1 = p1;
    c->res.drop_fit();
    return GPMI_OK;
}

int gpmi_set_kernel_params(gpmi_ctx* c, int kind, const double* params, int nparams) {
    if (!c || !params) return fail_arg("gpmi_set_kernel_params: null argument");
    if (kind != 3) {
        if (kind < 0 || kind > 6 || nparams != 2) return fail_arg("gpmi_set_kernel_params: kinds 0-2 and 4-6 take 2 parameters");
        return gpmi_set_kernel(c, kind, params[0], params[1]);
    }
    if (nparams != 11) return fail_arg("gpmi_set_kernel_params: the CO2 composite kernel takes 11 hyper-parameters (CO2_example.py:86-89)");
    if (!(params[1] != 0.0) || !(params[3] != 0.0) || !(params[4] != 0.0) || !(params[6] != 0.0) || !(params[7] != 0.0) ||
        !(params[9] != 0.0))
        return fail_arg("gpmi_set_kernel_params: theta_2, 4, 5, 7, 8, 10 divide and must be non-zero");
    c->kind = 3;
    for (int i = 0; i < 11; ++i) c->kpv[i] = params[i];
    c->res.drop_fit();
    return GPMI_OK;
}

int gpmi_sync(gpmi_ctx* c) {
    if (!c) return fail_arg("gpmi_sync: null context");
    HIP_TRY(hipSetDevice(c->device));
    HIP_TRY(hipStreamSynchronize(c->stream));
    return GPMI_OK;
}

static int cov_impl(gpmi_ctx* c, int kind, const double* a, int64_t N, const double* b, int64_t M, int64_t d,
                    double p0, double p1, const double* kpv, double* out);

int gpmi_cov(gpmi_ctx* c, int kind, const double* a, int64_t N, const double* b, int64_t M, int64_t d,
             double p0, double p1, double* out) {
    if (kind < 0 || kind == 3 || kind > 6) return fail_arg("gpmi_cov: kind must be 0, 1, 2, 4, 5 or 6");
    return cov_impl(c, kind, a, N, b, M, d, p0, p1, nullptr, out);
}

int gpmi_cov_params(gpmi_ctx* c, int kind, const double* a, int64_t N, const double* b, int64_t M, int64_t d,
                    const double* params, int nparams, double* out) {
    if (!params) return fail_arg("gpmi_cov_params: null parameters");
    if (kind != 3) {
        if (kind < 0 || kind > 6 || nparams != 2) return fail_arg("gpmi_cov_params: kinds 0-2 and 4-6 take 2 parameters");
        return cov_impl(c, kind, a, N, b, M, d, params[0], params[1], nullptr, out);
    }
    if (nparams != 11) return fail_arg("gpmi_cov_params: the CO2 composite kernel takes 11 hyper-parameters");
    if (!(params[1] != 0.0) || !(params[3] != 0.0) || !(params[4] != 0.0) || !(params[6] != 0.0) || !(params[7] != 0.0) ||
        !(params[9] != 0.0))
        return fail_arg("gpmi_cov_params: theta_2, 4, 5, 7, 8, 10 divide and must be non-zero");
    return cov_impl(c, 3, a, N, b, M, d, 0., 0., params, out);
}

int gpmi_rbf(gpmi_ctx* c, const double* a, int64_t N, const double* b, int64_t M, int64_t d,
             double sigma, double ell, double* out) {
    return gpmi_cov(c, 0, a, N, b, M, d, sigma, ell, out);
}

static int cov_impl(gpmi_ctx* c, int kind, const double* a, int64_t N, const double* b, int64_t M, int64_t d,
                    double p0, double p1, const double* kpv, double* out) {
    const double sigma = p0, ell = p1;
    if (!c || !a || !b || !out) return fail_arg("gpmi_rbf: null argument");
    if (N < 0 || M < 0 || d <= 0) return fail_arg("gpmi_rbf: bad dimensions");
    if (cov_stationary(kind) && !(ell != 0.0)) return fail_arg("gpmi_rbf: ell must be non-zero");
    if (kind == 2 && (d != 1 || !(p0 != 0.0) || !(p1 != 0.0)))
        return fail_arg("gpmi_cov: the periodic kernel is 1-D with non-zero period and lengthscale");
    if (N == 0 || M == 0) return GPMI_OK;
    HIP_TRY(hipSetDevice(c->device));
    TuneScope tune_scope(&c->tune);
    hipStream_t s = c->stream;
    DevBuf &da = c->cov_a, &db = c->cov_b, &dout = c->cov_out;   // pooled: grow-only, freed with the context
    const int64_t Mp = round_up(M, TILE), ld = Mp + 32;
    const int64_t chunk = std::max<int64_t>(TILE, std::min<int64_t>(round_up(N, TILE),
                          ((int64_t)1 << 30) / (ld * 8) / TILE * TILE));
    int rc = GPMI_OK;
    hipError_t e;
    double max_sq = -1.0;
    if (cov_stationary(kind)) {
        Box ba, bb;
        ba.assign(a, N, d);
        bb.assign(b, M, d);
        max_sq = box_max_sq(ba, bb);
    }
    do {
        if ((e = da.ensure((size_t)N * d * 8)) != hipSuccess) { rc = fail_runtime(e, "hipMalloc a"); break; }
        if ((e = db.ensure((size_t)M * d * 8)) != hipSuccess) { rc = fail_runtime(e, "hipMalloc b"); break; }
        if ((e = dout.ensure((size_t)chunk * ld * 8)) != hipSuccess) { rc = fail_runtime(e, "hipMalloc out"); break; }
        if ((e = hipMemcpyAsync(da.p, a, (size_t)N * d * 8, hipMemcpyHostToDevice, s)) != hipSuccess ||
            (e = hipMemcpyAsync(db.p, b, (size_t)M * d * 8, hipMemcpyHostToDevice, s)) != hipSuccess) {
            rc = fail_runtime(e, "hipMemcpy H2D"); break;
        }
        for (int64_t r0 = 0; r0 < N && rc == GPMI_OK; r0 += chunk) {
            const int64_t rows = std::min(chunk, N - r0);
            RbfArgs r;
            r.A = da.as<double>(); r.B = db.as<double>();
            r.nA = N; r.nB = M; r.d = d; r.row0 = r0; r.nrows = round_up(rows, TILE); r.ncols = Mp;
            r.coef = cov_stationary(kind) ? cov_coef(kind, ell) : 0.; r.sig2 = sigma * sigma; r.diag_add = 0.; r.symmetric = 0;
            r.kind = kind; r.kp0 = p0; r.kp1 = p1;
            if (kpv) for (int i = 0; i < 11; ++i) r.kpv[i] = kpv[i];
            r.delta_square = (N == M) ? 1 : 0;
            r.max_sq = max_sq;
            r.out = dout.as<double>(); r.ld = ld;
            if ((e = launch_rbf(s, r)) != hipSuccess) { rc = fail_runtime(e, "rbf kernel"); break; }
            if ((e = hipMemcpy2DAsync(out + r0 * M, (size_t)M * 8, dout.p, (size_t)ld * 8, (size_t)M * 8,
                                      (size_t)rows, hipMemcpyDeviceToHost, s)) != hipSuccess ||
                (e = hipStreamSynchronize(s)) != hipSuccess) {
                rc = fail_runtime(e, "rbf D2H"); break;
            }
        }
    } while (0);
    (void)hipStreamSynchronize(s);
    return rc;
}

int gpmi_set_train(gpmi_ctx* c, const double* X, int64_t N, int64_t d, const double* y) {
    if (!c || !X || !y) return fail_arg("gpmi_set_train: null argument");
    if (N <= 0 || d <= 0) return fail_arg("gpmi_set_train: N and d must be positive");
    HIP_TRY(hipSetDevice(c->device));
    c->res.drop_train();
    c->release_sparse_grad();
    HIP_TRY(c->X.ensure((size_t)N * d * 8));
    HIP_TRY(c->y.ensure((size_t)N * 8));
    HIP_TRY(hipMemcpyAsync(c->X.p, X, (size_t)N * d * 8, hipMemcpyHostToDevice, c->stream));
    HIP_TRY(hipMemcpyAsync(c->y.p, y, (size_t)N * 8, hipMemcpyHostToDevice, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
    c->N = N; c->d = d;
    c->boxX.assign(X, N, d);
    if (c->ard() && (int64_t)c->ard_r.size() != d) c->ard_r.clear();    // another d: back to isotropic
    int rc = ard_rescale_train(c);
    if (rc) return rc;
    c->res.train_set();
    return GPMI_OK;
}

int gpmi_set_lengthscales(gpmi_ctx* c, const double* r, int64_t d) {
    if (!c) return fail_arg("gpmi_set_lengthscales: null context");
    if (d < 0) return fail_arg("gpmi_set_lengthscales: d < 0");
    if (r && d > 0) {
        if (c->res.have_train && d != c->d) return fail_arg("gpmi_set_lengthscales: d differs from the resident training set's");
        for (int64_t k = 0; k < d; ++k)
            if (!std::isfinite(r[k]) || !(r[k] > 0.0)) return fail_arg("gpmi_set_lengthscales: every lengthscale must be finite and > 0");
    }
    HIP_TRY(hipSetDevice(c->device));
    // as a new training set: whatever was fitted belongs to the old covariance
    c->res.drop_fit();
    if (r && d > 0) c->ard_r.assign(r, r + d);
    else c->ard_r.clear();
    if (!c->ard()) return GPMI_OK;
    HIP_TRY(c->ard_rdev.ensure((size_t)d * 8));
    HIP_TRY(hipMemcpyAsync(c->ard_rdev.p, c->ard_r.data(), (size_t)d * 8, hipMemcpyHostToDevice, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
    int rc = c->res.have_train ? ard_rescale_train(c) : GPMI_OK;
    if (rc == GPMI_OK && c->res.have_train && c->res.have_test) rc = ard_rescale_test(c);
    return rc;
}

int gpmi_factorize(gpmi_ctx* c, double sigma, double ell, double noise_var, double* lml,
                   int64_t* bad_pivot) {
    if (!c) return fail_arg("gpmi_factorize: null context");
    HIP_TRY(hipSetDevice(c->device));
    TuneScope tune_scope(&c->tune);
    return factorize_impl(c, sigma, ell, noise_var, lml, bad_pivot);
}

int gpmi_fit(gpmi_ctx* c, const double* X, int64_t N, int64_t d, const double* y, double sigma,
             double ell, double noise_var, double* lml, int64_t* bad_pivot) {
    int rc = gpmi_set_train(c, X, N, d, y);
    if (rc) return rc;
    return gpmi_factorize(c, sigma, ell, noise_var, lml, bad_pivot);
}

// k more observations into the resident regression factorisation: the border of the factor, not a new fit (append.hip).
// It solves and factors with the kind of leaves that produced the resident factor, so the factor stays of one kind.
int gpmi_append(gpmi_ctx* c, const double* Xnew, int64_t k, const double* ynew, double* lml, int64_t* bad_pivot) {
    if (!c) return fail_arg("gpmi_append: null context");
    HIP_TRY(hipSetDevice(c->device));
    const Tuning tn = resident_tuning(c);
    TuneScope tune_scope(&tn);
    return append_impl(c, Xnew, k, ynew, lml, bad_pivot);
}

// k observations out of the resident regression factorisation: a positive rank-k update of the trailing factor, not a
// new fit (remove.hip).  No element of K is evaluated, so every covariance kind is served.
int gpmi_remove(gpmi_ctx* c, const int64_t* idx, int64_t k, double* lml) {
    if (!c) return fail_arg("gpmi_remove: null context");
    HIP_TRY(hipSetDevice(c->device));
    const Tuning tn = resident_tuning(c);
    TuneScope tune_scope(&tn);
    return remove_impl(c, idx, k, lml);
}

int gpmi_get_layout(gpmi_ctx* c, int64_t* out5) {
    if (!c || !out5) return fail_arg("gpmi_get_layout: null argument");
    out5[0] = c->res.have_train ? c->N : 0;
    out5[1] = c->Np;
    out5[2] = c->ldA;
    out5[3] = c->rows_cap;
    out5[4] = c->append_route;
    return GPMI_OK;
}

int gpmi_get_m(gpmi_ctx* c, double* m_out) {
    if (!c || !m_out) return fail_arg("gpmi_get_m: null argument");
    if (!c->res.regression()) return fail_arg("gpmi_get_m: no factorisation resident");
    HIP_TRY(hipSetDevice(c->device));
    HIP_TRY(hipMemcpyAsync(m_out, c->m_row(), (size_t)c->N * 8,
                           hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
    return GPMI_OK;
}

int gpmi_get_diag(gpmi_ctx* c, double* diag_out) {
    if (!c || !diag_out) return fail_arg("gpmi_get_diag: null argument");
    if (!c->res.regression()) return fail_arg("gpmi_get_diag: no factorisation resident");
    HIP_TRY(hipSetDevice(c->device));
    HIP_TRY(hipMemcpy2DAsync(diag_out, 8, c->A.p, (size_t)(c->ldA + 1) * 8, 8, (size_t)c->N,
                             hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
    return GPMI_OK;
}

int gpmi_get_factor_block(gpmi_ctx* c, int64_t r0, int64_t r1, int64_t c0, int64_t c1, double* out) {
    if (!c || !out) return fail_arg("gpmi_get_factor_block: null argument");
    if (!c->res.regression()) return fail_arg("gpmi_get_factor_block: no factorisation resident");
    if (r0 < 0 || c0 < 0 || r1 > c->N || c1 > c->N || r0 > r1 || c0 > c1)
        return fail_arg("gpmi_get_factor_block: block out of range");
    if (r0 == r1 || c0 == c1) return GPMI_OK;
    HIP_TRY(hipSetDevice(c->device));
    const size_t bytes = (size_t)(r1 - r0) * (c1 - c0) * 8;
    HIP_TRY(c->dense.ensure(bytes));
    HIP_TRY(launch_extract(c->stream, c->A.as<double>(), c->ldA, r0, r1, c0, c1, c->dense.as<double>(), 1));
    HIP_TRY(hipMemcpyAsync(out, c->dense.p, bytes, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
    return GPMI_OK;
}

int gpmi_get_alpha(gpmi_ctx* c, double* alpha_out) {
    if (!c || !alpha_out) return fail_arg("gpmi_get_alpha: null argument");
    HIP_TRY(hipSetDevice(c->device));
    TuneScope tune_scope(&c->tune);
    return alpha_impl(c, alpha_out);
}

int gpmi_set_test(gpmi_ctx* c, const double* Xs, int64_t n) {
    if (!c || !Xs) return fail_arg("gpmi_set_test: null argument");
    if (!c->res.have_train) return fail_arg("gpmi_set_test: set the training set first");
    if (n <= 0) return fail_arg("gpmi_set_test: n must be positive");
    HIP_TRY(hipSetDevice(c->device));
    c->res.drop_test();
    HIP_TRY(c->Xs.ensure((size_t)n * c->d * 8));
    HIP_TRY(hipMemcpyAsync(c->Xs.p, Xs, (size_t)n * c->d * 8, hipMemcpyHostToDevice, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
    c->hXs.assign(Xs, Xs + (size_t)n * c->d);
    c->boxXs.assign(Xs, n, c->d);
    c->n = n;
    c->np_ = round_up(n, TILE);
    int rc = ard_rescale_test(c);
    if (rc) return rc;
    c->res.test_set();
    return GPMI_OK;
}

int gpmi_predict_resident(gpmi_ctx* c, double* mu, double* out2, int want_sd) {
    if (!c) return fail_arg("gpmi_predict: null context");
    HIP_TRY(hipSetDevice(c->device));
    const Tuning tn = resident_tuning(c);
    TuneScope tune_scope(&tn);
    return predict_resident_impl(c, mu, out2, want_sd);
}

// prediction() in one pass (a11 = a1 .. a8 for a training AND a test set known up front, GP_regression.py:109-156): the
// rows K(X*, X) are appended below the y row, so the panel solves and trailing updates of the Cholesky turn them into
// v^T = K_s^T L^-T on the way (a7 costs no launches of its own and fills the chip while the last, short updates leave
// it idle), and mean / variance are read off behind the LML.  Same results as gpmi_factorize + gpmi_predict_resident to
// rounding (the block widths of the two sweeps can differ).
int gpmi_fit_predict_resident(gpmi_ctx* c, double sigma, double ell, double noise_var, double* lml, int64_t* bad_pivot,
                              double* mu, double* out2, int want_sd) {
    if (!c) return fail_arg("gpmi_fit_predict: null context");
    if (!c->res.have_test) return fail_arg("gpmi_fit_predict: no test set (call gpmi_set_test)");
    HIP_TRY(hipSetDevice(c->device));
    TuneScope tune_scope(&c->tune);
    return factorize_impl(c, sigma, ell, noise_var, lml, bad_pivot, true, mu, out2, want_sd);
}

// prediction() WITH its posterior-sample factor in one pass (a11 + f1, GP_regression.py:109-156): one Cholesky of the augmented
//     [[K + sI, .], [K(X*, X), K_ss + jitter I]]        (N + n columns; the y rows ride below)
// -- its first N columns are L, the test rows' first N columns v^T, and its last n columns cholesky(K_ss + jitter I - v^T v):
// the Schur complement the trailing updates leave there IS the posterior covariance.  Same flops as the three separate steps
// ((N + n)^3 / 3), no SYRK launch and no second factorisation.  L_out (n x n row-major, zeros above the diagonal) may be
// null: gpmi_post_chol with the same jitter then only downloads it.
int gpmi_fit_predict_sample_resident(gpmi_ctx* c, double sigma, double ell, double noise_var, double jitter, double* lml,
                                     int64_t* bad_pivot, double* mu, double* out2, int want_sd, double* L_out) {
    if (!c) return fail_arg("gpmi_fit_predict_sample: null context");
    if (!c->res.have_test) return fail_arg("gpmi_fit_predict_sample: no test set (call gpmi_set_test)");
    HIP_TRY(hipSetDevice(c->device));
    TuneScope tune_scope(&c->tune);
    int rc = factorize_impl(c, sigma, ell, noise_var, lml, bad_pivot, true, mu, out2, want_sd, true, jitter);
    if (rc || !L_out) return rc;
    return gpmi_post_chol(c, jitter, L_out, bad_pivot);
}

int gpmi_predict(gpmi_ctx* c, const double* Xs, int64_t n, double* mu, double* out2, int want_sd) {
    int rc = gpmi_set_test(c, Xs, n);
    if (rc) return rc;
    return gpmi_predict_resident(c, mu, out2, want_sd);
}

// the gradients of the prediction at the resident test inputs (predgrad.hip); solves with the resident factor's kind of leaves
int gpmi_predict_grad_resident(gpmi_ctx* c, double* mu, double* var, double* dmu, double* dvar) {
    if (!c) return fail_arg("gpmi_predict_grad: null context");
    HIP_TRY(hipSetDevice(c->device));
    const Tuning tn = resident_tuning(c);
    TuneScope tune_scope(&tn);
    return predict_grad_impl(c, mu, var, dmu, dvar);
}

// Regression behind its fit (regress.hip): the gradient and leave-one-out calls solve with the kind of leaves that produced
// the resident factor; the posterior-sample factor is a factorisation of its own and takes the context's options
int gpmi_lml_grad(gpmi_ctx* c, double* d_ell, double* d_sigma) {
    if (!c || !d_ell || !d_sigma) return fail_arg("gpmi_lml_grad: null argument");
    HIP_TRY(hipSetDevice(c->device));
    const Tuning tn = resident_tuning(c);
    TuneScope tune_scope(&tn);
    return lml_grad_impl(c, d_ell, d_sigma);
}

int gpmi_lml_grad_ard(gpmi_ctx* c, double* d_r, double* d_ell, double* d_sigma, double* d_noise) {
    if (!c) return fail_arg("gpmi_lml_grad_ard: null context");
    HIP_TRY(hipSetDevice(c->device));
    const Tuning tn = resident_tuning(c);
    TuneScope tune_scope(&tn);
    return lml_grad_ard_impl(c, d_r, d_ell, d_sigma, d_noise);
}

int gpmi_lml_grad_co2(gpmi_ctx* c, double* d_theta, double* d_noise) {
    if (!c) return fail_arg("gpmi_lml_grad_co2: null context");
    HIP_TRY(hipSetDevice(c->device));
    const Tuning tn = resident_tuning(c);
    TuneScope tune_scope(&tn);
    return lml_grad_co2_impl(c, d_theta, d_noise);
}

int gpmi_loo(gpmi_ctx* c, double* mu, double* var, double* logp, double* loo) {
    if (!c) return fail_arg("gpmi_loo: null context");
    HIP_TRY(hipSetDevice(c->device));
    const Tuning tn = resident_tuning(c);
    TuneScope tune_scope(&tn);
    return loo_impl(c, mu, var, logp, loo);
}

int gpmi_loo_grad(gpmi_ctx* c, double* d_ell, double* d_sigma, double* d_noise) {
    if (!c) return fail_arg("gpmi_loo_grad: null context");
    HIP_TRY(hipSetDevice(c->device));
    const Tuning tn = resident_tuning(c);
    TuneScope tune_scope(&tn);
    return loo_grad_impl(c, d_ell, d_sigma, d_noise);
}

int gpmi_grad_trace(gpmi_ctx* c, const double* a_in, const double* b_in, int64_t N, int64_t d, double sigma,
                    double ell, const double* alpha_in, const double* Kinv_in, double* d_ell, double* d_sigma) {
    if (!c || !a_in || !b_in || !alpha_in || !Kinv_in || !d_ell || !d_sigma) return fail_arg("gpmi_grad_trace: null argument");
    HIP_TRY(hipSetDevice(c->device));
    return grad_trace_impl(c, a_in, b_in, N, d, sigma, ell, alpha_in, Kinv_in, d_ell, d_sigma);
}

int gpmi_post_chol(gpmi_ctx* c, double jitter, double* L_out, int64_t* bad_pivot) {
    if (!c || !L_out) return fail_arg("gpmi_post_chol: null argument");
    HIP_TRY(hipSetDevice(c->device));
    TuneScope tune_scope(&c->tune);
    return post_chol_impl(c, jitter, L_out, bad_pivot);
}

int gpmi_post_sample(gpmi_ctx* c, double jitter, const double* Z, int64_t num_fun, double* LZ_out, int64_t* bad_pivot) {
    if (!c || !Z || !LZ_out) return fail_arg("gpmi_post_sample: null argument");
    HIP_TRY(hipSetDevice(c->device));
    TuneScope tune_scope(&c->tune);
    return post_sample_impl(c, jitter, Z, num_fun, LZ_out, bad_pivot);
}

// Lane l of a batch: its own context (streams, A, workspaces) on the same device, with the parent's
// training set copied device to device.  Small and mid-size factorisations leave most of the chip idle
// in their latency-bound panel steps; two in flight fill it (measured per triple, 1 -> 2 lanes: N = 512
// 0.45 -> 0.24 ms, N = 2048 1.74 -> 0.93 ms, N = 8192 10.5 -> 6.9 ms, N = 16384 39.5 -> 32.1 ms,
// N = 32768 213 -> 201 ms).
static int lane_prepare(gpmi_ctx* c, gpmi_ctx* l) {
    l->nb = c->nb; l->ld_pad = c->ld_pad; l->lookahead = c->lookahead; l->la_min = c->la_min; l->timing = c->timing;
    l->tune = c->tune;
    l->kind = c->kind; l->kp0 = c->kp0; l->kp1 = c->kp1;
    for (int i = 0; i < 11; ++i) l->kpv[i] = c->kpv[i];
    l->N = c->N; l->d = c->d; l->boxX = c->box_train();    // a lane is isotropic on the parent's (scaled) inputs
    HIP_TRY(l->X.ensure((size_t)c->N * c->d * 8));
    HIP_TRY(l->y.ensure((size_t)c->N * 8));
    HIP_TRY(hipMemcpyAsync(l->X.p, c->x_train(), (size_t)c->N * c->d * 8, hipMemcpyDeviceToDevice, l->stream));
    HIP_TRY(hipMemcpyAsync(l->y.p, c->y.p, (size_t)c->N * 8, hipMemcpyDeviceToDevice, l->stream));
    HIP_TRY(hipStreamSynchronize(l->stream));
    l->res.drop_train();
    l->res.train_set();
    return GPMI_OK;
}

int gpmi_lml_batch(gpmi_ctx* c, const double* triples, int64_t T, double* lml_out, int* status_out) {
    if (!c || !triples || !lml_out) return fail_arg("gpmi_lml_batch: null argument");
    if (T < 0) return fail_arg("gpmi_lml_batch: T < 0");
    if (!c->res.have_train) return fail_arg("gpmi_lml_batch: no training set (call gpmi_set_train)");
    HIP_TRY(hipSetDevice(c->device));
    const int64_t Np = round_up(c->N, TILE);
    // lanes by size, measured with 24 triples per call (round 4, profiles/r04_lml_batch_lanes_small.txt; ms per triple with
    // 2 / 3 / 4 / 5 / 6 lanes): N = 512 0.159 / 0.112 / 0.092 / 0.161 / 0.163, 2048 0.572 / 0.408 / 0.322 / 0.468 / 0.505,
    // 8192 5.21 / 4.46 / 4.13 / 4.85 / 4.75 -- four single-stream lanes below the lookahead threshold (round 2's "two, more
    // do not help" was measured with four hardware queues; _lib.py now asks for eight); 12288 12.6 / 12.4 / 12.1 / 11.8 /
    // 11.8 and 16384 26.5 / 25.3 / 26.2 / 24.8 / 24.8 -- five there; N = 32768 (profiles/r04_cfg5_lanes.txt) 0.1934 / 0.1865 /
    // 0.1849 / 0.1855 s with 1 / 2 / 3 / 4 -- three
    int L = c->lanes ? c->lanes : (Np > 32768 ? 1 : Np >= 24576 ? 3 : Np >= 12288 ? 5 : 4);
    L = (int)std::min<int64_t>(L, std::max<int64_t>(T, 1));
    // lanes beside each other fill the chip themselves: below 12288 columns every lane runs on ONE stream (a lane's
    // lookahead would add a second stream per lane and loses: N = 8192, 3 lanes 4.46 ms per triple without, 5.45 with;
    // profiles/r04_la_min_batch.txt), whatever the threshold of this context's single fits
    struct LaMinScope {
        gpmi_ctx* c; int64_t keep;
        ~LaMinScope() { c->la_min = keep; }
    } la_scope{c, c->la_min};
    if (L > 1) c->la_min = std::max<int64_t>(c->la_min, 12288);
    while ((int)c->lane_ctx.size() < L - 1) {
        gpmi_ctx* l = nullptr;
        int rc = gpmi_ctx_create(c->device, &l);
        if (rc) return rc;
        c->lane_ctx.push_back(l);
    }
    for (int j = 0; j < L - 1; ++j) {
        int rc = lane_prepare(c, c->lane_ctx[(size_t)j]);
        if (rc) return rc;
    }
    // residue class r of the triple index runs on lane r; the parent context takes the class of the last
    // triple, so the factor left resident afterwards is that of triples[T-1], as with one lane
    const int parent_class = (int)((T - 1 + L) % L);
    std::vector<gpmi_ctx*> lane((size_t)L);
    for (int r = 0, nx = 0; r < L; ++r) lane[(size_t)r] = (r == parent_class) ? c : c->lane_ctx[(size_t)nx++];
    std::vector<int> lane_rc((size_t)L, GPMI_OK);
    std::vector<std::string> lane_err((size_t)L);
    std::vector<std::vector<double>> lane_ms((size_t)L, std::vector<double>(GPMI_T_COUNT, 0.0));
    auto work = [&](int r) {
        gpmi_ctx* l = lane[(size_t)r];
        TuneScope tune_scope(&l->tune);         // this lane's thread runs with this lane's options
        SharingScope shares_chip(L > 1 ? sharing().and_chip_shared() : sharing());   // another lane's kernels run beside this one's: no launch takes the whole chip
        if (hipSetDevice(l->device) != hipSuccess) { lane_rc[(size_t)r] = GPMI_ERR_RUNTIME; lane_err[(size_t)r] = "hipSetDevice"; return; }
        for (int64_t t = r; t < T; t += L) {
            const double ell = triples[3 * t], sigma = triples[3 * t + 1], s2 = triples[3 * t + 2];
            double lml = 0.;
            int64_t bad = 0;
            const int rc = factorize_impl(l, sigma, ell, s2, &lml, &bad);
            if (rc == GPMI_ERR_RUNTIME || rc == GPMI_ERR_BAD_ARG) {
                lane_rc[(size_t)r] = rc;
                lane_err[(size_t)r] = g_err;       // this thread's message
                return;
            }
            lml_out[t] = lml;
            if (status_out) status_out[t] = rc;
            for (int i = 0; i < GPMI_T_COUNT; ++i) lane_ms[(size_t)r][(size_t)i] += l->stage_ms[i];
        }
    };
    if (L == 1) {
        work(0);
    } else {
        std::vector<std::thread> th;
        for (int r = 0; r < L; ++r) th.emplace_back(work, r);
        for (auto& t : th) t.join();
    }
    for (int r = 0; r < L; ++r)
        if (lane_rc[(size_t)r] != GPMI_OK) {
            g_err = lane_err[(size_t)r];
            return lane_rc[(size_t)r];
        }
    for (int i = 0; i < GPMI_T_COUNT; ++i) {
        c->stage_ms[i] = 0.0;
        for (int r = 0; r < L; ++r) c->stage_ms[i] += lane_ms[(size_t)r][(size_t)i];
    }
    return GPMI_OK;
}

// Binary GP classification, GPML Algorithms 3.1 / 3.2 with the logistic likelihood (laplace.hip)
int gpmi_laplace_fit(gpmi_ctx* c, double sigma, double ell, double tol, int max_iter, double* log_q, int* iters,
                     int* converged, double* f_hat) {
    if (!c) return fail_arg("gpmi_laplace_fit: null context");
    HIP_TRY(hipSetDevice(c->device));
    TuneScope tune_scope(&c->tune);
    return laplace_fit_impl(c, sigma, ell, tol, max_iter, log_q, iters, converged, f_hat);
}

int gpmi_laplace_predict_resident(gpmi_ctx* c, double* f_mean, double* f_var, double* prob) {
    if (!c) return fail_arg("gpmi_laplace_predict: null context");
    HIP_TRY(hipSetDevice(c->device));
    return laplace_predict_impl(c, f_mean, f_var, prob);
}

int gpmi_laplace_grad(gpmi_ctx* c, double* d_r, double* d_ell, double* d_sigma) {
    if (!c) return fail_arg("gpmi_laplace_grad: null context");
    HIP_TRY(hipSetDevice(c->device));
    return laplace_grad_impl(c, d_r, d_ell, d_sigma);
}

// Multi-class GP classification, GPML Algorithms 3.3 / 3.4 with the softmax likelihood (softmax.hip)
int gpmi_softmax_fit(gpmi_ctx* c, int n_classes, double sigma, double ell, double tol, int max_iter, double* log_q,
                     int* iters, int* converged, double* f_hat) {
    if (!c) return fail_arg("gpmi_softmax_fit: null context");
    HIP_TRY(hipSetDevice(c->device));
    TuneScope tune_scope(&c->tune);
    return softmax_fit_impl(c, n_classes, sigma, ell, tol, max_iter, log_q, iters, converged, f_hat);
}

int gpmi_softmax_predict_resident(gpmi_ctx* c, double* mu, double* cov, int64_t n_samples, const double* normals,
                                  double* prob) {
    if (!c) return fail_arg("gpmi_softmax_predict: null context");
    HIP_TRY(hipSetDevice(c->device));
    return softmax_predict_impl(c, mu, cov, n_samples, normals, prob);
}

int gpmi_softmax_grad(gpmi_ctx* c, double* d_r, double* d_ell, double* d_sigma) {
    if (!c) return fail_arg("gpmi_softmax_grad: null context");
    HIP_TRY(hipSetDevice(c->device));
    return softmax_grad_impl(c, d_r, d_ell, d_sigma);
}

int gpmi_sparse_fit(gpmi_ctx* c, const double* Z, int64_t m, double sigma, double ell, double noise_var, double jitter,
                    int method, double* value, int64_t* bad_pivot) {
    if (!c || !Z) return fail_arg("gpmi_sparse_fit: null argument");
    HIP_TRY(hipSetDevice(c->device));
    TuneScope tune_scope(&c->tune);
    return sparse_fit_impl(c, Z, m, sigma, ell, noise_var, jitter, method, value, bad_pivot);
}

int gpmi_sparse_predict_resident(gpmi_ctx* c, double* mu, double* out2, int want_sd) {
    if (!c) return fail_arg("gpmi_sparse_predict: null context");
    HIP_TRY(hipSetDevice(c->device));
    return sparse_predict_impl(c, mu, out2, want_sd);
}

int gpmi_sparse_get(gpmi_ctx* c, double* c_out, double* q_out) {
    if (!c) return fail_arg("gpmi_sparse_get: null context");
    HIP_TRY(hipSetDevice(c->device));
    return sparse_get_impl(c, c_out, q_out);
}

int gpmi_sparse_grad(gpmi_ctx* c, double* d_ell, double* d_sigma, double* d_noise, double* d_r, double* d_Z) {
    if (!c) return fail_arg("gpmi_sparse_grad: null context");
    HIP_TRY(hipSetDevice(c->device));
    return sparse_grad_impl(c, d_ell, d_sigma, d_noise, d_r, d_Z);
}

int gpmi_get_timers(gpmi_ctx* c, double* stage_ms, int count) {
    if (!c || !stage_ms) return fail_arg("gpmi_get_timers: null argument");
    for (int i = 0; i < count; ++i) stage_ms[i] = i < GPMI_T_COUNT ? c->stage_ms[i] : 0.;
    return GPMI_OK;
}

}  // extern "C"
