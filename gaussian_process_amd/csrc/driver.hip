// Single-GPU drivers behind the C-ABI: recursive panel factorisation, the recursive triangular
// solve of a block, the blocked right-looking Cholesky with lookahead, the TRSM sweep for
// v = L^-1 K_s (and for L^-T), and the fit (K build + Cholesky + LML) they add up to.
// Data layout: see gpmi_api.hip.
#include "gpmi_ctx.h"
#include "gpmi_plan.h"

namespace gpmi {

// ---------------------------------------------------------------------------
// Panel factorisation: the nb-wide block column whose diagonal block starts at
// A (global column col_offset), `mrows` rows tall (mrows >= nb, multiple of
// 128).  Recursive halving down to 64 columns:
//   factor the left half (all rows), update the right half with ONE MFMA GEMM of
//   depth = width of the left half, factor the right half.
// The leaves are the 64 x 64 potf2 and the substitution TRSM of every row below
// it.  Same flops and the same number of launches as a flat right-looking sweep
// in 64-column steps, but half of the update flops run at depth >= nb/4 instead of
// 64, and the panel is streamed 2.3x less often.
// ---------------------------------------------------------------------------
hipError_t panel_rec(hipStream_t s, double* A, int64_t ld, int64_t mrows, int64_t off, int64_t w,
                     int64_t col_offset, int64_t* info) {
    hipError_t e;
    // leaves: 128 columns on the matrix pipe (potrf128 + trsm128, panel_mfma.hip), or -- option
    // "panel_fused" 0, and widths that are not a multiple of 128 -- the first-generation 64-column pair
    const bool fused = tuning().panel_fused && w % 128 == 0 && off % 128 == 0;
    const int64_t leaf = fused ? 128 : IB;
    if (w <= leaf) {
        double* Ajj = A + off * ld + off;
        const int64_t below = mrows - off - leaf;
        if (fused) {
            if ((e = launch_potrf128(s, Ajj, ld, col_offset + off, info)) != hipSuccess) return e;
            if (below > 0) return launch_trsm128(s, Ajj, ld, A + (off + leaf) * ld + off, ld, below);
            return hipSuccess;
        }
        if ((e = launch_potf2_64(s, Ajj, ld, col_offset + off, info)) != hipSuccess) return e;
        if (below > 0) return launch_trsm_rlt64(s, Ajj, ld, A + (off + IB) * ld + off, ld, below);
        return hipSuccess;
    }
    const int64_t h = (w / 2) / leaf * leaf;       // left width (multiple of the leaf width, >= one leaf)
    if ((e = panel_rec(s, A, ld, mrows, off, h, col_offset, info)) != hipSuccess) return e;
    {
        // right half -= (rows of the left half) * (its own rows of the left half)^T, lower part.
        // Rows start at the 128-aligned row at or above off+h: the extra 64 rows (when off+h is
        // not a multiple of 128) lie above the diagonal of the updated columns and are never read.
        const int64_t c0 = off + h;
        const int64_t r0 = c0 / TILE * TILE;
        const GemmArgs g = gemm_minus_lower(A + r0 * ld + c0, ld, A + r0 * ld + off, ld, A + c0 * ld + off, ld, mrows - r0,
                                            w - h, h, r0 - c0);
        if ((e = launch_gemm_nt(s, g)) != hipSuccess) return e;
    }
    return panel_rec(s, A, ld, mrows, off + h, w - h, col_offset, info);
}

hipError_t panel_factor(hipStream_t s, double* A, int64_t ld, int64_t nb, int64_t mrows,
                        int64_t col_offset, int64_t* info) {
    return panel_rec(s, A, ld, mrows, 0, nb, col_offset, info);
}

// X (m x nb) <- X * L^-T, L nb x nb lower; m multiple of 128, nb multiple of 64.
// Same recursion: X1 <- X1 L11^-T;  X2 <- (X2 - X1 L21^T) L22^-T.
hipError_t trsm_rec(hipStream_t s, const double* L, int64_t ldl, double* X, int64_t ldx, int64_t m,
                    int64_t off, int64_t w) {
    hipError_t e;
    const bool fused = tuning().panel_fused && w % 128 == 0 && off % 128 == 0 && m % 128 == 0;
    const int64_t leaf = fused ? 128 : IB;
    if (w <= leaf) {
        if (fused) return launch_trsm128(s, L + off * ldl + off, ldl, X + off, ldx, m);
        return launch_trsm_rlt64(s, L + off * ldl + off, ldl, X + off, ldx, m);
    }
    const int64_t h = (w / 2) / leaf * leaf;
    if ((e = trsm_rec(s, L, ldl, X, ldx, m, off, h)) != hipSuccess) return e;
    const GemmArgs g = gemm_minus(X + off + h, ldx, X + off, ldx, L + (off + h) * ldl + off, ldl, m, w - h, h);
    if ((e = launch_gemm_nt(s, g)) != hipSuccess) return e;
    return trsm_rec(s, L, ldl, X, ldx, m, off + h, w - h);
}

hipError_t trsm_block(hipStream_t s, const double* L, int64_t ldl, double* X, int64_t ldx,
                      int64_t m, int64_t nb) {
    return trsm_rec(s, L, ldl, X, ldx, m, 0, nb);
}

// In-place blocked right-looking Cholesky of the leading ncols x ncols block of
// A; rows ncols..nrows-1 are carried along (they end up multiplied by L^-T).
// Without lookahead every step is a panel and one trailing update on the main stream.
//
// With lookahead the trailing update of step k is split in two launches: (a) the next
// block column only and (b) the rest.  (a) goes on the panel stream (high priority), right behind panel k and in
// front of panel k+1, (b) on the main stream.  (a) and (b) write different columns
// and both only read panel k, so they start together: the tail of (a) -- a launch whose last
// tiles leave most CUs idle -- and the whole latency-bound panel k+1 run under (b).  That pays at mid sizes
// (N = 16384: -4 %, 32768: -1 %), where a launch's tail and the panel chain are a visible share of a step, and at
// the headline size, where the tail of (a) is a smaller share but a 256 x 128 one, twice as long as a 128 x 128 tail
// (LAB_NOTES.md, "leftover 128 x 128 updates").
// From 49152 columns up the panel chain is 4-5x shorter than the step it runs under, so nothing on the critical path
// waits for a workgroup that holds its CU twice as long: the launches of such a factorisation -- (a), (b) and the
// updates inside the panel -- take the 256 x 128 form from tall_min_tiles_slack live tiles on (Sharing::panel_slack).
// Dependencies:
//   panel k  ->  (a)_k                 (same stream)
//   panel k  ->  (b)_k                 (main waits on the panel event)
//   (a)_k    ->  panel k+1             (same stream)
//   (b)_k    ->  (a)_{k+1}             (panel stream waits on the event behind (b)_k)
//   (b)_k    ->  (b)_{k+1}             (same stream)
hipError_t cholesky_inplace(gpmi_ctx* c, double* A, int64_t ld, int64_t ncols, int64_t nrows,
                            int64_t* info, bool account, int64_t carried_rows) {
    hipError_t e;
    hipStream_t sm = c->stream;
    const int64_t NB = c->block(ncols);
    const bool la = c->lookahead_for(ncols);
    hipStream_t sp_ = la ? c->pstream : sm;
    // panel kernels beside the trailing update use their small-LDS forms -- while there IS a trailing update of some length
    // to run beside: once the columns right of the panel are fewer than c->shallow_min, part (b) of a step is over long
    // before the panel chain is, and the one-launch forms (which then find empty CUs) are the shorter chain
    const bool slack = la && ncols >= 49152;
    SharingScope shallow(la ? Sharing::beside_update().with_panel_slack(slack) : sharing());
    const int slot_p = account ? GPMI_T_CHOL_PANEL : GPMI_T_COUNT - 1;
    const int slot_t = account ? GPMI_T_CHOL_TRAIL : GPMI_T_COUNT - 1;
    if (la && (e = c->order(sm, sp_)) != hipSuccess) return e;   // panel 0 after the K build
    // `counted`: the launch enters the roofline figures (GPMI_T_CHOL_TRAIL, its own kernel symbol).  Under lookahead
    // only (b) does: (a) runs at the same time on the other stream, so summing both durations would count that
    // time twice; (a) is launched under the generic symbol and timed with the panel it belongs to.
    auto trail = [&](hipStream_t st, bool counted, int64_t r0, int64_t c0, int64_t k, int64_t nb, int64_t ncol_upd) -> hipError_t {
        // C = A[r0.., c0..c0+ncol_upd) -= A[r0.., k..k+nb) * A[c0.., k..k+nb)^T, lower part
        GemmArgs g = gemm_minus_lower(A + r0 * ld + c0, ld, A + r0 * ld + k, ld, A + c0 * ld + k, ld, nrows - r0, ncol_upd,
                                      nb, r0 - c0);
        g.role = counted ? 1 : 0;
        // the roofline figures are those of the LDS-DMA kernel: the last, small updates that
        // run on the first-generation kernel are timed into the scratch slot
        const GemmRoute route = gemm_nt_route(g);
        const bool dma = gemm_kernel_is_dma(route.kernel);
        size_t sp = c->span_begin(counted ? (dma ? slot_t : GPMI_T_COUNT - 1) : slot_p, st);
        hipError_t er = launch_gemm_nt(st, g, route);
        c->span_end(sp, st);
        if (account && dma && counted) {
            c->stage_ms[GPMI_T_TRAIL_LAUNCHES] += 1.0;
            // algorithmic: the lower triangle of the real rows plus the one row that carries y (plus the test set's rows
            // when they ride along: all of them reach every column, so only their number counts)
            c->stage_ms[GPMI_T_TRAIL_FLOPS] += gemm_nt_algorithmic_flops(g, ncols - r0 + 1 + carried_rows);
        }
        return er;
    };
    hipEvent_t ev_b = nullptr;                    // behind the last (b) on the main stream
    for (int64_t k = 0; k < ncols; k += NB) {
        const int64_t nb = std::min<int64_t>(NB, ncols - k);
        size_t sp = c->span_begin(slot_p, sp_);
        {
            SharingScope panel_forms(!la ? sharing().large_lds()
                                     : (ncols - k >= c->shallow_min ? Sharing::beside_update() : Sharing::chip_shared_only()).with_panel_slack(slack));
            e = panel_factor(sp_, A + k * ld + k, ld, nb, nrows - k, k, info);
        }
        c->span_end(sp, sp_);
        if (e != hipSuccess) return e;
        if (la && (e = c->order(sp_, sm)) != hipSuccess) return e;
        const int64_t r0 = k + nb;
        if (r0 >= ncols) continue;
        if (!la) {
            if ((e = trail(sm, true, r0, r0, k, nb, ncols - r0)) != hipSuccess) return e;
            continue;
        }
        const int64_t nbn = std::min<int64_t>(NB, ncols - r0);
        // (a) next block column, behind panel k on the panel stream and behind (b) of the step before
        if (ev_b && (e = hipStreamWaitEvent(sp_, ev_b, 0)) != hipSuccess) return e;
        if ((e = trail(sp_, false, r0, r0, k, nb, nbn)) != hipSuccess) return e;
        if (r0 + nbn < ncols) {                                                          // (b) rest
            if ((e = trail(sm, true, r0 + nbn, r0 + nbn, k, nb, ncols - r0 - nbn)) != hipSuccess) return e;
            ev_b = c->new_event();
            if (!ev_b) return c->ev_error;
            if ((e = hipEventRecord(ev_b, sm)) != hipSuccess) return e;
        }
    }
    return hipSuccess;
}

RbfArgs rbf_cross(const gpmi_ctx* c, const double* A, int64_t nA, const Box& ba, const double* B, int64_t nB, const Box& bb,
                  int64_t row0, int64_t nrows, int64_t ncols, double* out, int64_t ld) {
    RbfArgs r;
    r.A = A; r.B = B;
    r.nA = nA; r.nB = nB; r.d = c->d; r.row0 = row0; r.nrows = nrows; r.ncols = ncols;
    r.coef = c->coef; r.sig2 = c->sig2;
    r.kind = c->kind; r.kp0 = c->kp0; r.kp1 = c->kp1;
    for (int i = 0; i < 11; ++i) r.kpv[i] = c->kpv[i];
    r.diag_add = 0.; r.symmetric = 0;
    // kernel_4's delta is eye whenever the matrix is square (CO2_example.py:58): the test set against the training set
    r.delta_square = (A == c->x_test() && B == c->x_train() && nA == nB) ? 1 : 0;
    r.max_sq = box_max_sq(ba, bb);
    r.out = out; r.ld = ld;
    return r;
}

RbfArgs rbf_sym(const gpmi_ctx* c, const double* X, int64_t n, const Box& box, double diag_add, int64_t npad, double* out,
                int64_t ld) {
    RbfArgs r = rbf_cross(c, X, n, box, X, n, box, 0, npad, npad, out, ld);
    r.diag_add = diag_add; r.symmetric = 1; r.delta_square = 1;
    return r;
}

RbfArgs rbf_test_train(const gpmi_ctx* c, double* out, int64_t ld) {
    return rbf_cross(c, c->x_test(), c->n, c->box_test(), c->x_train(), c->N, c->box_train(), 0, c->np_, c->Np, out, ld);
}

int ensure_train_buffers(gpmi_ctx* c, int64_t test_rows, bool test_cols) {
    c->spareA.release();               // any fit into A drops the buffer a removal kept
    c->pgW.release();                  // ... and the W of gpmi_predict_grad_resident
    c->Np = round_up(c->N, TILE);
    // option "reserve": columns and rows for that many more points, which gpmi_append then fills in place (0: cap == Np)
    const int64_t cap = round_up(c->N + c->reserve, TILE);
    c->ldA = cap + (test_cols ? test_rows : 0) + c->ld_pad;
    c->Mp = c->Np + TILE + test_rows;              // the rows a factorisation carries: never the reserve's
    c->rows_cap = cap + TILE + test_rows;          // the rows A has (the append plan's capacity)
    c->yrow = test_cols ? c->Np + test_rows : c->Np;         // with their own columns the test rows come BEFORE the y rows
    HIP_TRY(c->A.ensure((size_t)c->rows_cap * c->ldA * sizeof(double)));
    HIP_TRY(c->info.ensure(sizeof(int64_t)));
    HIP_TRY(c->red.ensure(16 * sizeof(double)));
    return GPMI_OK;
}

// mean and variance (or standard deviation) from the row dots of v^T: h = [v_i . m for i < n_p | v_i . v_i for i < n_p]
void meanvar_to_host(gpmi_ctx* c, const std::vector<double>& h, double* mu, double* out2, int want_sd) {
    for (int64_t i = 0; i < c->n; ++i) {
        if (mu) mu[i] = h[i];
        if (out2) {
            double kss = c->sig2;                          // diag(K_ss) == sigma^2 exactly for the RBF (GP_regression.py:147) and the Materns
            if (c->kind == 2) kss = 1.0;                   // periodic: exp(0)
            else if (c->kind == 3) {                       // composite at sqdist 0, square K_ss: every factor is 1
                const double* th = c->kpv;
                kss = ((th[0] * th[0] + th[2] * th[2]) + th[5] * th[5]) + (th[8] * th[8] + th[10] * th[10]);
            }
            else if (c->kind == 1) {                       // linear: (x - c).(x - c)
                kss = 0.0;
                for (int64_t k = 0; k < c->d; ++k) {
                    const double e = c->hXs[(size_t)i * c->d + k] - c->kp0;
                    kss = kss + e * e;
                }
            }
            const double var = kss - h[c->np_ + i];
            out2[i] = want_sd ? std::sqrt(var) : var;      // sqrt(<0) -> NaN like np.sqrt (:148)
        }
    }
}

// K build + Cholesky (+ forward solve through the y row) + LML on the stream
int factorize_impl(gpmi_ctx* c, double sigma, double ell, double noise_var, double* lml,
                   int64_t* bad_pivot, bool with_test, double* mu, double* out2, int want_sd, bool with_post, double jitter) {
    if (!c->res.have_train) return fail_arg("gpmi_factorize: no training set (call gpmi_set_train)");
    if (cov_stationary(c->kind) && (!(ell != 0.0) || std::isnan(ell) || std::isnan(sigma)))
        return fail_arg("gpmi_factorize: ell must be non-zero and hyper-parameters finite");
    if (std::isnan(noise_var)) return fail_arg("gpmi_factorize: noise_var is NaN");
    if (c->kind == 2 && c->d != 1) return fail_arg("gpmi_factorize: the periodic kernel is 1-D only (GP_regression.py:48)");
    if (!cov_stationary(c->kind) && c->ard())
        return fail_arg("gpmi_factorize: per-dimension lengthscales need the squared-exponential or a Matern kernel (kinds 0, 4, 5, 6)");
    // with_test: the test set's rows ride inside the panel and update launches of the factorisation (against a solve call
    // of their own, profiles/r04_one_pass_ab.txt, ms: N = 2048 1.69 -> 1.32, 8192 10.5 -> 8.94, 16384 37.5 -> 34.9, 32768
    // 262.7 -> 257.9, 65536 1702 -> 1698: riding costs no launches).  with_post (only with with_test): the augmented matrix,
    // where they ride with columns of their own
    if (with_post && std::isnan(jitter)) return fail_arg("gpmi_fit_predict_sample: jitter is NaN");
    c->res.drop_fit();                // a regression factorisation replaces whatever fit was resident
    c->release_sparse_grad();
    int rc = ensure_train_buffers(c, with_test ? c->np_ : 0, with_post);
    if (rc) return rc;
    hipStream_t s = c->stream;
    c->timers_reset({GPMI_T_KBUILD, GPMI_T_CHOL, GPMI_T_CHOL_PANEL, GPMI_T_CHOL_TRAIL, GPMI_T_LML,
                     GPMI_T_TRAIL_LAUNCHES, GPMI_T_TRAIL_FLOPS});
    if (with_test) c->timers_reset({GPMI_T_KS, GPMI_T_SOLVE_V, GPMI_T_MEANVAR});
    c->sig2 = sigma * sigma;
    c->coef = cov_coef(c->kind, ell);       // GP_regression.py:19 evaluation order; a Matern kind: -sqrt(2 nu) / |l|
    c->sigma = sigma; c->ell = ell; c->noise = noise_var;
    double* A = c->A.as<double>();
    const int64_t big = std::numeric_limits<int64_t>::max();
    HIP_TRY(hipMemcpyAsync(c->info.p, &big, sizeof big, hipMemcpyHostToDevice, s));

    size_t sp = c->span_begin(GPMI_T_KBUILD);
    const RbfArgs r = rbf_sym(c, c->x_train(), c->N, c->box_train(), noise_var, c->Np, A, c->ldA);
    HIP_TRY(launch_rbf(s, r));
    c->span_end(sp);                  // GPMI_T_KBUILD is the kernel-matrix build (a1 + a2) alone
    // the augmented rows: y then zeros (a4 rides in the factorisation)
    const int64_t ncols = c->Np + (with_post ? c->np_ : 0);   // columns of the factorisation
    HIP_TRY(launch_fill_rows(s, c->m_row(), c->ldA, TILE, ncols, 0.0));
    HIP_TRY(launch_set_yrow(s, c->m_row(), c->y.as<double>(), c->N, c->Np));
    c->v_row0 = with_post ? c->Np : c->Np + TILE;
    double* Vr = A + c->v_row0 * c->ldA;
    if (with_test) {                  // K(X*, X) below the y rows (a1 for K_s, GP_regression.py:127): they leave as v^T
        sp = c->span_begin(GPMI_T_KS);
        const RbfArgs t = rbf_test_train(c, Vr, c->ldA);
        HIP_TRY(launch_rbf(s, t));
        if (with_post) {              // K_ss + jitter I in the rows' own columns, lower tiles (GP_regression.py:128, 154)
            const RbfArgs q = rbf_sym(c, c->x_test(), c->n, c->box_test(), jitter, c->np_, Vr + c->Np, c->ldA);
            HIP_TRY(launch_rbf(s, q));
        }
        c->span_end(sp);
    }

    sp = c->span_begin(GPMI_T_CHOL);
    // test rows with columns of their own are rows of the factorisation, not carried ones
    HIP_TRY(cholesky_inplace(c, A, c->ldA, ncols, c->Mp, c->info.as<int64_t>(), true, with_test && !with_post ? c->n : 0));
    c->span_end(sp);

    sp = c->span_begin(GPMI_T_LML);
    HIP_TRY(launch_lml_reduce(s, A, c->ldA, c->m_row(), c->N, c->red.as<double>()));
    c->span_end(sp);

    std::vector<double> h;
    if (with_test) {                  // a6 + a8 off the finished rows: mean_i = v_i . m, sum of squares for the variance
        HIP_TRY(c->vec.ensure((size_t)std::max(c->Np, c->np_) * 4 * 8));
        sp = c->span_begin(GPMI_T_MEANVAR);
        double* dot = c->vec.as<double>();
        HIP_TRY(launch_row_dots(s, Vr, c->ldA, c->np_, c->Np, c->m_row(), dot, dot + c->np_));
        c->span_end(sp);
        h.resize(2 * (size_t)c->np_);
        HIP_TRY(hipMemcpyAsync(h.data(), dot, h.size() * 8, hipMemcpyDeviceToHost, s));
    }
    double red[2];
    int64_t info;
    HIP_TRY(hipMemcpyAsync(red, c->red.p, sizeof red, hipMemcpyDeviceToHost, s));
    HIP_TRY(hipMemcpyAsync(&info, c->info.p, sizeof info, hipMemcpyDeviceToHost, s));
    HIP_TRY(hipStreamSynchronize(s));
    c->timers_collect();
    if (info != big && (info < c->N || (with_post && info >= c->Np && info < c->Np + c->n))) {
        // a pivot of K + sI (GP_regression.py:138) or, in the augmented form, of the posterior covariance (:154; counted from
        // its own first column, as gpmi_post_chol reports it)
        if (bad_pivot) *bad_pivot = info < c->N ? info + 1 : info - c->Np + 1;
        if (lml) *lml = std::numeric_limits<double>::quiet_NaN();
        g_err = "Matrix is not positive definite";
        return GPMI_ERR_NOT_PD;
    }
    if (bad_pivot) *bad_pivot = 0;
    // tune_hyperparms_regression.py:312, with y^T alpha = m^T m
    if (lml) *lml = -.5 * red[1] - red[0] - (double)c->N / 2.0 * std::log(2 * M_PI);
    c->res.factor_replaced(tuning().panel_fused);
    c->res.fit_done(Fit::Regression);
    if (with_test) {
        c->ldV = c->ldA;
        c->res.v_in_rows_of_A(with_post, jitter);
        meanvar_to_host(c, h, mu, out2, want_sd);
    }
    return GPMI_OK;
}

// v^T = K_s^T L^-T: right-looking sweep over the block columns of L, with the
// same lookahead split as the Cholesky (the triangular solve of block column
// k+1 overlaps the update of the columns beyond it).
// tri: V starts as the identity (m == Np), so at step k only rows < k + nb are non-zero in
// block column k -- the sweep then costs Np^3/3 and leaves the upper triangular L^-T.
hipError_t solve_sweep(gpmi_ctx* c, double* V, int64_t ldv, int64_t m, bool tri) {
    return solve_sweep_factor(c, c->A.as<double>(), c->ldA, c->Np, V, ldv, m, tri);
}

hipError_t solve_sweep_factor(gpmi_ctx* c, const double* A, int64_t ld, int64_t Np, double* V, int64_t ldv, int64_t m,
                              bool tri) {
    hipError_t e;
    hipStream_t sm = c->stream;
    const int64_t NB = c->block(Np);
    const bool la = c->lookahead_for(Np);
    hipStream_t sp_ = la ? c->pstream : sm;
    // small-LDS panel forms beside the update only for sweeps with enough rows to keep the chip busy: for a few
    // hundred test points the chain of launches is what counts, and the one-launch trsm128 is shorter
    // (N = 16384, n = 1024: 7.96 against 8.47 ms)
    SharingScope shallow(!la ? sharing() : m >= 2048 ? Sharing::beside_update() : sharing().and_chip_shared());
    if (la && (e = c->order(sm, sp_)) != hipSuccess) return e;
    auto update = [&](int64_t c0, int64_t k, int64_t nb, int64_t ncol_upd) -> hipError_t {
        // V[:, c0..c0+ncol_upd) -= V[:, k..k+nb) * L[c0.., k..k+nb)^T
        return launch_gemm_nt(sm, gemm_minus(V + c0, ldv, V + k, ldv, A + c0 * ld + k, ld, tri ? std::min(m, k + nb) : m,
                                             ncol_upd, nb));
    };
    for (int64_t k = 0; k < Np; k += NB) {
        const int64_t nb = std::min<int64_t>(NB, Np - k);
        if ((e = trsm_block(sp_, A + k * ld + k, ld, V + k, ldv, tri ? std::min(m, k + nb) : m, nb)) != hipSuccess) return e;
        if (la && (e = c->order(sp_, sm)) != hipSuccess) return e;
        const int64_t r0 = k + nb;
        if (r0 >= Np) continue;
        if (!la) {
            if ((e = update(r0, k, nb, Np - r0)) != hipSuccess) return e;
            continue;
        }
        const int64_t nbn = std::min<int64_t>(NB, Np - r0);
        if ((e = update(r0, k, nb, nbn)) != hipSuccess) return e;
        if ((e = c->order(sm, sp_)) != hipSuccess) return e;
        if (r0 + nbn < Np && (e = update(r0 + nbn, k, nb, Np - r0 - nbn)) != hipSuccess) return e;
    }
    return hipSuccess;
}

// V = F^-T (upper triangular) for a resident lower factor F (n x n): the sweep on the identity.  Columns >= n of V are
// neither written nor read, here or by any reader of the result.
hipError_t inverse_transposed(gpmi_ctx* c, const double* F, int64_t ldf, int64_t n, double* V, int64_t ldv) {
    hipError_t e = launch_fill_rows(c->stream, V, ldv, n, n, 0.0);
    if (e != hipSuccess) return e;
    if ((e = launch_set_identity_diag(c->stream, V, ldv, n)) != hipSuccess) return e;
    return solve_sweep_factor(c, F, ldf, n, V, ldv, n, true);
}

// Out = -V V^T on the lower tiles for an upper triangular V (n x n, both with leading dimension ld), one launch per row
// block: row block r0 of V is zero left of column r0, so the product starts there
hipError_t neg_gram_lower(gpmi_ctx* c, const double* V, double* Out, int64_t ld, int64_t n) {
    hipError_t e = launch_fill_rows(c->stream, Out, ld, n, n, 0.0);
    const int64_t NB = c->block(n);
    for (int64_t r0 = 0; r0 < n && e == hipSuccess; r0 += NB) {
        const int64_t nb = std::min<int64_t>(NB, n - r0);
        e = launch_gemm_nt(c->stream, gemm_minus_lower(Out + r0 * ld, ld, V + r0 * ld + r0, ld, V + r0, ld, nb, r0 + nb, n - r0, r0));
    }
    return e;
}

// Out -= V V^T on the lower tiles for a dense V: every row block runs over all n columns of V, and nothing is zeroed
// (the softmax gradient adds one such product per class)
hipError_t neg_gram_lower_dense(gpmi_ctx* c, const double* V, double* Out, int64_t ld, int64_t n) {
    hipError_t e = hipSuccess;
    const int64_t NB = c->block(n);
    for (int64_t r0 = 0; r0 < n && e == hipSuccess; r0 += NB) {
        const int64_t nb = std::min<int64_t>(NB, n - r0);
        e = launch_gemm_nt(c->stream, gemm_minus_lower(Out + r0 * ld, ld, V + r0 * ld, ld, V, ld, nb, r0 + nb, n, r0));
    }
    return e;
}

}  // namespace gpmi
