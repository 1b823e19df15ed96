// GP regression behind its fit: what the C-ABI computes from the resident factorisation (driver.hip: factorize_impl) --
// alpha, prediction for a test set, both LML gradients, leave-one-out with its gradient, and the posterior-sample factor.
// The shims of gpmi_api.hip check their pointers, select the device and install the call's options.  Data layout: see
// gpmi_api.hip.
#include "gpmi_ctx.h"

namespace gpmi {

// L^T x = b on the resident fused factor (a5): the first call after a factorisation inverts the 128 x 128 diagonal
// blocks into their upper triangles (one launch, all blocks at once), every call then runs one product per block
hipError_t backward_solve_fused(gpmi_ctx* c, double* b, double* xout) {
    double* A = c->A.as<double>();
    const int mode = tuning().trsv_vinv;
    if (!mode) return launch_trsv_lt_fused(c->stream, A, c->ldA, b, xout, c->Np);
    hipError_t e;
    if (mode >= 2 && (e = c->vside.ensure((size_t)c->Np * 128 * 8)) != hipSuccess) return e;
    if (!c->res.have_vinv || (mode >= 2 && !c->res.have_vside)) {
        e = launch_vinv128(c->stream, A, c->ldA, c->Np, mode >= 2 ? c->vside.as<double>() : nullptr);
        if (e != hipSuccess) return e;
        c->res.block_inverses_made(mode >= 2);
    }
    if (mode >= 2) {
        if ((e = c->flag.ensure(64)) != hipSuccess) return e;
        if ((e = hipMemsetAsync(c->flag.p, 0, 64, c->stream)) != hipSuccess) return e;
        return launch_trsv_lt_chain(c->stream, A, c->ldA, c->vside.as<double>(), b, xout, c->Np, c->flag.as<int>());
    }
    return launch_trsv_lt_vinv(c->stream, A, c->ldA, b, xout, c->Np);
}

hipError_t backward_solve_resident(gpmi_ctx* c, double* x2, double** x_out) {
    // padded tail of m is zero (identity padding), so the padded system stays consistent
    hipError_t e = hipMemcpyAsync(x2, c->m_row(), (size_t)c->Np * 8, hipMemcpyDeviceToDevice, c->stream);
    if (e != hipSuccess) return e;
    return backward_solve_rhs(c, x2, x_out);
}

hipError_t backward_solve_rhs(gpmi_ctx* c, double* x2, double** x_out) {
    *x_out = c->res.factor_fused ? x2 + c->Np : x2;
    if (c->res.factor_fused) return backward_solve_fused(c, x2, x2 + c->Np);
    return launch_trsv_lt(c->stream, c->A.as<double>(), c->ldA, x2, c->Np);
}

int fail_gave_up(const char* api) {
    return fail_runtime(hipErrorUnknown, (std::string(api) + ": the single-launch backward solve gave up waiting for a block").c_str());
}

// The end of a call that ran backward_solve_resident, behind the caller's own device-to-host copies: the read of the
// one-launch solve's "a poll gave up" word where that solve ran, the call's one synchronisation, the timers, and the
// word's status under the caller's API name
int solve_epilogue(gpmi_ctx* c, const char* api) {
    hipStream_t s = c->stream;
    int gave_up = 0;
    if (c->res.factor_fused && tuning().trsv_vinv >= 2)
        HIP_TRY(hipMemcpyAsync(&gave_up, c->flag.p, sizeof(int), hipMemcpyDeviceToHost, s));
    HIP_TRY(hipStreamSynchronize(s));
    c->timers_collect();
    return gave_up ? fail_gave_up(api) : GPMI_OK;
}

// The ending of a lower-tile sums kernel (grad.hip: the ARD and the CO2 sums): the partials' and the sums' buffers, the
// launch, the end of the caller's span, the ncomp x launches sums to the host and the solve epilogue (solve_api null: a
// plain synchronisation)
template <class Args>
static int tile_sums_finish(gpmi_ctx* c, Args& a, hipError_t (*launch)(hipStream_t, const Args&), int64_t ncomp,
                            int64_t launches, size_t span, const char* solve_api, double* sums) {
    hipStream_t s = c->stream;
    HIP_TRY(c->gpart.ensure((size_t)tri_tile_count(a.n) * (size_t)ncomp * 8));
    HIP_TRY(c->gsum.ensure((size_t)launches * (size_t)ncomp * 8));
    a.partial = c->gpart.as<double>();
    a.sums = c->gsum.as<double>();
    HIP_TRY(launch(s, a));
    c->span_end(span);
    HIP_TRY(hipMemcpyAsync(sums, a.sums, (size_t)launches * (size_t)ncomp * 8, hipMemcpyDeviceToHost, s));
    if (solve_api) return solve_epilogue(c, solve_api);
    HIP_TRY(hipStreamSynchronize(s));
    c->timers_collect();
    return GPMI_OK;
}

int grad_ard_finish(gpmi_ctx* c, GradArdArgs& a, size_t span, const char* solve_api, std::vector<double>* sums) {
    const int64_t nl = grad_ard_launches(a), ncomp = grad_ard_width(a) + 3;
    sums->resize((size_t)nl * (size_t)ncomp);
    return tile_sums_finish(c, a, launch_grad_ard, ncomp, nl, span, solve_api, sums->data());
}

// launch q holds sum w K/sigma^2 e_k^2 for its dimensions, then (first launch) the l, sigma and noise sums
void grad_ard_scale(const gpmi_ctx* c, const GradArdArgs& a, const std::vector<double>& sums, double l2, double* d_r,
                    double* d_ell, double* d_sigma, double* d_noise) {
    const int64_t w = grad_ard_width(a);
    if (d_r)
        for (int64_t k = 0; k < c->d; ++k) {
            const double rk = c->ard() ? c->ard_r[(size_t)k] : 1.0;
            d_r[k] = .5 * (c->sig2 * sums[(size_t)((k / w) * (w + 3) + k % w)] / (l2 * rk));
        }
    if (d_ell) *d_ell = .5 * (c->sig2 * sums[(size_t)w] / (l2 * c->ell));
    if (d_sigma) *d_sigma = .5 * (2 * c->sigma * sums[(size_t)w + 1]);
    if (d_noise) *d_noise = .5 * sums[(size_t)w + 2];
}

int alpha_impl(gpmi_ctx* c, double* alpha_out) {
    if (!c->res.regression()) return fail_arg("gpmi_get_alpha: no factorisation resident");
    c->timers_reset({GPMI_T_ALPHA});
    HIP_TRY(c->vec.ensure((size_t)std::max(c->Np, c->np_) * 4 * 8));
    double* x = c->vec.as<double>();
    size_t sp = c->span_begin(GPMI_T_ALPHA);
    HIP_TRY(backward_solve_resident(c, x, &x));
    c->span_end(sp);
    HIP_TRY(hipMemcpyAsync(alpha_out, x, (size_t)c->N * 8, hipMemcpyDeviceToHost, c->stream));
    return solve_epilogue(c, "gpmi_get_alpha");
}

int predict_front(gpmi_ctx* c, int ks_slot) {
    c->res.drop_v();
    c->ldV = c->Np + c->ld_pad;
    HIP_TRY(c->V.ensure((size_t)c->np_ * c->ldV * 8));
    const size_t sp = ks_slot >= 0 ? c->span_begin(ks_slot) : gpmi_ctx::NO_SPAN;
    HIP_TRY(launch_rbf(c->stream, rbf_test_train(c, c->V.as<double>(), c->ldV)));
    c->span_end(sp);
    return GPMI_OK;
}

int predict_resident_impl(gpmi_ctx* c, double* mu, double* out2, int want_sd) {
    if (!c->res.regression()) return fail_arg("gpmi_predict: no factorisation resident (call gpmi_factorize)");
    if (!c->res.have_test) return fail_arg("gpmi_predict: no test set (call gpmi_set_test)");
    hipStream_t s = c->stream;
    c->timers_reset({GPMI_T_KS, GPMI_T_SOLVE_V, GPMI_T_MEANVAR});
    HIP_TRY(c->vec.ensure((size_t)std::max(c->Np, c->np_) * 4 * 8));
    int rc = predict_front(c, GPMI_T_KS);
    if (rc) return rc;
    double* V = c->V.as<double>();

    size_t sp = c->span_begin(GPMI_T_SOLVE_V);
    HIP_TRY(solve_sweep(c, V, c->ldV, c->np_));
    c->span_end(sp);

    sp = c->span_begin(GPMI_T_MEANVAR);
    double* dot = c->vec.as<double>();
    double* sq = dot + c->np_;
    HIP_TRY(launch_row_dots(s, V, c->ldV, c->np_, c->Np, c->m_row(), dot, sq));
    c->span_end(sp);

    std::vector<double> h(2 * (size_t)c->np_);
    HIP_TRY(hipMemcpyAsync(h.data(), dot, h.size() * 8, hipMemcpyDeviceToHost, s));
    HIP_TRY(hipStreamSynchronize(s));
    c->timers_collect();
    c->res.v_computed();
    meanvar_to_host(c, h, mu, out2, want_sd);
    return GPMI_OK;
}

// The front of both LML gradients and of the leave-one-out calls: the resident factorisation and -- rbf_only not null --
// its kernel (kinds 0, 4, 5, 6: the stationary ones the gradient kernels have a family for) checked with the caller's own texts, the slot's timer reset, and inside a span of that slot, which it opens:
// alpha = L^-T m (a5; solve_epilogue reads the backward solve's give-up word), U = L^-T by the TRSM sweep on the identity
// and -- want_kn -- Kn = -U U^T on the lower tiles.  Everything behind the two checks is factor_inverse_front, which the
// binary classifier's gradient (laplace.hip) runs on its own factor without the backward solve.
static int grad_front(gpmi_ctx* c, const char* not_resident, const char* rbf_only, int slot, bool want_kn, double** alpha_out,
                      size_t* span) {
    if (!c->res.regression()) return fail_arg(not_resident);
    if (rbf_only && !cov_stationary(c->kind)) return fail_arg(rbf_only);
    return factor_inverse_front(c, slot, want_kn, alpha_out, span);
}

int factor_inverse_front(gpmi_ctx* c, int slot, bool want_kn, double** alpha_out, size_t* span) {
    c->timers_reset({slot});
    const int64_t Np = c->Np, ld = c->ldA;
    HIP_TRY(c->U.ensure((size_t)Np * ld * 8));
    if (want_kn) HIP_TRY(c->Kn.ensure((size_t)Np * ld * 8));
    HIP_TRY(c->vec.ensure((size_t)std::max(c->Np, c->np_) * 4 * 8));
    *span = c->span_begin(slot);
    if (alpha_out) HIP_TRY(backward_solve_resident(c, c->vec.as<double>(), alpha_out));
    HIP_TRY(inverse_transposed(c, c->A.as<double>(), ld, Np, c->U.as<double>(), ld));
    if (want_kn) HIP_TRY(neg_gram_lower(c, c->U.as<double>(), c->Kn.as<double>(), ld, Np));
    return GPMI_OK;
}

// f2 -- gradient of the log marginal likelihood at the resident factorisation:
// 0.5 * tr((alpha alpha^T - K_y^-1) dK/dtheta)  (tune_hyperparms_regression.py:43-57; the reference
// builds K_y^-1 = inv(L.T) inv(L) at :144 and two N x N products).  Here: U = L^-T by the TRSM
// sweep on the identity (N^3/3), -K_y^-1 = -U U^T by one MFMA GEMM per row block over the
// non-zero column range (N^3/3), then one fused pass for the trace (grad.hip).
int lml_grad_impl(gpmi_ctx* c, double* d_ell, double* d_sigma) {
    double* alpha = nullptr;
    size_t sp = 0;
    int rc = grad_front(c, "gpmi_lml_grad: no factorisation resident (call gpmi_factorize)",
                        "gpmi_lml_grad: squared-exponential or Matern kernel only (kinds 0, 4, 5, 6)", GPMI_T_GRAD, true,
                        &alpha, &sp);
    if (rc) return rc;
    hipStream_t s = c->stream;
    GradArgs a;
    a.A = a.B = c->x_train(); a.nA = a.nB = c->N; a.d = c->d;
    a.row0 = 0; a.nrows = c->N;
    a.alpha_r = a.alpha_c = alpha;
    a.Kinv = c->Kn.as<double>(); a.ld = c->ldA; a.kinv_sign = -1.0;
    a.coef = c->coef; a.sig2 = c->sig2; a.two_sigma = 2 * c->sigma;
    a.family = cov_family(c->kind);
    // dK/dl = K sq / l^3; a Matern: sigma^2 H sq a^2 / l
    a.inv_l3 = a.family ? cov_inv_l2(c->kind, c->ell, c->coef) / c->ell : 1.0 / (c->ell * c->ell * c->ell);
    a.tri = 1;
    const int64_t nblk = grad_trace_blocks(a);
    HIP_TRY(c->gpart.ensure((size_t)nblk * 16));
    a.partial = c->gpart.as<double>();
    HIP_TRY(launch_grad_trace(s, a));
    c->span_end(sp);
    std::vector<double> part((size_t)nblk * 2);
    HIP_TRY(hipMemcpyAsync(part.data(), a.partial, part.size() * 8, hipMemcpyDeviceToHost, s));
    if ((rc = solve_epilogue(c, "gpmi_lml_grad"))) return rc;
    double sl = 0.0, ss = 0.0;
    for (int64_t b = 0; b < nblk; ++b) { sl += part[2 * b]; ss += part[2 * b + 1]; }   // fixed order
    *d_ell = .5 * sl;
    *d_sigma = .5 * ss;
    return GPMI_OK;
}

// The gradient with one lengthscale per input dimension, the output scale and the noise: d + 3 traces of the same
// W = alpha alpha^T - K_y^-1 in one fused pass (grad.hip, the ARD kernel).  alpha, U and -K_y^-1 are formed exactly as in
// lml_grad_impl; the per-block partials are summed on the device in a fixed order (at N = 65536 they are tens of MB).
int lml_grad_ard_impl(gpmi_ctx* c, double* d_r, double* d_ell, double* d_sigma, double* d_noise) {
    double* alpha = nullptr;
    size_t sp = 0;
    int rc = grad_front(c, "gpmi_lml_grad_ard: no factorisation resident (call gpmi_factorize)",
                        "gpmi_lml_grad_ard: squared-exponential or Matern kernel only (kinds 0, 4, 5, 6)", GPMI_T_GRAD, true, &alpha, &sp);
    if (rc) return rc;
    GradArdArgs a;
    a.Z = c->x_train(); a.n = c->N; a.d = c->d;
    a.alpha = alpha; a.Kn = c->Kn.as<double>(); a.ld = c->ldA; a.coef = c->coef;
    a.family = cov_family(c->kind);
    std::vector<double> sums;
    if ((rc = grad_ard_finish(c, a, sp, "gpmi_lml_grad_ard", &sums))) return rc;
    // a Matern kind has H(t) for K/sigma^2 in the lengthscale sums and a^2 for 1 / l^2
    const double l2 = a.family ? 1.0 / cov_inv_l2(c->kind, c->ell, c->coef) : c->ell * c->ell;
    grad_ard_scale(c, a, sums, l2, d_r, d_ell, d_sigma, d_noise);
    return GPMI_OK;
}

// The gradient of the CO2 composite kernel (kind 3; GPML section 5.4.3): the 11 hyper-parameters and the noise variance
// from eleven basis sums of the same W in one fused pass (grad.hip: grad_co2_kernel).  alpha, U and -K_y^-1 are formed
// exactly as in lml_grad_impl.  With K = theta_1^2 e1 + theta_3^2 q2 + theta_6^2 p3 + theta_9^2 e4 + theta_11^2 delta and
// g_m = .5 sum_ij W_ij dK_ij/dtheta_m the per-element constants are formed here in double and the sums scaled here.
int lml_grad_co2_impl(gpmi_ctx* c, double* d_theta, double* d_noise) {
    if (c->res.regression() && c->kind != 3)
        return fail_arg("gpmi_lml_grad_co2: CO2 composite kernel only (kind 3; gpmi_set_kernel_params)");
    double* alpha = nullptr;
    size_t sp = 0;
    int rc = grad_front(c, "gpmi_lml_grad_co2: no regression factorisation resident (call gpmi_factorize)",
                        nullptr /* the kind is checked above */, GPMI_T_GRAD, true, &alpha, &sp);
    if (rc) return rc;
    const double* th = c->kpv;             // th[i] = theta_(i+1)
    GradCo2Args a;
    a.Z = c->x_train(); a.n = c->N; a.d = c->d;
    a.alpha = alpha; a.Kn = c->Kn.as<double>(); a.ld = c->ldA;
    a.n1 = -1.0 / (2.0 * th[1] * th[1]);
    a.n4 = -1.0 / (2.0 * th[3] * th[3]);
    a.n5 = -2.0 / (th[4] * th[4]);
    a.cu = 1.0 / (2.0 * th[7] * (th[6] * th[6]));
    a.n8 = -th[7];
    a.n10 = -1.0 / (2.0 * th[9] * th[9]);
    double S[11];
    if ((rc = tile_sums_finish(c, a, launch_grad_co2, 11, 1, sp, "gpmi_lml_grad_co2", S))) return rc;
    if (d_theta) {
        d_theta[0] = th[0] * S[0];
        d_theta[1] = .5 * (th[0] * th[0]) * S[1] / (th[1] * th[1] * th[1]);
        d_theta[2] = th[2] * S[2];
        d_theta[3] = .5 * (th[2] * th[2]) * S[3] / (th[3] * th[3] * th[3]);
        d_theta[4] = 2.0 * (th[2] * th[2]) * S[4] / (th[4] * th[4] * th[4]);
        d_theta[5] = th[5] * S[5];
        d_theta[6] = .5 * (th[5] * th[5]) * S[6] / (th[6] * th[6] * th[6]);
        d_theta[7] = .5 * (th[5] * th[5]) * S[7];
        d_theta[8] = th[8] * S[8];
        d_theta[9] = .5 * (th[8] * th[8]) * S[9] / (th[9] * th[9] * th[9]);
        d_theta[10] = th[10] * S[10];
    }
    if (d_noise) *d_noise = .5 * S[10];
    return GPMI_OK;
}

// Leave-one-out cross-validation at the resident factorisation (GPML section 5.4.2, eqs. 5.10-5.12): with alpha =
// K_y^-1 y and kappa_i = [K_y^-1]_ii the prediction of y_i from the other N - 1 points is N(y_i - alpha_i / kappa_i,
// 1 / kappa_i).  alpha and U = L^-T as in lml_grad_impl; kappa_i is the squared norm of row i of U (K_y^-1 = U U^T), so
// the N^3/3 product -U U^T of the gradients is not needed.  Reads L, m and y only: every kernel kind.
int loo_impl(gpmi_ctx* c, double* mu, double* var, double* logp, double* loo) {
    double* alpha = nullptr;
    size_t sp = 0;
    int rc = grad_front(c, "gpmi_loo: no regression factorisation resident (call gpmi_factorize)", nullptr, GPMI_T_LOO, false,
                        &alpha, &sp);
    if (rc) return rc;
    hipStream_t s = c->stream;
    const int64_t N = c->N, Np = c->Np;
    HIP_TRY(c->loov.ensure((size_t)(4 * Np + 8) * 8));
    double* kappa = c->loov.as<double>();
    double *dmu = kappa + Np, *dvar = dmu + Np, *dlogp = dvar + Np, *dsum = dlogp + Np;
    HIP_TRY(launch_loo_kappa(s, c->U.as<double>(), c->ldA, N, kappa));
    HIP_TRY(launch_loo_points(s, c->y.as<double>(), alpha, kappa, N, dmu, dvar, dlogp, dsum));
    c->span_end(sp);
    if (mu) HIP_TRY(hipMemcpyAsync(mu, dmu, (size_t)N * 8, hipMemcpyDeviceToHost, s));
    if (var) HIP_TRY(hipMemcpyAsync(var, dvar, (size_t)N * 8, hipMemcpyDeviceToHost, s));
    if (logp) HIP_TRY(hipMemcpyAsync(logp, dlogp, (size_t)N * 8, hipMemcpyDeviceToHost, s));
    double sum = 0.0;
    HIP_TRY(hipMemcpyAsync(&sum, dsum, 8, hipMemcpyDeviceToHost, s));
    if ((rc = solve_epilogue(c, "gpmi_loo"))) return rc;
    if (loo) *loo = sum;
    return GPMI_OK;
}

// The derivatives of the leave-one-out log probability (GPML eq. 5.13) w.r.t. l, sigma and the noise variance:
//   sum_i (alpha_i r_i - .5 (1 + alpha_i^2 / kappa_i) s_i) / kappa_i,   r = Z alpha,  s_i = [Z K_y^-1]_ii,  Z = K_y^-1 dK_y
// alpha, U and Kn = -K_y^-1 as in lml_grad_impl; kappa from U as in loo_impl; Kn mirrored into a full matrix; D = K o sq
// (dK/dl = D / l^3) built in full into U's buffer, which is dead by then; one pass over the rows of D for t = D alpha and
// one over the rows of Kn for c_i = sum_a Kn_ia^2, Kn alpha and Kn t; then K_y^-1 D one row block at a time (the routed
// GEMM into an NB x ld workspace, 2 N^3 flops in all) with s_i read off each block by a row dot with Kn -- the product is
// never stored whole.  sigma and the noise need no N^3 product (dK_y = 2 (K_y - noise I) / sigma and I).
int loo_grad_impl(gpmi_ctx* c, double* d_ell, double* d_sigma, double* d_noise) {
    double* alpha = nullptr;
    size_t sp = 0;
    int rc = grad_front(c, "gpmi_loo_grad: no regression factorisation resident (call gpmi_factorize)",
                        "gpmi_loo_grad: squared-exponential or Matern kernel only (kinds 0, 4, 5, 6)", GPMI_T_LOO, true, &alpha, &sp);
    if (rc) return rc;
    hipStream_t s = c->stream;
    const int64_t N = c->N, Np = c->Np, ld = c->ldA;
    const int64_t NB = std::min<int64_t>(c->block(Np), Np);
    HIP_TRY(c->loov.ensure((size_t)(6 * Np + 8) * 8));
    HIP_TRY(c->loow.ensure((size_t)NB * ld * 8));
    double* kappa = c->loov.as<double>();
    double *cn = kappa + Np, *qn = cn + Np, *un = qn + Np, *t = un + Np, *sn = t + Np, *sums = sn + Np;
    double *D = c->U.as<double>(), *Kn = c->Kn.as<double>(), *W = c->loow.as<double>();
    HIP_TRY(launch_loo_kappa(s, D, ld, N, kappa));               // U is still L^-T here
    HIP_TRY(launch_mirror_lower(s, Kn, ld, Np));
    HIP_TRY(launch_loo_dmat(s, c->x_train(), N, c->d, c->coef, c->sig2, cov_family(c->kind), D, ld, Np));
    HIP_TRY(launch_row_pass(s, D, ld, N, alpha, nullptr, nullptr, t, nullptr));
    HIP_TRY(launch_row_pass(s, Kn, ld, N, alpha, t, cn, qn, un));
    for (int64_t r0 = 0; r0 < N; r0 += NB) {                     // a row block of padding only has nothing to give
        const int64_t nb = std::min<int64_t>(NB, Np - r0);
        HIP_TRY(launch_fill_rows(s, W, ld, nb, Np, 0.0));
        // W = -Kn[r0 .. r0 + nb) D^T = (K_y^-1 D) rows; D is symmetric
        HIP_TRY(launch_gemm_nt(s, gemm_minus(W, ld, Kn + r0 * ld, ld, D, ld, nb, Np, Np)));
        HIP_TRY(launch_row_dot2(s, W, ld, Kn + r0 * ld, ld, std::min<int64_t>(nb, N - r0), N, sn + r0));
    }
    LooGradArgs a;
    a.alpha = alpha; a.kappa = kappa; a.cn = cn; a.qn = qn; a.un = un; a.sn = sn;
    a.n = N; a.noise = c->noise; a.out3 = sums;
    HIP_TRY(launch_loo_grad_sums(s, a));
    c->span_end(sp);
    double h[3] = {0.0, 0.0, 0.0};
    HIP_TRY(hipMemcpyAsync(h, sums, sizeof h, hipMemcpyDeviceToHost, s));
    if ((rc = solve_epilogue(c, "gpmi_loo_grad"))) return rc;
    if (d_ell) *d_ell = cov_family(c->kind) ? h[0] * (cov_inv_l2(c->kind, c->ell, c->coef) / c->ell)      // dK/dl = a^2 D / l
                                            : h[0] / (c->ell * c->ell * c->ell);
    if (d_sigma) *d_sigma = 2.0 / c->sigma * h[1];
    if (d_noise) *d_noise = h[2];
    return GPMI_OK;
}

// The same trace from caller-supplied alpha and K_y^-1 (host, N x N row-major): the arguments the
// reference's gradient_ascent(a, b, sigma, l, alpha, K_y) receives (tune_hyperparms_regression.py:31).
int grad_trace_impl(gpmi_ctx* c, const double* a_in, const double* b_in, int64_t N, int64_t d, double sigma, double ell,
                    const double* alpha_in, const double* Kinv_in, double* d_ell, double* d_sigma) {
    if (N <= 0 || d <= 0) return fail_arg("gpmi_grad_trace: N and d must be positive");
    if (cov_family(c->kind)) return fail_arg("gpmi_grad_trace: squared-exponential kernel only (the context is set to a Matern kind)");
    if (!(ell != 0.0)) return fail_arg("gpmi_grad_trace: ell must be non-zero");
    hipStream_t s = c->stream;
    DevBuf da, db, dal, dk, dp;
    const int64_t chunk = std::max<int64_t>(TILE, std::min<int64_t>(round_up(N, TILE), ((int64_t)1 << 30) / (N * 8) / TILE * TILE));
    int rc = GPMI_OK;
    hipError_t e = hipSuccess;
    double sl = 0.0, ss = 0.0;
    do {
        if ((e = da.ensure((size_t)N * d * 8)) != hipSuccess || (e = db.ensure((size_t)N * d * 8)) != hipSuccess ||
            (e = dal.ensure((size_t)N * 8)) != hipSuccess || (e = dk.ensure((size_t)chunk * N * 8)) != hipSuccess) {
            rc = fail_runtime(e, "hipMalloc"); break;
        }
        if ((e = hipMemcpyAsync(da.p, a_in, (size_t)N * d * 8, hipMemcpyHostToDevice, s)) != hipSuccess ||
            (e = hipMemcpyAsync(db.p, b_in, (size_t)N * d * 8, hipMemcpyHostToDevice, s)) != hipSuccess ||
            (e = hipMemcpyAsync(dal.p, alpha_in, (size_t)N * 8, hipMemcpyHostToDevice, s)) != hipSuccess) {
            rc = fail_runtime(e, "hipMemcpy H2D"); break;
        }
        for (int64_t r0 = 0; r0 < N && rc == GPMI_OK; r0 += chunk) {
            const int64_t rows = std::min(chunk, N - r0);
            if ((e = hipMemcpyAsync(dk.p, Kinv_in + r0 * N, (size_t)rows * N * 8, hipMemcpyHostToDevice, s)) != hipSuccess) {
                rc = fail_runtime(e, "hipMemcpy H2D"); break;
            }
            GradArgs g;
            g.A = da.as<double>(); g.B = db.as<double>(); g.nA = g.nB = N; g.d = d;
            g.row0 = r0; g.nrows = rows;
            g.alpha_r = g.alpha_c = dal.as<double>();
            g.Kinv = dk.as<double>(); g.ld = N; g.kinv_sign = 1.0;
            g.coef = -.5 * (1 / (ell * ell)); g.sig2 = sigma * sigma; g.two_sigma = 2 * sigma;
            g.inv_l3 = 1.0 / (ell * ell * ell);
            g.tri = 0;
            const int64_t nblk = grad_trace_blocks(g);
            if ((e = dp.ensure((size_t)nblk * 16)) != hipSuccess) { rc = fail_runtime(e, "hipMalloc"); break; }
            g.partial = dp.as<double>();
            std::vector<double> part((size_t)nblk * 2);
            if ((e = launch_grad_trace(s, g)) != hipSuccess ||
                (e = hipMemcpyAsync(part.data(), g.partial, part.size() * 8, hipMemcpyDeviceToHost, s)) != hipSuccess ||
                (e = hipStreamSynchronize(s)) != hipSuccess) {
                rc = fail_runtime(e, "gradient trace"); break;
            }
            for (int64_t b = 0; b < nblk; ++b) { sl += part[2 * b]; ss += part[2 * b + 1]; }
        }
    } while (0);
    (void)hipStreamSynchronize(s);
    da.release(); db.release(); dal.release(); dk.release(); dp.release();
    if (rc == GPMI_OK) { *d_ell = .5 * sl; *d_sigma = .5 * ss; }
    return rc;
}

// the posterior-sample factor on the device: where cholesky(K_ss + jitter I - v^T v) of the resident test set sits (factor, ld)
// -- behind L when it rode through the augmented factorisation (gpmi_fit_predict_sample_resident), else formed now in P
// (K_ss build, v^T v by one MFMA SYRK, the same Cholesky) unless P already holds it for this jitter
static int post_factor_device(gpmi_ctx* c, double jitter, const double** factor, int64_t* ld, int64_t* bad_pivot) {
    if (!c->res.have_v) return fail_arg("gpmi_post_chol: run gpmi_predict first");
    hipStream_t s = c->stream;
    const int64_t np_ = c->np_, n = c->n;
    if (bad_pivot) *bad_pivot = 0;
    if (c->res.post_rides(jitter)) {
        *factor = c->A.as<double>() + c->Np * c->ldA + c->Np;
        *ld = c->ldA;
        return GPMI_OK;
    }
    if (c->res.post_cached(jitter)) {
        *factor = c->P.as<double>();
        *ld = c->ldP;
        return GPMI_OK;
    }
    c->res.drop_post_in_P();
    c->timers_reset({GPMI_T_POSTCHOL});
    c->ldP = np_ + 32;
    HIP_TRY(c->P.ensure((size_t)np_ * c->ldP * 8));
    double* P = c->P.as<double>();
    const int64_t big = std::numeric_limits<int64_t>::max();
    HIP_TRY(hipMemcpyAsync(c->info.p, &big, sizeof big, hipMemcpyHostToDevice, s));
    size_t sp = c->span_begin(GPMI_T_POSTCHOL);
    // K_ss + jitter*I, lower tiles (GP_regression.py:128,154)
    const RbfArgs r = rbf_sym(c, c->x_test(), n, c->box_test(), jitter, np_, P, c->ldP);
    HIP_TRY(launch_rbf(s, r));
    // P -= v^T v  (rows of V are the columns of v)
    HIP_TRY(launch_gemm_nt(s, gemm_minus_lower(P, c->ldP, c->v_rows(), c->ldV, c->v_rows(), c->ldV, np_, np_, c->Np, 0)));
    HIP_TRY(cholesky_inplace(c, P, c->ldP, np_, np_, c->info.as<int64_t>(), false));
    c->span_end(sp);
    int64_t info;
    HIP_TRY(hipMemcpyAsync(&info, c->info.p, sizeof info, hipMemcpyDeviceToHost, s));
    HIP_TRY(hipStreamSynchronize(s));
    c->timers_collect();
    if (info != big && info < n) {
        if (bad_pivot) *bad_pivot = info + 1;
        g_err = "Matrix is not positive definite";
        return GPMI_ERR_NOT_PD;
    }
    c->res.post_cached_in_P(jitter);
    *factor = P;
    *ld = c->ldP;
    return GPMI_OK;
}

int post_chol_impl(gpmi_ctx* c, double jitter, double* L_out, int64_t* bad_pivot) {
    const double* F = nullptr;
    int64_t ld = 0;
    int rc = post_factor_device(c, jitter, &F, &ld, bad_pivot);
    if (rc) return rc;
    hipStream_t s = c->stream;
    const int64_t n = c->n;
    HIP_TRY(c->dense.ensure((size_t)n * n * 8));
    HIP_TRY(launch_extract(s, F, ld, 0, n, 0, n, c->dense.as<double>(), 1));
    HIP_TRY(hipMemcpyAsync(L_out, c->dense.p, (size_t)n * n * 8, hipMemcpyDeviceToHost, s));
    HIP_TRY(hipStreamSynchronize(s));
    return GPMI_OK;
}

// L_ @ Z for the posterior samples f_post = mu + L_ @ normals (GP_regression.py:155) without bringing L_ to the host: Z
// (n x num_fun row-major, the caller's normals -- drawn on the host so that np.random's order is the reference's) goes up,
// the product comes down.  The factor is the one post_chol_impl(jitter) would return.
int post_sample_impl(gpmi_ctx* c, double jitter, const double* Z, int64_t num_fun, double* LZ_out, int64_t* bad_pivot) {
    if (num_fun <= 0 || num_fun > (1 << 20)) return fail_arg("gpmi_post_sample: num_fun must be in 1 .. 2^20");
    const double* F = nullptr;
    int64_t ld = 0;
    int rc = post_factor_device(c, jitter, &F, &ld, bad_pivot);
    if (rc) return rc;
    hipStream_t s = c->stream;
    const int64_t n = c->n;
    const size_t bytes = (size_t)n * (size_t)num_fun * 8;
    HIP_TRY(c->dense.ensure(2 * bytes));
    double* Zd = c->dense.as<double>();
    double* Od = Zd + (size_t)n * (size_t)num_fun;
    HIP_TRY(hipMemcpyAsync(Zd, Z, bytes, hipMemcpyHostToDevice, s));
    HIP_TRY(launch_tri_mul(s, F, ld, Zd, n, num_fun, Od));
    HIP_TRY(hipMemcpyAsync(LZ_out, Od, bytes, hipMemcpyDeviceToHost, s));
    HIP_TRY(hipStreamSynchronize(s));
    return GPMI_OK;
}

}  // namespace gpmi
