// Gradients of the predictive mean and variance with respect to the test inputs (include/gpmi.h:
// gpmi_predict_grad_resident).  With z = x / r (r: the context's relative lengthscales, 1 when none are set),
// k_j = k(z*, z_j), alpha = K_y^-1 y and w = K_y^-1 k = L^-T v, v = L^-1 k:
//     mu = sum_j alpha_j k_j            dmu/dx*_k  =      sum_j alpha_j D_jk
//     var = sigma^2 - k^T K_y^-1 k      dvar/dx*_k = -2 * sum_j w_j D_jk
//     D_jk = dk_j/dx*_k = -k_j (z*_k - z_jk) / (l^2 r_k)                  squared exponential
//                        = -sigma^2 a^2 H(t_j) (z*_k - z_jk) / r_k         Matern (a, t, H: gpmi_lml_grad)
// The device forms the plain sums over j of alpha_j g_j e_k and w_j g_j e_k (grad.hip: pgrad_kernel; g = k / sigma^2 or
// H); the factors -sigma^2 / (l^2 r_k) (a Matern: -sigma^2 a^2 / r_k) and the -2 are applied here, as grad_ard_scale does.
//
// v is formed exactly as gpmi_predict_resident forms it when it is not resident (and stays), and is reused wherever it
// lies when it is; it is never written.  W = V L^-1 goes to a buffer of the call's own by one of two routes
// (gpmi_pgrad_plan.h): a copy of v swept backwards (panel_mfma.hip: back_sweep_kernel), or U = L^-T by the forward sweep
// on the identity and W = V U^T by the routed GEMM.  With dvar null neither runs.
#include "gpmi_ctx.h"

namespace gpmi {

int predict_grad_impl(gpmi_ctx* c, double* mu, double* var, double* dmu, double* dvar) {
    if (!c->res.regression()) return fail_arg("gpmi_predict_grad: no factorisation resident (call gpmi_factorize)");
    if (!c->res.have_test) return fail_arg("gpmi_predict_grad: no test set (call gpmi_set_test)");
    if (!cov_stationary(c->kind))
        return fail_arg("gpmi_predict_grad: squared-exponential or Matern kernel only (kinds 0, 4, 5, 6)");
    if (c->d > PGRAD_MAXD)
        return fail_arg("gpmi_predict_grad: d must be at most 32 (a test point's 2 d sums are kept in registers)");
    hipStream_t s = c->stream;
    const int64_t n = c->n, np_ = c->np_, N = c->N, Np = c->Np, d = c->d;
    const PgradPlan plan = pgrad_plan(n, Np, c->ldA, c->ld_pad, c->res.factor_fused, dvar != nullptr, c->pgrad_sweep,
                                      c->pgrad_sweep_max);
    c->timers_reset({GPMI_T_ALPHA, GPMI_T_KS, GPMI_T_SOLVE_V, GPMI_T_MEANVAR});
    HIP_TRY(c->vec.ensure((size_t)std::max(Np, np_) * 4 * 8));
    const int ncomp = (int)(dvar ? 2 * d : d);
    const int64_t nch = pgrad_chunks(N);
    HIP_TRY(c->pgpart.ensure((size_t)nch * (size_t)n * ncomp * 8));
    HIP_TRY(c->pgsum.ensure((size_t)n * ncomp * 8));
    if (plan.w_bytes) HIP_TRY(c->pgW.ensure((size_t)plan.w_bytes));
    if (plan.route == PgradRoute::Inverse) HIP_TRY(c->U.ensure((size_t)plan.u_bytes));

    // v: a "predict" event when it is not resident, the steps of predict_resident_impl
    const bool made_v = !c->res.have_v;
    size_t sp;
    if (made_v) {
        int rc = predict_front(c, GPMI_T_KS);
        if (rc) return rc;
        sp = c->span_begin(GPMI_T_SOLVE_V);
        HIP_TRY(solve_sweep(c, c->V.as<double>(), c->ldV, np_));
        c->span_end(sp);
    }
    const double* V = c->v_rows();
    const int64_t ldV = c->ldV;

    // mean and variance: the row dots of gpmi_predict_resident on the same v (the copy is queued before alpha reuses vec)
    std::vector<double> h(2 * (size_t)np_);
    if (mu || var) {
        sp = c->span_begin(GPMI_T_MEANVAR);
        double* dot = c->vec.as<double>();
        HIP_TRY(launch_row_dots(s, V, ldV, np_, Np, c->m_row(), dot, dot + np_));
        c->span_end(sp);
        HIP_TRY(hipMemcpyAsync(h.data(), dot, h.size() * 8, hipMemcpyDeviceToHost, s));
    }

    double* alpha = nullptr;
    sp = c->span_begin(GPMI_T_ALPHA);
    HIP_TRY(backward_solve_resident(c, c->vec.as<double>(), &alpha));
    c->span_end(sp);

    double* W = nullptr;
    double w_sign = 1.0;
    if (plan.route != PgradRoute::None) {
        W = c->pgW.as<double>();
        sp = c->span_begin(GPMI_T_SOLVE_V);
        if (plan.route == PgradRoute::Sweep) {
            // the n rows of v, Np columns each (the identity padding keeps the padded system consistent)
            HIP_TRY(hipMemcpy2DAsync(W, (size_t)plan.ldw * 8, V, (size_t)ldV * 8, (size_t)Np * 8, (size_t)n,
                                     hipMemcpyDeviceToDevice, s));
            HIP_TRY(launch_back_sweep(s, c->A.as<double>(), c->ldA, Np, W, plan.ldw, n));
        } else {
            // W = -V U^T on a zeroed W: the routed GEMM subtracts, the sign goes into the scaling
            HIP_TRY(inverse_transposed(c, c->A.as<double>(), c->ldA, Np, c->U.as<double>(), c->ldA));
            HIP_TRY(launch_fill_rows(s, W, plan.ldw, np_, Np, 0.0));
            HIP_TRY(launch_gemm_nt(s, gemm_minus(W, plan.ldw, V, ldV, c->U.as<double>(), c->ldA, np_, Np, Np)));
            w_sign = -1.0;
        }
        c->span_end(sp);
    }

    std::vector<double> sums;
    if (dmu || dvar) {
        PgradArgs a;
        a.Zs = c->x_test(); a.Z = c->x_train(); a.n = n; a.N = N; a.d = d;
        a.alpha = alpha; a.W = W; a.ldw = plan.ldw;
        a.coef = c->coef; a.family = cov_family(c->kind);
        a.partial = c->pgpart.as<double>(); a.sums = c->pgsum.as<double>();
        sp = c->span_begin(GPMI_T_MEANVAR);
        HIP_TRY(launch_pgrad(s, a));
        c->span_end(sp);
        sums.resize((size_t)n * ncomp);
        HIP_TRY(hipMemcpyAsync(sums.data(), a.sums, sums.size() * 8, hipMemcpyDeviceToHost, s));
    }
    const int rc = solve_epilogue(c, "gpmi_predict_grad");
    if (made_v) c->res.v_computed();           // v is whole whatever the backward solve's word says
    if (rc) return rc;
    if (mu || var) meanvar_to_host(c, h, mu, var, 0);
    // D's factor: -sigma^2 / (l^2 r_k); a Matern kind has a^2 for 1 / l^2
    const double base = -c->sig2 * cov_inv_l2(c->kind, c->ell, c->coef);
    for (int64_t i = 0; i < n && (dmu || dvar); ++i)
        for (int64_t k = 0; k < d; ++k) {
            const double f = base / (c->ard() ? c->ard_r[(size_t)k] : 1.0);
            if (dmu) dmu[i * d + k] = f * sums[(size_t)(i * ncomp + k)];
            if (dvar) dvar[i * d + k] = -2.0 * (w_sign * f) * sums[(size_t)(i * ncomp + d + k)];
        }
    return GPMI_OK;
}

}  // namespace gpmi
