// gpmi_append: k more observations into the resident regression factorisation in O(N^2 k) -- one border of the factor
// instead of a new fit.  The plan (what is the border, which route, in place or not, whether the y row moves) is
// append_plan of gpmi_append_plan.h; this file carries it out with the pieces a fit is made of: the row builds of K, the
// TRSM sweep (or, for k <= 16, the border-sweep kernel of panel_mfma.hip), one rank-N0 update, cholesky_inplace with the
// y row carried, and the LML reduction.
#include "gpmi_append_plan.h"
#include "gpmi_ctx.h"

namespace gpmi {

namespace {

// a device buffer that keeps its first `used` bytes when it has to grow (DevBuf::ensure drops them)
hipError_t grow_keep(DevBuf& b, size_t used, size_t bytes) {
    if (bytes <= b.cap) return hipSuccess;
    // twice the old size at least: a loop that appends one point at a time reallocates O(log) times
    void* p = nullptr;
    size_t cap = std::max(bytes, 2 * b.cap);
    hipError_t e = hipMalloc(&p, cap);
    if (e != hipSuccess && cap > bytes) {
        (void)hipGetLastError();
        cap = bytes;
        e = hipMalloc(&p, cap);
    }
    if (e != hipSuccess) return e;
    if (b.p && used) {
        e = hipMemcpy(p, b.p, used, hipMemcpyDeviceToDevice);
        if (e != hipSuccess) { (void)hipFree(p); return e; }
    }
    b.release();
    b.p = p;
    b.cap = cap;
    return hipSuccess;
}

struct ReleaseOnExit {         // the new A until the context owns it
    DevBuf& b;
    ~ReleaseOnExit() { b.release(); }
};

}  // namespace

int append_impl(gpmi_ctx* c, const double* Xnew, int64_t k, const double* ynew, double* lml, int64_t* bad_pivot) {
    if (!c->res.regression()) return fail_arg("gpmi_append: no factorisation resident");
    if (!Xnew || !ynew) return fail_arg("gpmi_append: null argument");
    if (k < 1) return fail_arg("gpmi_append: k must be at least 1");
    if (c->kind == 3)
        return fail_arg("gpmi_append: the composite kernel (kind 3) is not supported: its delta term belongs to a square matrix");
    const int64_t d = c->d, N = c->N;
    for (int64_t i = 0; i < k * d; ++i)
        if (std::isnan(Xnew[i])) return fail_arg("gpmi_append: Xnew holds NaN");
    for (int64_t i = 0; i < k; ++i)
        if (std::isnan(ynew[i])) return fail_arg("gpmi_append: ynew holds NaN");

    const int fused = c->res.factor_fused;
    const AppendPlan p = append_plan(N, k, c->ldA, c->rows_cap, c->yrow, c->ld_pad, c->reserve, fused, c->append_skinny);
    const int64_t N0 = p.N0, N1 = p.N1, Np1 = p.Np1;
    hipStream_t s = c->stream;

    // ---- everything that can fail for want of memory, before anything of the resident fit changes
    DevBuf Anew;
    ReleaseOnExit anew_guard{Anew};
    if (!p.in_place) {
        const hipError_t e = Anew.ensure((size_t)p.rows * p.ld * sizeof(double));
        if (e != hipSuccess) {
            (void)hipGetLastError();
            return fail_runtime(e, "gpmi_append: the larger factor");
        }
    }
    const int64_t lds = N0 + 32;                            // leading dimension of the skinny route's rows of K
    hipError_t e = hipSuccess;
    if (p.skinny) e = c->app.ensure((size_t)(round_up(k * d, 2) + TILE * lds) * 8);
    if (e == hipSuccess) e = grow_keep(c->X, (size_t)N * d * 8, (size_t)N1 * d * 8);
    if (e == hipSuccess) e = grow_keep(c->y, (size_t)N * 8, (size_t)N1 * 8);
    if (e == hipSuccess && c->ard()) e = grow_keep(c->Xz, (size_t)N * d * 8, (size_t)N1 * d * 8);
    if (e != hipSuccess) {
        (void)hipGetLastError();
        return fail_runtime(e, "gpmi_append: workspace");
    }

    // ---- inputs: X, y, the boxes, the scaled copy; the lanes' copies of the training set are stale.  From here on a
    // failure (a runtime error as much as a failed pivot) leaves no fit and the extended training set, N = N + k at
    // once: gpmi_factorize lays A out anew from N alone, so a half-made layout does no harm.  Success puts the resident
    // state back, extended.
    c->N = N1;
    const Resident before = c->res;
    c->res.drop_fit();
    c->timers_reset({GPMI_T_KS, GPMI_T_SOLVE_V, GPMI_T_CHOL, GPMI_T_LML});
    HIP_TRY(hipMemcpyAsync(c->X.as<double>() + N * d, Xnew, (size_t)k * d * 8, hipMemcpyHostToDevice, s));
    HIP_TRY(hipMemcpyAsync(c->y.as<double>() + N, ynew, (size_t)k * 8, hipMemcpyHostToDevice, s));
    c->boxX.extend(Xnew, k, d);           // a stale box would let the K build skip an exp domain test it needs
    if (c->ard()) {
        HIP_TRY(launch_scale_inputs(s, c->X.as<double>() + N * d, c->ard_rdev.as<double>(), k, d, c->Xz.as<double>() + N * d));
        box_scale(c->boxX, c->ard_r, c->boxZ);
    }
    for (gpmi_ctx* l : c->lane_ctx) l->res.drop_train();

    // ---- storage
    double* Aold = c->A.as<double>();
    const int64_t ld_old = c->ldA, yrow_old = c->yrow;
    double* A = p.in_place ? Aold : Anew.as<double>();
    const int64_t ld = p.ld;
    double* yr = A + p.yrow * ld;
    if (!p.in_place) {
        if (N0 > 0)
            HIP_TRY(hipMemcpy2DAsync(A, (size_t)ld * 8, Aold, (size_t)ld_old * 8, (size_t)N0 * 8, (size_t)p.keep_rows,
                                     hipMemcpyDeviceToDevice, s));
    }
    if (p.yrow_moves || !p.in_place) {
        // the y block's new place first, while the old row is whole: the border rows land where it used to be
        HIP_TRY(launch_fill_rows(s, yr, ld, TILE, Np1, 0.0));
        if (N0 > 0)
            HIP_TRY(hipMemcpyAsync(yr, Aold + yrow_old * ld_old, (size_t)N0 * 8, hipMemcpyDeviceToDevice, s));
    } else {
        HIP_TRY(launch_fill_rows(s, yr + N0, ld, 1, Np1 - N0, 0.0));
    }
    // raw y over the border's columns (zeros beyond N1 are there)
    HIP_TRY(hipMemcpyAsync(yr + N0, c->y.as<double>() + N0, (size_t)(N1 - N0) * 8, hipMemcpyDeviceToDevice, s));
    if (!p.in_place) {
        // the old buffer goes once the copies out of it have run; from here on the context describes the new one
        HIP_TRY(hipStreamSynchronize(s));
        c->A.release();
        c->A = Anew;
        Anew = DevBuf();
    }
    c->Np = Np1; c->ldA = ld; c->Mp = Np1 + TILE; c->rows_cap = p.rows; c->yrow = p.yrow;
    const int64_t big = std::numeric_limits<int64_t>::max();
    HIP_TRY(hipMemcpyAsync(c->info.p, &big, sizeof big, hipMemcpyHostToDevice, s));

    // ---- W = K(border, X[0:N0]) L0^-T
    const double* Xt = c->x_train();
    c->append_route = p.skinny ? 1 : 0;
    if (N0 > 0) {
        if (p.skinny) {
            double* xn = c->app.as<double>();
            double* Ks = xn + round_up(k * d, 2);
            size_t sp = c->span_begin(GPMI_T_KS);
            HIP_TRY(hipMemcpyAsync(xn, Xt + N * d, (size_t)k * d * 8, hipMemcpyDeviceToDevice, s));
            HIP_TRY(launch_rbf(s, rbf_cross(c, xn, k, c->box_train(), Xt, N0, c->box_train(), 0, TILE, N0, Ks, lds)));
            c->span_end(sp);
            sp = c->span_begin(GPMI_T_SOLVE_V);
            HIP_TRY(launch_border_sweep(s, A, ld, N0, Ks, lds, k));
            HIP_TRY(hipMemcpy2DAsync(A + N * ld, (size_t)ld * 8, Ks, (size_t)lds * 8, (size_t)N0 * 8, (size_t)k,
                                     hipMemcpyDeviceToDevice, s));
            // the padding rows below the new points (the old tail rows [N0, N) are final and stay)
            HIP_TRY(launch_fill_rows(s, A + N1 * ld, ld, Np1 - N1, N0, 0.0));
            c->span_end(sp);
        } else {
            size_t sp = c->span_begin(GPMI_T_KS);
            HIP_TRY(launch_rbf(s, rbf_cross(c, Xt, N1, c->box_train(), Xt, N0, c->box_train(), N0, p.border, N0, A + N0 * ld, ld)));
            c->span_end(sp);
            sp = c->span_begin(GPMI_T_SOLVE_V);
            HIP_TRY(solve_sweep_factor(c, A, ld, N0, A + N0 * ld, ld, p.border));
            c->span_end(sp);
        }
    }

    // ---- the border block: K_bb + noise I (lower tiles, identity padding), minus W W^T with the y row, factored
    size_t sp = c->span_begin(GPMI_T_KS);
    double* Abb = A + N0 * ld + N0;
    HIP_TRY(launch_rbf(s, rbf_sym(c, Xt + N0 * d, N1 - N0, c->box_train(), c->noise, p.border, Abb, ld)));
    c->span_end(sp);
    sp = c->span_begin(GPMI_T_CHOL);
    if (N0 > 0)
        HIP_TRY(launch_gemm_nt(s, gemm_minus_lower(Abb, ld, A + N0 * ld, ld, A + N0 * ld, ld, p.border + TILE, p.border, N0, 0)));
    HIP_TRY(cholesky_inplace(c, Abb, ld, p.border, p.border + TILE, c->info.as<int64_t>(), false));
    c->span_end(sp);

    sp = c->span_begin(GPMI_T_LML);
    HIP_TRY(launch_lml_reduce(s, A, ld, yr, N1, c->red.as<double>()));
    c->span_end(sp);
    double red[2];
    int64_t info;
    HIP_TRY(hipMemcpyAsync(red, c->red.p, sizeof red, hipMemcpyDeviceToHost, s));
    HIP_TRY(hipMemcpyAsync(&info, c->info.p, sizeof info, hipMemcpyDeviceToHost, s));
    HIP_TRY(hipStreamSynchronize(s));
    c->timers_collect();
    if (info != big && info < N1 - N0) {
        if (bad_pivot) *bad_pivot = N0 + info + 1;
        if (lml) *lml = std::numeric_limits<double>::quiet_NaN();
        g_err = "Matrix is not positive definite";
        return GPMI_ERR_NOT_PD;
    }
    if (bad_pivot) *bad_pivot = 0;
    if (lml) *lml = -.5 * red[1] - red[0] - (double)N1 / 2.0 * std::log(2 * M_PI);
    c->res = before;
    c->res.factor_extended(fused);
    return GPMI_OK;
}

}  // namespace gpmi
