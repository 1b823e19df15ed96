// What a context holds on the device, and the Newton step decision and loop of the two classifiers: host-only, no HIP
// types (plain g++ compiles it; tests/sanitize/state_check.cpp holds it to the table of tests/state_table.py and to the
// classifiers' mirrors on the CPU).
//
// THE RULE.  A context has at most one fit resident, because every fit builds on the same buffers: a regression
// factorisation (A holds L, the y row m = L^-1 y), a binary Laplace fit (A holds the factor of B = I + W^1/2 K W^1/2 at
// the mode), a softmax fit (A holds M = chol(sum_c E_c)) or a sparse fit (sp_L, sp_B; A is not touched, but the
// hyper-parameters of the context are).  Starting any fit drops whatever was resident, and so does everything that
// changes the covariance or the layout the fit was made for: another kernel, other lengthscales, another ld_pad.  A new
// training set drops the test set as well.  A consumer asks for its own kind of fit and is refused otherwise.
//
// Derived from a regression fit and a test set: v^T = K_s^T L^-T, in V (gpmi_predict_resident) or in rows of A (the
// one-pass calls, v_in_A), and the posterior-sample factor cholesky(K_ss + jitter I - v^T v), in A behind L when it rode
// through the augmented factorisation (post_in_A, for post_jitter) or in P (post_in_P, for post_jitter_P and the v of
// generation post_gen_P; v_gen counts every (re)computation of v, so a factor cached for an older v is never served).
// A new test set drops v; the classifiers' and the sparse predictions keep nothing of their own.
//
// Derived from whatever factor is in A: the full inverses of its 128 x 128 diagonal blocks (launch_vinv128; made by the
// first backward solve).  OWNERSHIP: from then on the strict block-upper 16 x 16 tiles of every diagonal block of A hold
// L_kk^-T, not zeros and not K: nothing but the backward-solve kernels may read them (every other consumer of a diagonal
// block masks to the lower triangle; gpmi_get_factor_block zeroes the upper triangle on the way out).  have_vside: the
// row-major side copy of those inverses matches the factor.  Every factorisation into A makes both stale.
// factor_fused: the factor in A came from the fused panel kernels, whose diagonal 16 x 16 tiles carry their inverses
// above the diagonal, which trsm128 reads (panel_mfma.hip): whoever solves with it uses the same kind of leaves.
#pragma once
#include <algorithm>
#include <cmath>
#include <cstdint>

namespace gpmi {

enum class Fit { None, Regression, Laplace, Softmax, Sparse };

struct Resident {
    Fit fit = Fit::None;
    bool have_train = false, have_test = false;
    bool have_v = false, v_in_A = false;
    bool have_vinv = false, have_vside = false;
    bool post_in_A = false, post_in_P = false;
    double post_jitter = 0.0, post_jitter_P = 0.0;
    uint64_t v_gen = 0, post_gen_P = 0;
    int factor_fused = 1;

    bool regression() const { return fit == Fit::Regression; }
    bool laplace() const { return fit == Fit::Laplace; }
    bool softmax() const { return fit == Fit::Softmax; }
    bool sparse() const { return fit == Fit::Sparse; }
    // which posterior-sample factor serves this jitter without a new factorisation
    bool post_rides(double jitter) const { return post_in_A && v_in_A && jitter == post_jitter; }
    bool post_cached(double jitter) const { return post_in_P && jitter == post_jitter_P && post_gen_P == v_gen; }

    // every fit's start, another kernel, other lengthscales, another ld_pad: the fit and everything derived from it
    void drop_fit() {
        fit = Fit::None;
        have_v = v_in_A = have_vinv = have_vside = post_in_A = post_in_P = false;
    }
    void drop_train() { drop_fit(); have_train = have_test = false; }      // a new training set (or a lane's)
    void drop_test() { have_test = have_v = false; }                       // a new test set
    void train_set() { have_train = true; }
    void test_set() { have_test = true; }
    void factor_replaced(int fused) { have_vinv = have_vside = false; factor_fused = fused; }   // after any Cholesky into A
    // gpmi_append: the regression factor grew by a border.  The fit stays; the border's diagonal blocks are new, so the
    // next backward solve inverts again; v belongs to the shorter factor and goes, and the riding posterior factor with
    // it (one cached in P is tied to its v by v_gen: the next v_computed() outdates it)
    void factor_extended(int fused) { factor_replaced(fused); drop_v(); post_in_A = false; }
    // gpmi_remove: the regression factor lost rows and columns and everything behind them was rotated.  The fit stays;
    // the diagonal blocks from the first removed index on are new, so the next backward solve inverts again; v belongs to
    // the longer factor and goes, and the riding posterior factor with it (one cached in P: as above)
    void factor_shrunk(int fused) { factor_replaced(fused); drop_v(); post_in_A = false; }
    void block_inverses_made(bool side) { have_vinv = true; have_vside = side; }
    void fit_done(Fit f) { fit = f; }
    void drop_v() { have_v = v_in_A = false; }                             // a prediction is about to overwrite V
    void v_computed() { have_v = true; ++v_gen; }
    void v_in_rows_of_A(bool post, double jitter) {                        // the one-pass regression's ending
        v_in_A = true;
        v_computed();
        post_in_A = post;
        post_jitter = jitter;
    }
    void drop_post_in_P() { post_in_P = false; }                           // P is about to be overwritten
    void post_cached_in_P(double jitter) { post_in_P = true; post_jitter_P = jitter; post_gen_P = v_gen; }
};

// What a classifier's Newton iteration does with the objective Psi of a new iterate against the previous one's: it has
// converged when Psi moved by at most tol max(1, |Psi|), the step is halved when Psi fell by more than that (at most 20
// times), and is accepted otherwise.
enum class Step { Converged, Halve, Accept };
inline Step newton_decide(double psi, double psi_prev, double tol, int halvings) {
    const double d = psi - psi_prev, thr = tol * std::max(1.0, std::fabs(psi));
    if (std::fabs(d) <= thr) return Step::Converged;
    if (d < -thr && halvings < 20) return Step::Halve;
    return Step::Accept;
}

// The Newton iteration of both classifiers around newton_decide.  The problem supplies four callbacks, each returning a
// status (non-zero ends the run at once with that status, *iters and *converged untouched):
//   forward()             the products the objective needs from the current iterate
//   evaluate(mode, &psi)  Psi of the fresh iterate (mode 0) or of the step halved once more (mode 1)
//   factor(last)          the factorisations at the iterate; last: no step follows, the factor stays resident
//   step()                the Newton step from that factor (the problem keeps the previous iterate for the halvings)
// No line search runs before the first step; a step is halved while newton_decide says so; the run ends behind the factor
// of a converged iterate or of iterate max_iter.  The problem keeps the last Psi it reported: it is the final iterate's.
template <class Problem>
int newton_iterate(Problem& p, double tol, int max_iter, int* iters, bool* converged) {
    double psi = 0.0, psi_prev = 0.0;
    bool have_prev = false, conv = false;
    int it = 0, rc;
    for (;;) {
        if ((rc = p.forward())) return rc;
        if ((rc = p.evaluate(0, &psi))) return rc;
        if (have_prev) {
            for (int halvings = 0;; ++halvings) {
                const Step step = newton_decide(psi, psi_prev, tol, halvings);
                if (step != Step::Halve) { conv = step == Step::Converged; break; }
                if ((rc = p.evaluate(1, &psi))) return rc;
            }
        }
        const bool last = conv || it >= max_iter;
        if ((rc = p.factor(last))) return rc;
        if (last) break;
        if ((rc = p.step())) return rc;
        psi_prev = psi;
        have_prev = true;
        ++it;
    }
    *iters = it;
    *converged = conv;
    return 0;
}

}  // namespace gpmi
