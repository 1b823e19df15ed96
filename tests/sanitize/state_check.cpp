// TEST INFRASTRUCTURE: Resident, newton_decide and newton_iterate (gaussian_process_amd/csrc/gpmi_state.h) asked from the command line,
// built with g++ -fsanitize=address,undefined by tests/test_state_cpu.py.
//   state_check events   one event name of tests/state_table.py per line of standard input ("reset": a fresh context);
//                        each is applied through the transitions the library's entry point of that name goes through,
//                        and answered by one line: the consumer groups the state then accepts ("-": none)
//   state_check newton   one "psi psi_prev tol halvings" per line (hex floats); the answer is newton_decide's
//   state_check iterate  one run of newton_iterate per line: "tol max_iter fail nth status psi ..." (hex floats); the
//                        psi are what the problem's evaluate reports, call by call; the nth call (from 1) of the
//                        callback `fail` (forward, eval, factor or step; "-": none) returns `status`.  The answer is
//                        the trace of calls (forward, eval0, eval1, factor0, factor1, step), then iters, converged and
//                        the status (iters and converged are -1 where newton_iterate left them alone)
// An unknown word, or a run that asks for more psi than its line holds, prints FAIL and exits non-zero.
#include <cstdio>
#include <cstdlib>
#include <iostream>
#include <sstream>
#include <string>
#include <vector>

#include "gpmi_state.h"

using namespace gpmi;

static const double JITTER = 1e-6;      // every post_chol of the table asks for the same jitter

static void start_fit(Resident& r, Fit f) {
    r.drop_fit();
    if (f != Fit::Sparse) r.factor_replaced(1);      // a sparse fit leaves A alone
    r.fit_done(f);
}

// false: the entry point refuses the call before it changes anything
static bool apply_event(Resident& r, const std::string& ev) {
    if (ev == "set_train") { r.drop_train(); r.train_set(); return true; }
    if (ev == "set_kernel" || ev == "set_lengthscales" || ev == "ld_pad") { r.drop_fit(); return true; }
    if (!r.have_train) return false;
    if (ev == "set_test") { r.drop_test(); r.test_set(); return true; }
    if (ev == "factorize") { start_fit(r, Fit::Regression); return true; }
    if (ev == "laplace_fit") { start_fit(r, Fit::Laplace); return true; }
    if (ev == "softmax_fit") { start_fit(r, Fit::Softmax); return true; }
    if (ev == "sparse_fit") { start_fit(r, Fit::Sparse); return true; }
    if (ev == "post_chol") {
        if (!r.have_v) return false;
        if (!r.post_rides(JITTER) && !r.post_cached(JITTER)) { r.drop_post_in_P(); r.post_cached_in_P(JITTER); }
        return true;
    }
    if (!r.have_test) return false;
    if (ev == "fit_predict" || ev == "fit_predict_sample") {
        start_fit(r, Fit::Regression);
        r.v_in_rows_of_A(ev == "fit_predict_sample", JITTER);
        return true;
    }
    if (ev == "predict") {
        if (!r.regression()) return false;
        r.drop_v();
        r.v_computed();
        return true;
    }
    if (ev == "laplace_predict" || ev == "softmax_predict") {
        if (!(ev == "laplace_predict" ? r.laplace() : r.softmax())) return false;
        r.drop_v();
        return true;
    }
    if (ev == "sparse_predict") return r.sparse();
    std::printf("FAIL: unknown event %s\n", ev.c_str());
    std::exit(1);
}

static void answer(const Resident& r) {
    std::string out;
    auto add = [&](bool on, const char* name) { if (on) out += std::string(out.empty() ? "" : " ") + name; };
    add(r.regression(), "regression");
    add(r.laplace(), "laplace");
    add(r.softmax(), "softmax");
    add(r.sparse(), "sparse");
    add(r.have_test, "test");
    add(r.have_v, "post");
    add(r.have_v && (r.post_rides(JITTER) || r.post_cached(JITTER)), "post_kept");
    std::puts(out.empty() ? "-" : out.c_str());
}

// newton_iterate's problem from a script: every callback appends its name to the trace
struct ScriptedProblem {
    std::vector<double> psi;
    size_t next = 0;
    std::string fail;
    int nth = 0, status = 0;
    int calls[4] = {0, 0, 0, 0};
    std::string trace;

    int called(int which, const char* name, const std::string& shown) {
        trace += shown + " ";
        return fail == name && ++calls[which] == nth ? status : 0;
    }
    int forward() { return called(0, "forward", "forward"); }
    int evaluate(int mode, double* out) {
        if (next == psi.size()) { std::printf("FAIL: the script ran out of psi after: %s\n", trace.c_str()); std::exit(1); }
        *out = psi[next++];
        return called(1, "eval", mode ? "eval1" : "eval0");
    }
    int factor(bool last) { return called(2, "factor", last ? "factor1" : "factor0"); }
    int step() { return called(3, "step", "step"); }
};

int main(int argc, char** argv) {
    const std::string mode = argc > 1 ? argv[1] : "";
    std::string line;
    if (mode == "events") {
        Resident r;
        while (std::getline(std::cin, line)) {
            if (line == "reset") { r = Resident(); continue; }
            apply_event(r, line);
            answer(r);
        }
        return 0;
    }
    if (mode == "newton") {
        while (std::getline(std::cin, line)) {
            std::istringstream in(line);
            std::string a, b, c;
            int halvings = 0;
            if (!(in >> a >> b >> c >> halvings)) { std::printf("FAIL: %s\n", line.c_str()); return 1; }
            const Step s = newton_decide(std::strtod(a.c_str(), nullptr), std::strtod(b.c_str(), nullptr),
                                         std::strtod(c.c_str(), nullptr), halvings);
            std::puts(s == Step::Converged ? "converged" : s == Step::Halve ? "halve" : "accept");
        }
        return 0;
    }
    if (mode == "iterate") {
        while (std::getline(std::cin, line)) {
            std::istringstream in(line);
            std::string tol, word;
            int max_iter = 0;
            ScriptedProblem p;
            if (!(in >> tol >> max_iter >> p.fail >> p.nth >> p.status)) { std::printf("FAIL: %s\n", line.c_str()); return 1; }
            while (in >> word) p.psi.push_back(std::strtod(word.c_str(), nullptr));
            int iters = -1;
            bool converged = false;
            const int rc = newton_iterate(p, std::strtod(tol.c_str(), nullptr), max_iter, &iters, &converged);
            std::printf("%s%d %d %d\n", p.trace.c_str(), iters, iters < 0 ? -1 : (int)converged, rc);
        }
        return 0;
    }
    std::printf("FAIL: mode must be events, newton or iterate\n");
    return 1;
}
