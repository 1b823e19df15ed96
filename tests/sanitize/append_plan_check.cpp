// TEST INFRASTRUCTURE: append_plan (gaussian_process_amd/csrc/gpmi_append_plan.h) against brute force, and
// Resident::factor_extended (gpmi_state.h); built with g++ -fsanitize=address,undefined by tests/test_append_plan_cpu.py.
// Brute force means loops over rows, columns and multiples of 128 -- no division, no rounding formula.
#include <cstdint>
#include <cstdio>
#include <vector>

#include "gpmi_append_plan.h"
#include "gpmi_state.h"

using namespace gpmi;

static int failures = 0;
#define CHECK(cond, ...)                                  \
    do {                                                  \
        if (!(cond)) {                                    \
            if (failures++ < 20) {                        \
                printf("FAIL %s: ", #cond);               \
                printf(__VA_ARGS__);                      \
                printf("\n");                             \
            }                                             \
        }                                                 \
    } while (0)

static int64_t up_by_loop(int64_t x) {      // smallest multiple of 128 that is >= x
    int64_t m = 0;
    while (m < x) m += 128;
    return m;
}
static int64_t down_by_loop(int64_t x) {    // largest multiple of 128 that is <= x
    int64_t m = 0;
    while (m + 128 <= x) m += 128;
    return m;
}

// Row i of the padded matrix of a fit of M points, lower triangle: real (K) left of min(i + 1, M) when i < M, identity
// otherwise.  A row differs between the fits of N and N + k points when it is real in one and padding in the other, or
// does not exist in the smaller one; a 128-row tile has to be rebuilt when any of its rows differs.
static void brute_border(int64_t N, int64_t k, int64_t* first, int64_t* last) {
    const int64_t Np = up_by_loop(N), Np1 = up_by_loop(N + k);
    *first = -1; *last = -1;
    for (int64_t t = 0; t < Np1; t += 128) {
        bool differs = false;
        for (int64_t i = t; i < t + 128; ++i) {
            const bool exists_old = i < Np;
            const bool real_old = i < N, real_new = i < N + k;
            if (!exists_old || real_old != real_new) differs = true;
        }
        if (differs) {
            if (*first < 0) *first = t;
            *last = t + 128;
        } else {
            CHECK(*first < 0, "an unchanged tile row %lld behind a changed one (N %lld k %lld)", (long long)t, (long long)N, (long long)k);
        }
    }
}

static void check_plan(int64_t N, int64_t k, int64_t reserve, int64_t ld_pad, int fused, int opt) {
    // the resident layout: what a fit of N points with this reserve chose
    const int64_t cap = up_by_loop(N + reserve), ld = cap + ld_pad, rows = cap + 128, Np = up_by_loop(N);
    const AppendPlan p = append_plan(N, k, ld, rows, Np, ld_pad, reserve, fused, opt);
    const int64_t Np1 = up_by_loop(N + k), N0 = down_by_loop(N);
    CHECK(p.N1 == N + k && p.Np == Np && p.Np1 == Np1 && p.N0 == N0, "sizes N %lld k %lld", (long long)N, (long long)k);
    int64_t first, last;
    brute_border(N, k, &first, &last);
    CHECK(first == p.N0 && last == p.Np1 && p.border == last - first, "border [%lld, %lld) against plan [%lld, %lld) N %lld k %lld",
          (long long)first, (long long)last, (long long)p.N0, (long long)p.Np1, (long long)N, (long long)k);
    CHECK(p.border % 128 == 0 && p.border >= 128, "border %lld", (long long)p.border);
    const bool skinny = k <= 16 && fused && N0 > 0 && opt != 0;
    CHECK(p.skinny == skinny, "route N %lld k %lld fused %d opt %d", (long long)N, (long long)k, fused, opt);
    // in place exactly when every row and column the result needs exists: the factor's columns are those left of the
    // pad, its rows are followed by the 128 rows of the y block
    bool fits = true;
    for (int64_t t = 0; t < Np1; t += 128)
        if (t + 128 > ld - ld_pad) fits = false;
    for (int64_t t = 0; t < Np1 + 128; t += 128)
        if (t + 128 > rows) fits = false;
    CHECK(p.in_place == fits, "in place N %lld k %lld reserve %lld", (long long)N, (long long)k, (long long)reserve);
    CHECK(p.yrow == Np1 && p.yrow_moves == (Np1 != Np), "y row N %lld k %lld", (long long)N, (long long)k);
    if (N + k <= Np) CHECK(p.in_place && !p.yrow_moves, "an append inside the padding N %lld k %lld", (long long)N, (long long)k);
    if (p.in_place) {
        CHECK(p.ld == ld && p.rows == rows && p.copy_bytes == 0, "in-place layout N %lld k %lld", (long long)N, (long long)k);
    } else {
        const int64_t cap1 = up_by_loop(N + k + reserve);
        CHECK(p.ld == cap1 + ld_pad && p.rows == cap1 + 128, "fresh layout N %lld k %lld", (long long)N, (long long)k);
        CHECK(p.keep_rows == (skinny ? N : N0) && p.copy_bytes == p.keep_rows * N0 * 8, "copy N %lld k %lld", (long long)N, (long long)k);
        // the next append of the same size fits the new layout when the reserve covers it
        const AppendPlan q = append_plan(N + k, 1, p.ld, p.rows, p.yrow, ld_pad, reserve, fused, opt);
        if (reserve >= 1) CHECK(q.in_place, "reserve does not cover the next point N %lld k %lld", (long long)N, (long long)k);
    }
    int64_t blocks = 0;
    for (int64_t r = 0; r < N0; r += 128)
        for (int64_t c = 0; c <= r; c += 128) ++blocks;
    CHECK(p.sweep_bytes == blocks * 128 * 128 * 8, "sweep bytes N %lld", (long long)N);
    CHECK(p.build_rows == (skinny ? k : p.border), "build rows N %lld k %lld", (long long)N, (long long)k);
}

static void check_state() {
    const double J = 1e-6;
    for (int fused = 0; fused <= 1; ++fused)
        for (int riding = 0; riding <= 1; ++riding) {
            Resident r;
            r.drop_train(); r.train_set();
            r.drop_test(); r.test_set();
            r.drop_fit(); r.factor_replaced(fused); r.fit_done(Fit::Regression);
            if (riding) r.v_in_rows_of_A(true, J);
            else { r.drop_v(); r.v_computed(); r.drop_post_in_P(); r.post_cached_in_P(J); }
            r.block_inverses_made(true);
            CHECK(r.have_v && r.have_vinv && r.have_vside && (riding ? r.post_rides(J) : r.post_cached(J)), "setup");
            r.factor_extended(fused);
            CHECK(r.regression() && r.fit == Fit::Regression, "the fit stays a regression");
            CHECK(r.have_train && r.have_test, "the sets stay");
            CHECK(!r.have_v && !r.v_in_A && !r.post_in_A, "v and the riding posterior factor go");
            CHECK(!r.have_vinv && !r.have_vside, "both inverse flags go");
            CHECK(!r.post_rides(J), "no riding factor is served");
            CHECK(r.factor_fused == fused, "the factor's kind");
            // the next prediction computes v anew: a factor cached in P for the old v is not served for it
            r.drop_v(); r.v_computed();
            CHECK(!r.post_cached(J), "a P-cached factor of the old v is served");
            r.drop_post_in_P(); r.post_cached_in_P(J);
            CHECK(r.post_cached(J), "a factor cached for the new v");
            // a later drop_fit behaves as before
            r.block_inverses_made(false);
            r.drop_fit();
            CHECK(r.fit == Fit::None && !r.have_v && !r.v_in_A && !r.have_vinv && !r.have_vside && !r.post_in_A && !r.post_in_P,
                  "drop_fit after an append");
            CHECK(r.have_train && r.have_test, "drop_fit keeps the sets");
        }
}

int main() {
    std::vector<int64_t> Ns;
    for (int64_t m = 0; m <= 1280; m += 128)
        for (int64_t dlt = -2; dlt <= 2; ++dlt)
            if (m + dlt >= 1) Ns.push_back(m + dlt);
    for (int64_t n : {65535, 65536, 65537}) Ns.push_back(n);
    const int64_t ks[] = {1, 2, 15, 16, 17, 127, 128, 129, 1000};
    const int64_t reserves[] = {0, 1, 200, 1000};
    long cases = 0;
    for (int64_t N : Ns)
        for (int64_t k : ks)
            for (int64_t r : reserves)
                for (int64_t pad : {(int64_t)544, (int64_t)0})
                    for (int fused = 0; fused <= 1; ++fused)
                        for (int opt = -1; opt <= 1; ++opt) {
                            check_plan(N, k, r, pad, fused, opt);
                            ++cases;
                        }
    check_state();
    if (failures) {
        printf("append_plan_check: %d failures\n", failures);
        return 1;
    }
    printf("append_plan_check: ok (%ld plans)\n", cases);
    return 0;
}
