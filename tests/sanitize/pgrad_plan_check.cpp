// TEST INFRASTRUCTURE: pgrad_plan (gaussian_process_amd/csrc/gpmi_pgrad_plan.h) against a brute-force table; built with
// g++ -fsanitize=address,undefined by tests/test_predgrad_cpu.py.  Brute force means loops over rows, blocks and
// multiples -- no division, no rounding formula -- and the route written out as the table of the feature's description:
//   dvar not asked for            -> none, no buffer, whatever else is set
//   factor not fused              -> inverse, whatever the option says
//   option 0                      -> inverse
//   option 1                      -> sweep
//   option -1                     -> sweep exactly when n <= sweep_max
#include <cstdint>
#include <cstdio>

#include "gpmi_pgrad_plan.h"

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

static int64_t up_by_loop(int64_t x, int64_t step) {      // smallest multiple of step that is >= x
    int64_t m = 0;
    while (m < x) m += step;
    return m;
}

static PgradRoute brute_route(int64_t n, int fused, bool want, int opt, int64_t smax) {
    if (!want) return PgradRoute::None;
    if (!fused) return PgradRoute::Inverse;
    if (opt == 0) return PgradRoute::Inverse;
    if (opt == 1) return PgradRoute::Sweep;
    for (int64_t m = 0; m <= smax; ++m)
        if (m == n) return PgradRoute::Sweep;
    return PgradRoute::Inverse;
}

static void check(int64_t n, int64_t Np, int64_t ld_pad, int fused, bool want, int opt, int64_t smax) {
    const int64_t ldA = Np + ld_pad;
    const PgradPlan p = pgrad_plan(n, Np, ldA, ld_pad, fused, want, opt, smax);
    const PgradRoute r = brute_route(n, fused, want, opt, smax);
    CHECK(p.route == r, "n %lld fused %d want %d opt %d smax %lld: route %d, table %d", (long long)n, fused, (int)want, opt,
          (long long)smax, (int)p.route, (int)r);
    CHECK(p.np == up_by_loop(n, 128), "np %lld for n %lld", (long long)p.np, (long long)n);
    if (r == PgradRoute::None) {
        CHECK(p.w_bytes == 0 && p.ldw == 0 && p.groups == 0 && p.launches == 0 && p.stream_bytes == 0 && p.u_bytes == 0,
              "a plan without dvar asks for something (n %lld)", (long long)n);
        return;
    }
    CHECK(p.ldw == Np + ld_pad && p.ldw >= Np && p.ldw % 2 == 0, "ldw %lld", (long long)p.ldw);
    int64_t bytes = 0;
    for (int64_t i = 0; i < up_by_loop(n, 128); ++i) bytes += 8 * (Np + ld_pad);
    CHECK(p.w_bytes == bytes, "w_bytes %lld, by rows %lld", (long long)p.w_bytes, (long long)bytes);
    if (r == PgradRoute::Sweep) {
        int64_t groups = 0, launches = 0, blocks = 0;
        for (int64_t i = 0; i < n; i += 16) ++groups;
        for (int64_t t = 0; t < Np; t += 128) {
            ++launches;
            for (int64_t c = 0; c <= t; c += 128) ++blocks;       // launch t reads one 128 x 128 block per workgroup
        }
        CHECK(p.groups == groups && p.launches == launches, "groups %lld / %lld launches %lld / %lld", (long long)p.groups,
              (long long)groups, (long long)p.launches, (long long)launches);
        CHECK(p.stream_bytes == groups * blocks * 128 * 128 * 8, "stream_bytes %lld", (long long)p.stream_bytes);
        CHECK(p.u_bytes == 0, "the sweep route asks for U");
    } else {
        int64_t ub = 0;
        for (int64_t i = 0; i < Np; ++i) ub += 8 * ldA;
        CHECK(p.u_bytes == ub, "u_bytes %lld, by rows %lld", (long long)p.u_bytes, (long long)ub);
        CHECK(p.groups == 0 && p.launches == 0 && p.stream_bytes == 0, "the inverse route plans a sweep");
    }
}

int main() {
    const int64_t ns[] = {1, 2, 15, 16, 17, 31, 32, 33, 127, 128, 129, 200, 1023, 1024, 1025, 4095, 4096, 4097, 65535};
    const int64_t nps[] = {128, 256, 640, 1152, 1536, 16384, 65536};
    const int64_t smaxs[] = {0, 1, 16, 127, 128, 129, 1024, 4096, 1 << 20};
    const int64_t pads[] = {0, 32, 544};
    long cases = 0;
    for (int64_t n : ns)
        for (int64_t Np : nps)
            for (int64_t smax : smaxs)
                for (int64_t pad : pads)
                    for (int fused = 0; fused <= 1; ++fused)
                        for (int want = 0; want <= 1; ++want)
                            for (int opt = -1; opt <= 1; ++opt) {
                                check(n, Np, pad, fused, want != 0, opt, smax);
                                ++cases;
                            }
    // the default is the documented one, and d's bound is gpmi_sparse_grad's
    CHECK(PGRAD_SWEEP_MAX_DEFAULT == 4096, "default %lld", (long long)PGRAD_SWEEP_MAX_DEFAULT);
    CHECK(PGRAD_MAXD == 32, "PGRAD_MAXD %d", PGRAD_MAXD);
    if (failures) {
        printf("pgrad_plan_check: %d failures in %ld cases\n", failures, cases);
        return 1;
    }
    printf("pgrad_plan_check: ok (%ld cases)\n", cases);
    return 0;
}
