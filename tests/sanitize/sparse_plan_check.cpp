// TEST INFRASTRUCTURE: gram_plan and sparse_slabs (gaussian_process_amd/csrc/gpmi_sparse_plan.h) against brute force;
// built with g++ -fsanitize=address,undefined by tests/test_sparse_routes_cpu.py.  Brute force means loops over rows,
// 128-row units and tiles -- the walk gram_tn_kernel and sparse_fit_impl make -- and no rounding formula of the header.
//
//   sparse_plan_check                  every mp in 128..4096 and rows in 128..20480; every (Np, slab option, mp)
//   sparse_plan_check plan N slab mp   prints the slabs of that fit and the Gram plan of each, one line per slab
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "gpmi_sparse_plan.h"

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

typedef long long ll;

static int64_t up_by_loop(int64_t x, int64_t step) {      // smallest multiple of step that is >= x
    int64_t m = 0;
    while (m < x) m += step;
    return m;
}
static int64_t pieces_by_loop(int64_t x, int64_t piece) {  // pieces of `piece` that cover x
    int64_t n = 0;
    for (int64_t at = 0; at < x; at += piece) ++n;
    return n;
}
static int64_t lower_tiles_by_loop(int64_t mp) {
    int64_t n = 0;
    for (int64_t I = 0; I < mp; I += 128)
        for (int64_t J = 0; J <= I; J += 128) ++n;
    return n;
}

// the chunks as gram_tn_kernel walks them: split z takes rows [z chunk, min((z + 1) chunk, rows)) in stages of 16
struct Walk { int64_t units, last_chunk, splits; };
static Walk check_gram(int64_t rows, int64_t mp, int64_t ntiles) {
    const GramPlan p = gram_plan(rows, mp);
    const int64_t units = pieces_by_loop(rows, 128);
    CHECK(p.ntiles == ntiles, "tiles %lld of mp %lld", (ll)p.ntiles, (ll)mp);
    CHECK(p.ntiles <= 0x7fffffff && p.nsplit >= 1 && p.nsplit <= 65535, "grid %lld x %lld", (ll)p.ntiles, (ll)p.nsplit);
    CHECK(p.nsplit <= units, "%lld splits of %lld units (rows %lld mp %lld)", (ll)p.nsplit, (ll)units, (ll)rows, (ll)mp);
    CHECK(p.chunk >= 128 && p.chunk % 128 == 0, "chunk %lld", (ll)p.chunk);
    std::vector<int> seen((size_t)units, 0);
    int64_t next = 0, last = 0, splits = 0;
    for (int64_t z = 0; z < p.nsplit; ++z) {
        const int64_t k0 = z * p.chunk, k1 = k0 + p.chunk < rows ? k0 + p.chunk : rows;
        CHECK(k0 == next && k1 > k0, "split %lld [%lld, %lld) after %lld (rows %lld mp %lld)", (ll)z, (ll)k0, (ll)k1, (ll)next, (ll)rows, (ll)mp);
        if (k1 <= k0) break;
        CHECK((k1 - k0) % 128 == 0 && (k1 - k0) % 16 == 0, "split %lld holds %lld rows", (ll)z, (ll)(k1 - k0));
        for (int64_t r = k0; r < k1; r += 128) {
            CHECK(r + 128 <= rows, "unit at %lld leaves %lld rows", (ll)r, (ll)rows);
            if (r + 128 <= rows) ++seen[(size_t)(r / 128)];
        }
        next = k1;
        last = k1 - k0;
        ++splits;
    }
    CHECK(next == rows, "the splits end at %lld of %lld rows (mp %lld)", (ll)next, (ll)rows, (ll)mp);
    for (int64_t u = 0; u < units; ++u) CHECK(seen[(size_t)u] == 1, "unit %lld taken %d times (rows %lld mp %lld)", (ll)u, seen[(size_t)u], (ll)rows, (ll)mp);
    // as many splits as the target of 1024 workgroups allows: the chunk is the shortest whose splits stay within
    // min(units, the splits that bring tiles x splits to the target)
    int64_t want = 0;
    while (want * ntiles < GRAM_TARGET_GROUPS) ++want;
    const int64_t most = units < want ? units : want;
    int64_t cu = 1;
    while (pieces_by_loop(units, cu) > most) ++cu;
    CHECK(p.chunk == cu * 128 && p.nsplit == pieces_by_loop(units, cu), "chunk %lld x %lld against %lld units x %lld (rows %lld mp %lld)",
          (ll)p.chunk, (ll)p.nsplit, (ll)cu, (ll)pieces_by_loop(units, cu), (ll)rows, (ll)mp);
    return Walk{units, last, splits};
}

// doubles launch_gemv_t (solve.hip) writes into its scratch for `rows` x mp: one row of mp partial sums per row chunk --
// chunks of rpw 128-row pieces in the aligned form, of 64 rows in the other
static int64_t gemv_need(int64_t rows, int64_t mp) {
    const int64_t nch128 = pieces_by_loop(rows, 128), ccols = pieces_by_loop(mp, 256);
    int64_t rpw = nch128 * ccols / 1024;
    if (rpw < 1) rpw = 1;
    if (rpw > 16) rpw = 16;
    const int64_t aligned = pieces_by_loop(nch128, rpw) * mp, plain = pieces_by_loop(rows, 64) * mp;
    return aligned > plain ? aligned : plain;
}

// per mp, by slab length in units: what a slab needs (filled by main from the walks above)
static std::vector<int64_t> part_need, scratch_need;

static void check_fit(int64_t N, int64_t opt, int64_t mp) {
    const SparseSlabs s = sparse_slabs(N, opt, mp);
    const int64_t Np = up_by_loop(N, 128);
    int64_t S = opt ? up_by_loop(opt, 128) : 16384;
    if (S > Np) S = Np;
    CHECK(s.Np == Np && s.S == S && S >= 128, "N %lld option %lld: Np %lld S %lld", (ll)N, (ll)opt, (ll)s.Np, (ll)s.S);
    int64_t nslabs = 0, covered = 0, rows = 0;
    for (int64_t row0 = 0; row0 < Np; row0 += S) {          // the loop of sparse_fit_impl
        rows = S < Np - row0 ? S : Np - row0;
        const int64_t nreal = rows < N - row0 ? rows : N - row0;
        CHECK(rows % 128 == 0 && rows >= 128 && rows <= s.S, "slab at %lld of %lld rows", (ll)row0, (ll)rows);
        CHECK(nreal >= 1, "slab at %lld holds no real row (N %lld option %lld)", (ll)row0, (ll)N, (ll)opt);
        const size_t u = (size_t)(rows / 128);
        CHECK(part_need[u] <= s.part_doubles, "slab of %lld rows needs %lld doubles of partial tiles, %lld held (Np %lld option %lld mp %lld)",
              (ll)rows, (ll)part_need[u], (ll)s.part_doubles, (ll)Np, (ll)opt, (ll)mp);
        CHECK(scratch_need[u] <= s.gemv_doubles, "gemv on %lld rows needs %lld of %lld doubles (mp %lld)", (ll)rows,
              (ll)scratch_need[u], (ll)s.gemv_doubles, (ll)mp);
        covered += rows;
        ++nslabs;
    }
    CHECK(covered == Np && nslabs == s.nslabs && rows == s.last_rows, "N %lld option %lld: %lld slabs cover %lld, the last %lld (header: %lld, %lld)",
          (ll)N, (ll)opt, (ll)nslabs, (ll)covered, (ll)rows, (ll)s.nslabs, (ll)s.last_rows);
}

static int print_plan(int64_t N, int64_t opt, int64_t mp) {
    if (N < 1 || opt < 0 || mp < 128 || mp % 128) { fprintf(stderr, "plan N slab mp: mp a multiple of 128\n"); return 2; }
    const SparseSlabs s = sparse_slabs(N, opt, mp);
    const int64_t ntiles = lower_tiles_by_loop(mp);
    printf("fit Np %lld S %lld nslabs %lld last_rows %lld mp %lld ntiles %lld part_doubles %lld gemv_doubles %lld\n", (ll)s.Np,
           (ll)s.S, (ll)s.nslabs, (ll)s.last_rows, (ll)mp, (ll)ntiles, (ll)s.part_doubles, (ll)s.gemv_doubles);
    int64_t i = 0;
    for (int64_t row0 = 0; row0 < s.Np; row0 += s.S, ++i) {
        const int64_t rows = s.S < s.Np - row0 ? s.S : s.Np - row0, nreal = rows < N - row0 ? rows : N - row0;
        const GramPlan p = gram_plan(rows, mp);
        const Walk w = check_gram(rows, mp, ntiles);
        printf("slab %lld rows %lld real %lld units %lld nsplit %lld chunk %lld last_chunk %lld\n", (ll)i, (ll)rows, (ll)nreal,
               (ll)w.units, (ll)p.nsplit, (ll)p.chunk, (ll)w.last_chunk);
    }
    return failures ? 1 : 0;
}

int main(int argc, char** argv) {
    if (argc == 5 && !strcmp(argv[1], "plan")) return print_plan(atoll(argv[2]), atoll(argv[3]), atoll(argv[4]));
    if (argc != 1) { fprintf(stderr, "usage: sparse_plan_check [plan N slab mp]\n"); return 2; }
    long plans = 0, fits = 0;
    std::vector<int64_t> opts = {0, 1, 127, 129, 1000, 3000, 16383, 16385, 1 << 20};
    for (int64_t o = 128; o <= 20480; o += 128) opts.push_back(o);
    for (int64_t mp = 128; mp <= 4096; mp += 128) {
        const int64_t ntiles = lower_tiles_by_loop(mp);
        part_need.assign(161, 0);
        scratch_need.assign(161, 0);
        for (int64_t rows = 128; rows <= 20480; rows += 128) {
            const Walk w = check_gram(rows, mp, ntiles);
            part_need[(size_t)w.units] = ntiles * w.splits * 128 * 128;      // a 128 x 128 tile per (lower tile, split walked)
            scratch_need[(size_t)w.units] = gemv_need(rows, mp);
            ++plans;
        }
        for (int64_t Np = 128; Np <= 20480; Np += 128)
            for (int64_t opt : opts)
                for (int64_t N : {Np - 127, Np - 36, Np}) {
                    check_fit(N, opt, mp);
                    ++fits;
                }
    }
    if (failures) {
        printf("sparse_plan_check: %d failures\n", failures);
        return 1;
    }
    printf("sparse_plan_check: ok (%ld plans, %ld fits)\n", plans, fits);
    return 0;
}
