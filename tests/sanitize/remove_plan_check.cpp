// TEST INFRASTRUCTURE: remove_plan (gaussian_process_amd/csrc/gpmi_remove_plan.h) against brute force, and
// Resident::factor_shrunk (gpmi_state.h); built with g++ -fsanitize=address,undefined by tests/test_remove_cpu.py.
// Brute force means loops over points, rows, columns and multiples of 128 -- no division, no rounding formula.
#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <set>
#include <vector>

#include "gpmi_remove_plan.h"
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

static void check_plan(int64_t N, const std::vector<int64_t>& idx, int64_t reserve, int64_t ld_pad, const char* what) {
    const int64_t k = (int64_t)idx.size();
    const int64_t cap = up_by_loop(N + reserve), ld = cap + ld_pad, rows = cap + 128, Np = up_by_loop(N);
    const RemovePlan p = remove_plan(N, idx.data(), k, ld, rows, Np, ld_pad);
#define WHERE "%s N %lld k %lld", what, (long long)N, (long long)k
    CHECK(p.ok, WHERE);
    if (!p.ok) return;
    // the sorted list
    std::set<int64_t> all(idx.begin(), idx.end());
    CHECK((int64_t)all.size() == k && std::equal(all.begin(), all.end(), p.sorted.begin()) && (int64_t)p.sorted.size() == k, WHERE);
    const int64_t lo = *all.begin();
    CHECK(p.J0 == down_by_loop(lo) && p.ld == ld && p.rows == rows, WHERE);
    // the sweeps carried out on the list of points: what is left is the survivors in their order
    std::vector<int64_t> pts;
    for (int64_t i = 0; i < N; ++i) pts.push_back(i);
    std::set<int64_t> pending = all;
    int64_t n = N, yr = Np;
    for (size_t si = 0; si < p.sweeps.size(); ++si) {
        const RemoveSweep& s = p.sweeps[si];
        CHECK(s.count >= 1 && s.count <= REMOVE_MAX && s.first >= 0 && s.first + s.count <= k, WHERE);
        // descending groups: the 16 largest of what is pending, all of it when fewer are left
        const int64_t want = std::min<int64_t>((int64_t)pending.size(), 16);
        CHECK(s.count == want, WHERE);
        std::vector<int64_t> mine(p.sorted.begin() + s.first, p.sorted.begin() + s.first + s.count);
        for (int64_t j : mine) {
            CHECK(pending.count(j) == 1, WHERE);
            pending.erase(j);
        }
        for (int64_t j : pending) CHECK(j < mine.front(), WHERE);            // pending indices keep their positions
        CHECK(s.N_in == n && s.N_out == n - s.count && mine.back() < n, WHERE);
        CHECK(s.Np_in == up_by_loop(n) && s.Np_out == up_by_loop(n - s.count), WHERE);
        CHECK(s.J0 == down_by_loop(mine.front()), WHERE);
        int64_t blocks = 0;
        for (int64_t c = s.J0; c < s.Np_in; c += 128) ++blocks;
        CHECK(s.blocks == blocks && s.launches == blocks + 1 && blocks >= 1, WHERE);
        CHECK(s.yrow_in == yr && s.yrow_out == s.Np_out && s.yrow_moves == (s.Np_out != yr), WHERE);
        // what fits before still fits: a removal never needs a larger allocation
        CHECK(s.Np_out <= ld - ld_pad && s.Np_out + 128 <= rows, WHERE);
        int64_t copied = 0, streamed = 0;
        for (int64_t r = 0; r < s.J0; r += 128)
            for (int64_t c = 0; c < s.J0; c += 128) copied += 128 * 128 * 8;
        for (int64_t r = s.J0; r < s.Np_in; r += 128)
            for (int64_t c = 0; c <= r; c += 128) streamed += 128 * 128 * 8;
        CHECK(s.copy_bytes == copied && s.stream_bytes == streamed, WHERE);
        // positions in the CURRENT ordering: take them out of the list
        std::vector<int64_t> next;
        for (int64_t i = 0; i < (int64_t)pts.size(); ++i)
            if (!std::binary_search(mine.begin(), mine.end(), i)) next.push_back(pts[(size_t)i]);
        pts.swap(next);
        n = s.N_out;
        yr = s.yrow_out;
    }
    CHECK(pending.empty(), WHERE);
    std::vector<int64_t> want;
    for (int64_t i = 0; i < N; ++i)
        if (!all.count(i)) want.push_back(i);
    CHECK(pts == want, WHERE);
    CHECK(p.N_out == N - k && p.Np_out == up_by_loop(N - k) && p.yrow_out == p.Np_out, WHERE);
    int64_t nsweeps = 0;
    for (int64_t left = k; left > 0; left -= 16) ++nsweeps;
    CHECK((int64_t)p.sweeps.size() == nsweeps, WHERE);
    // every sweep after the first starts no later than the one before
    for (size_t si = 1; si < p.sweeps.size(); ++si) CHECK(p.sweeps[si].J0 <= p.sweeps[si - 1].J0, WHERE);
    CHECK(p.sweeps.back().J0 == p.J0 && p.first_tile * 16 == p.J0, WHERE);
#undef WHERE
}

static void check_refusals() {
    const int64_t N = 300, ld = 384 + 544, rows = 512, pad = 544;
    const int64_t one[] = {5}, dup[] = {5, 9, 5}, low[] = {-1, 3}, high[] = {3, 300};
    std::vector<int64_t> everything;
    for (int64_t i = 0; i < N; ++i) everything.push_back(i);
    CHECK(remove_plan(N, one, 1, ld, rows, 384, pad).ok, "a plain removal");
    CHECK(!remove_plan(N, nullptr, 1, ld, rows, 384, pad).ok, "null idx");
    CHECK(!remove_plan(N, one, 0, ld, rows, 384, pad).ok, "k = 0");
    CHECK(!remove_plan(N, one, -3, ld, rows, 384, pad).ok, "k < 0");
    CHECK(!remove_plan(N, everything.data(), N, ld, rows, 384, pad).ok, "k = N");
    CHECK(remove_plan(N, everything.data(), N - 1, ld, rows, 384, pad).ok, "k = N - 1");
    CHECK(!remove_plan(N, dup, 3, ld, rows, 384, pad).ok, "a duplicate");
    CHECK(!remove_plan(N, low, 2, ld, rows, 384, pad).ok, "an index below 0");
    CHECK(!remove_plan(N, high, 2, ld, rows, 384, pad).ok, "an index == N");
    CHECK(!remove_plan(1, one, 1, ld, rows, 128, pad).ok, "the only point");
    const RemovePlan r = remove_plan(N, dup, 3, ld, rows, 384, pad);
    CHECK(r.sweeps.empty() && r.sorted.empty() && r.why[0] != 0, "a refusal plans nothing and says why");
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
            Resident e = r;                      // factor_extended is the model: the same effects
            e.factor_extended(fused);
            r.factor_shrunk(fused);
            CHECK(r.regression() && r.fit == Fit::Regression, "the fit stays a regression");
            CHECK(r.have_train && r.have_test, "the sets stay");
            CHECK(!r.have_v && !r.v_in_A && !r.post_in_A, "v and the riding posterior factor go");
            CHECK(!r.have_vinv && !r.have_vside, "both inverse flags go");
            CHECK(!r.post_rides(J), "no riding factor is served");
            CHECK(r.factor_fused == fused, "the factor's kind");
            CHECK(r.fit == e.fit && r.have_train == e.have_train && r.have_test == e.have_test && r.have_v == e.have_v &&
                  r.v_in_A == e.v_in_A && r.have_vinv == e.have_vinv && r.have_vside == e.have_vside &&
                  r.post_in_A == e.post_in_A && r.post_in_P == e.post_in_P && r.v_gen == e.v_gen &&
                  r.post_gen_P == e.post_gen_P && r.factor_fused == e.factor_fused, "the effects of factor_extended");
            r.drop_v(); r.v_computed();
            CHECK(!r.post_cached(J), "a P-cached factor of the old v is served");
            r.drop_post_in_P(); r.post_cached_in_P(J);
            CHECK(r.post_cached(J), "a factor cached for the new v");
            r.block_inverses_made(false);
            r.drop_fit();
            CHECK(r.fit == Fit::None && !r.have_v && !r.v_in_A && !r.have_vinv && !r.have_vside && !r.post_in_A && !r.post_in_P,
                  "drop_fit after a removal");
            CHECK(r.have_train && r.have_test, "drop_fit keeps the sets");
        }
}

// index sets of size k in [0, N): at the first index, at the last, on tile edges, spread out; each also unsorted
static std::vector<std::vector<int64_t>> index_sets(int64_t N, int64_t k) {
    std::vector<std::vector<int64_t>> out;
    if (k >= N) return out;
    std::vector<int64_t> a, b, c, d;
    for (int64_t i = 0; i < k; ++i) a.push_back(i);                      // from the first index
    for (int64_t i = 0; i < k; ++i) b.push_back(N - 1 - i);              // down from the last (descending: unsorted)
    for (int64_t i = 0; i < k; ++i) c.push_back(i * N / k);              // spread out (i N / k is strictly increasing for k <= N)
    // tile edges: around every multiple of 16, taken from both ends
    std::set<int64_t> edges;
    for (int64_t e = 0; e <= N + 16 && (int64_t)edges.size() < k; e += 16)
        for (int64_t dl = -1; dl <= 1 && (int64_t)edges.size() < k; ++dl) {
            const int64_t lo = e + dl, hi = N - 1 - (e + dl);
            if (lo >= 0 && lo < N) edges.insert(lo);
            if ((int64_t)edges.size() < k && hi >= 0 && hi < N) edges.insert(hi);
        }
    d.assign(edges.begin(), edges.end());
    out.push_back(a);
    out.push_back(b);
    out.push_back(c);
    if ((int64_t)d.size() == k) out.push_back(d);
    // unsorted: a fixed shuffle of the spread set
    std::vector<int64_t> s = c;
    uint64_t x = 88172645463325252ull + (uint64_t)N * 977 + (uint64_t)k;
    for (size_t i = s.size(); i > 1; --i) {
        x ^= x << 13; x ^= x >> 7; x ^= x << 17;
        std::swap(s[i - 1], s[(size_t)(x % i)]);
    }
    out.push_back(s);
    return out;
}

int main() {
    std::vector<int64_t> Ns;
    for (int64_t m = 0; m <= 1280; m += 128)
        for (int64_t dlt = -2; dlt <= 2; ++dlt)
            if (m + dlt >= 2) Ns.push_back(m + dlt);
    for (int64_t n : {65535, 65536, 65537}) Ns.push_back(n);
    const int64_t ks[] = {1, 2, 15, 16, 17, 33, 200};
    long cases = 0;
    for (int64_t N : Ns)
        for (int64_t k : ks)
            for (const auto& idx : index_sets(N, k))
                for (int64_t reserve : {(int64_t)0, (int64_t)200})
                    for (int64_t pad : {(int64_t)544, (int64_t)0}) {
                        if (N > 60000 && (reserve || !pad)) continue;     // the brute-force lists are long there
                        check_plan(N, idx, reserve, pad, "plan");
                        ++cases;
                    }
    check_refusals();
    check_state();
    if (failures) {
        printf("remove_plan_check: %d failures\n", failures);
        return 1;
    }
    printf("remove_plan_check: ok (%ld plans)\n", cases);
    return 0;
}
