// TEST INFRASTRUCTURE: the pair plans of gaussian_process_amd/csrc/gpmi_plan.h (the 256 x 128 form of the LDS-DMA GEMM:
// one block = row tiles ti, ti + 1 of one tile column) against brute force, built with g++ -fsanitize=address,undefined
// by tests/test_pair_plan_cpu.py.
//   * every live 128-tile is covered by exactly one block, as one of that block's live halves (plan_pair_live), and no
//     block writes a dead tile -- rectangles, lower triangles with any diagonal offset, row maps with and without a host
//     copy, odd tile counts, every supertile edge, the trailing updates of the headline size;
//   * in a lower-triangular plan with diag_off 0 no block that maps into the grid has two dead halves, except the
//     last, half-outside pair row of an odd tile count;
//   * the pair plan keeps the 128-tile plan's supertiles (edge, count, staircase table) and prices a block at two tiles.
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <random>
#include <vector>

#include "gpmi_plan.h"

using namespace gpmi;

static int g_fail = 0;
#define CHECK(cond, ...) do { if (!(cond)) { ++g_fail; fprintf(stderr, "FAIL %s:%d: ", __FILE__, __LINE__); fprintf(stderr, __VA_ARGS__); fprintf(stderr, "\n"); if (g_fail > 20) exit(1); } } while (0)

static bool brute_live(int64_t ti, int64_t tj, int lower, int64_t diag_off, const std::vector<int32_t>* map, int rbt) {
    if (lower && tj * 128 > ti * 128 + 127 + diag_off) return false;
    if (map && tj * 128 >= (*map)[(size_t)(ti / rbt)]) return false;
    return true;
}

static long check_pair_plan(int64_t Tm, int64_t Tn, int lower, int64_t diag_off, const std::vector<int32_t>* map,
                            bool host_copy, int rbt, int force_S, bool balance) {
    const int32_t* hmap = (map && host_copy) ? map->data() : nullptr;
    const int bands = (map && host_copy) ? (int)map->size() : 0;
    TilePlan p;
    const bool ok = plan_tiles(p, Tm, Tn, lower, diag_off, map != nullptr, hmap, bands, rbt, force_S, balance, true);
    if (force_S == 1) {
        CHECK(!ok, "a pair plan with supertile edge 1 must be refused");
        return 0;
    }
    CHECK(ok, "plan_tiles refused Tm=%ld Tn=%ld", (long)Tm, (long)Tn);
    if (!ok) return 0;
    CHECK(p.pair == 1, "pair flag");
    CHECK(p.S == 2 || p.S == 4 || p.S == 8, "S=%d", p.S);
    CHECK((1 << p.logS) == p.S, "logS");
    CHECK(p.nblocks % 8 == 0 && p.nblocks == ((p.nsuper + 7) / 8) * 8 * p.S * p.S / 2, "nblocks");
    if (p.tri == 2) CHECK(p.SM <= DMA_MAX_SM && p.sprefix[p.SM] == p.nsuper, "staircase prefix");
    // same supertiles as the 128-tile plan at the same edge
    TilePlan t;
    CHECK(plan_tiles(t, Tm, Tn, lower, diag_off, map != nullptr, hmap, bands, rbt, p.S, false, false), "tile plan");
    CHECK(t.nsuper == p.nsuper && t.tri == p.tri && t.SM == p.SM && t.SN == p.SN, "supertiles differ from the tile plan");
    std::vector<unsigned char> seen((size_t)Tm * Tn, 0);
    long written = 0, both_dead = 0;
    for (int b = 0; b < p.nblocks; ++b) {
        int ti = -1, tj = -1;
        if (!plan_block_to_tile(p, b, ti, tj)) continue;
        CHECK(ti >= 0 && ti < Tm && tj >= 0 && tj < Tn, "block out of range b=%d -> (%d,%d)", b, ti, tj);
        CHECK(ti % 2 == 0, "pair starts on an odd tile row b=%d ti=%d", b, ti);
        bool l0 = false, l1 = false;
        plan_pair_live(p, ti, tj, map ? map->data() : nullptr, l0, l1);
        if (!l0 && !l1) { ++both_dead; continue; }
        for (int h = 0; h < 2; ++h) {
            if (!(h ? l1 : l0)) continue;
            const int64_t r = ti + h;
            CHECK(r < Tm, "live half below the grid (%ld,%d)", (long)r, tj);
            CHECK(brute_live(r, tj, lower, diag_off, map, rbt), "block writes dead tile (%ld,%d)", (long)r, tj);
            CHECK(!seen[(size_t)r * Tn + tj], "tile (%ld,%d) covered twice (Tm=%ld Tn=%ld lower=%d S=%d tri=%d)", (long)r, tj,
                  (long)Tm, (long)Tn, lower, p.S, p.tri);
            seen[(size_t)r * Tn + tj] = 1;
            ++written;
        }
    }
    long live = 0;
    for (int64_t ti = 0; ti < Tm; ++ti)
        for (int64_t tj = 0; tj < Tn; ++tj)
            if (brute_live(ti, tj, lower, diag_off, map, rbt)) {
                ++live;
                CHECK(seen[(size_t)ti * Tn + tj], "live tile (%ld,%ld) not covered (Tm=%ld Tn=%ld lower=%d diag=%ld S=%d tri=%d map=%d host=%d)",
                      (long)ti, (long)tj, (long)Tm, (long)Tn, lower, (long)diag_off, p.S, p.tri, map != nullptr, (int)host_copy);
            }
    CHECK(live == written, "live %ld != written %ld", live, written);
    CHECK(plan_live_tiles(Tm, Tn, lower, diag_off, hmap, bands, rbt) == (map && !host_copy ? plan_live_tiles(Tm, Tn, lower, diag_off, nullptr, 0, rbt) : live),
          "plan_live_tiles");
    if (p.tri == 1 && Tm % 2 == 0) CHECK(both_dead == 0, "%ld blocks with two dead halves (Tm=%ld Tn=%ld S=%d)", both_dead, (long)Tm, (long)Tn, p.S);
    const double eff = plan_xcd_efficiency(p, hmap);
    CHECK(eff > 0.0 && eff <= 1.0 + 1e-12, "efficiency %g", eff);
    return live;
}

int main() {
    std::mt19937 rng(4321);
    long tiles = 0, plans = 0;
    const int forces[] = {0, 1, 2, 4, 8};
    const int64_t dims[] = {1, 2, 3, 5, 7, 8, 9, 15, 16, 17, 31, 33, 64, 100, 127, 128, 129, 255, 512};
    for (int64_t Tm : dims)
        for (int64_t Tn : dims) {
            if (Tm * Tn > 40000) continue;
            for (int f : forces) {
                tiles += check_pair_plan(Tm, Tn, 0, 0, nullptr, false, 1, f, true); ++plans;
                for (int64_t doff : {(int64_t)0, (int64_t)-128, (int64_t)128, (int64_t)-1000, (int64_t)4096, (int64_t)64, (int64_t)2048}) {
                    tiles += check_pair_plan(Tm, Tn, 1, doff, nullptr, false, 1, f, true); ++plans;
                }
            }
        }
    // the trailing updates of the headline step: A has 545 row tiles, every step starts 16 tiles further down, the
    // columns are the square part (rows below it: test rows and the y row ride along)
    for (int step = 0; step < 34; ++step) {
        const int64_t Tm = 545 - 16 * (step + 1), Tn = 512 - 16 * (step + 1);
        if (Tn <= 0) break;
        tiles += check_pair_plan(Tm, Tn, 1, 0, nullptr, false, 1, 0, true); ++plans;
        tiles += check_pair_plan(Tm, Tn, 1, 0, nullptr, false, 1, 0, false); ++plans;
    }
    for (int64_t T : {(int64_t)496, (int64_t)497, (int64_t)1008, (int64_t)1024}) {
        tiles += check_pair_plan(T, T, 1, 0, nullptr, false, 1, 0, true); ++plans;
        tiles += check_pair_plan(T, 16, 1, 0, nullptr, false, 1, 0, true); ++plans;
    }
    // row maps (staircases), with and without the host copy, bands of 1 .. 16 tiles (odd bands split pairs)
    for (int trial = 0; trial < 400; ++trial) {
        const int rbt = 1 << (rng() % 5);
        const int bands = 1 + rng() % 40;
        const int64_t Tm = (int64_t)bands * rbt - (rng() % rbt);
        const int64_t Tn = 1 + rng() % 300;
        std::vector<int32_t> map((size_t)bands);
        const int shape = rng() % 3;
        for (int q = 0; q < bands; ++q) {
            if (shape == 0) map[(size_t)q] = (int32_t)std::min<int64_t>(Tn * 128, (int64_t)(q + 1) * rbt * 128);
            else if (shape == 1) map[(size_t)q] = (int32_t)((rng() % (Tn + 1)) * 128);
            else map[(size_t)q] = (int32_t)((rng() % (Tn * 128 + 1)));
        }
        if (rng() % 8 == 0) map[rng() % map.size()] = 0;
        for (int f : forces) {
            if (f && ((Tm + f - 1) / f) > DMA_MAX_SM) continue;
            tiles += check_pair_plan(Tm, Tn, 0, 0, &map, true, rbt, f, true); ++plans;
            tiles += check_pair_plan(Tm, Tn, 0, 0, &map, false, rbt, f, true); ++plans;
        }
    }
    // pricing: a full pair plan of whole rounds is as efficient as the tile plan; a block with one live half costs two tiles
    {
        TilePlan p;
        CHECK(plan_tiles(p, 64, 64, 0, 0, false, nullptr, 0, 1, 8, false, true), "plan");
        CHECK(fabs(plan_xcd_efficiency(p, nullptr) - 1.0) < 1e-12, "full pair plan: %g", plan_xcd_efficiency(p, nullptr));
        CHECK(plan_tiles(p, 63, 64, 0, 0, false, nullptr, 0, 1, 8, false, true), "plan");
        CHECK(plan_xcd_efficiency(p, nullptr) < 63.0 / 64.0 + 1e-12, "half-dead pairs priced at two tiles: %g", plan_xcd_efficiency(p, nullptr));
    }
    if (g_fail) {
        printf("pair_plan_check: %d failures\n", g_fail);
        return 1;
    }
    printf("pair_plan_check: ok (%ld plans, %ld live tiles)\n", plans, tiles);
    return 0;
}
