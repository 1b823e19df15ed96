// Which kernel a launch of the update GEMM  C -= A * B^T  reaches, with what geometry: gemm_route() below is the ONE
// place that decides it.  Free of any HIP dependency like gpmi_plan.h, whose plans it hands out: hipcc compiles it into
// the launchers (gemm_nt.hip: launch_gemm_nt switches over its answer), plain g++ under -fsanitize=address,undefined
// compiles it into tests/sanitize/gemm_route_check.cpp, where tests/test_gemm_route_cpu.py holds the route table of the
// GPU tests (tests/gemm_route_table.py) against it.
#pragma once
#include <stddef.h>
#include <stdint.h>

#include "gpmi_plan.h"

namespace gpmi {

// The options that select a GEMM kernel (gpmi_set_option; the first part of Tuning, gpmi_internal.h).
struct GemmTuning {
    int gemm_use_dma = 1;       // LDS-DMA GEMM for launches of at least GEMM_FEW_TILES tiles
    int gemm_small_tiles = 1;   // 64 x 64 tiles for launches with fewer
    int gemm_persist = 1;       // resident workgroups that chain the K loops of consecutive tiles (launches with >= 2 rounds of tiles)
    int gemm_ticket = 0;        // ticket form of the per-tile kernel (resident workgroups, tiles drawn from counters, no state across tiles): 1 Cholesky trailing updates under lookahead, 2 every launch of at least one round
    int gemm_balance = 1;       // per-tile launches: choose the supertile edge of mid-size triangular launches by the deal of blocks to the XCDs (gpmi_plan.h: plan_xcd_efficiency); 0: always the widest
    int gemm_dma_waves = 8;     // 4: one wave per SIMD, 8: two waves per SIMD (32 x 64 per wave)
    int gemm_tall = 1;          // per-tile launches of the 8-wave kernel: 1 256 x 128 blocks (two tiles, 64 x 64 per wave) for launches of at least tall_min_tiles live tiles, 0 128 x 128 always
    int tall_min_tiles = 12288; // see gemm_tall (below: N = 16384 one pass +1.3 % with the tall form, lookahead panels wait for twice-as-long workgroups) -- the bar of every launch outside Sharing::panel_slack
    int tall_min_tiles_slack = 1024;    // the same bar for launches under Sharing::panel_slack (a Cholesky of 49152 columns and more: its panel chain has 4-5x slack, nothing waits for the longer workgroups)
    int gemm_small_dma = 1;     // 1: deep-prefetch LDS-DMA kernel for launches with few tiles, 0: first-generation 64 x 64 kernel
    // timing-only ablation bits (gpmi_probe_gemm); results are wrong when non-zero.  Non-zero keeps small launches off
    // the 64 x 64 kernels; 1 .. 255 keeps a launch off the LDS-DMA kernels, >= 256 does not; the low byte selects the
    // probe instantiation (which receives it) and switches the resident forms off
    int gemm_dbg = 0;
};

// What else runs on the chip while the calling thread's launches do (thread-local: sharing(), SharingScope in
// gpmi_internal.h).  The results are the same bits in every state.
struct Sharing {
    // the panel kernels run beside a trailing update, whose workgroups hold 96 KiB of every CU's 160 KiB of LDS: small
    // GEMMs use the 3-stage ring, trsm128 its two-launch form, which fit next to them and start at once
    bool small_lds = false;
    // another stream or lane keeps part of the chip busy: no launch may take the whole chip for its whole length (the
    // persistent form stays off), and gemm_ticket == 1 applies to the trailing updates
    bool chip_shared = false;
    // the launch belongs to a factorisation whose lookahead panel chain is far off the critical path (cholesky_inplace
    // from 49152 columns up: ~9 ms of panel kernels per ~50 ms step): the 256 x 128 form from tall_min_tiles_slack
    // live tiles on instead of tall_min_tiles -- the next-block-column launches, the late trailing updates and the
    // updates inside the panel
    bool panel_slack = false;

    static Sharing alone() { return Sharing(); }
    static Sharing chip_shared_only() { Sharing s; s.chip_shared = true; return s; }
    static Sharing beside_update() { Sharing s; s.small_lds = s.chip_shared = true; return s; }
    Sharing and_chip_shared() const { Sharing s = *this; s.chip_shared = true; return s; }     // the others as they are
    Sharing large_lds() const { Sharing s = *this; s.small_lds = false; return s; }            // the others as they are
    Sharing with_panel_slack(bool on) const { Sharing s = *this; s.panel_slack = on; return s; }
};

// Every kernel symbol a launch can reach.  Trail: the same code under the Cholesky trailing update's own symbol
// (role 1); Probe: the instantiation that honours the ablation bits.
enum class GemmKernel {
    Nothing,        // no work: an empty shape, or a row map without a live supertile (success)
    Invalid,        // unusable arguments (hipErrorInvalidValue)
    Reg64, Reg128x64, Reg128, Reg128Probe,                 // gemm_nt.hip: first generation, staging through registers
    Small8, Small3,                                         // gemm_dma.hip: 64 x 64 tiles, deep LDS-DMA ring
    Dma4, Dma4Probe, Dma8, Dma8Probe, Dma8Trail,            // gemm_dma.hip: one workgroup per 128 x 128 tile
    Tall, TallProbe, TallTrail,                             // ... per 256 x 128 pair of tiles
    Persist, PersistTrail, Ticket, TicketTrail,             // ... resident workgroups that draw tiles from counters
};

// the symbol as a kernel trace prints it
inline const char* gemm_kernel_name(GemmKernel k) {
    switch (k) {
        case GemmKernel::Nothing: return "nothing";
        case GemmKernel::Invalid: return "invalid";
        case GemmKernel::Reg64: return "gemm_nt_kernel<2, 2, false>";
        case GemmKernel::Reg128x64: return "gemm_nt_kernel<4, 2, false>";
        case GemmKernel::Reg128: return "gemm_nt_kernel<4, 4, false>";
        case GemmKernel::Reg128Probe: return "gemm_nt_kernel<4, 4, true>";
        case GemmKernel::Small8: return "gemm_nt_small_kernel<8>";
        case GemmKernel::Small3: return "gemm_nt_small_kernel<3>";
        case GemmKernel::Dma4: return "gemm_nt_dma_kernel<4, false>";
        case GemmKernel::Dma4Probe: return "gemm_nt_dma_kernel<4, true>";
        case GemmKernel::Dma8: return "gemm_nt_dma_kernel<2, false>";
        case GemmKernel::Dma8Probe: return "gemm_nt_dma_kernel<2, true>";
        case GemmKernel::Dma8Trail: return "chol_trailing_update_dma_kernel";
        case GemmKernel::Tall: return "gemm_nt_dma_tall_kernel<false>";
        case GemmKernel::TallProbe: return "gemm_nt_dma_tall_kernel<true>";
        case GemmKernel::TallTrail: return "chol_trailing_update_dma256_kernel";
        case GemmKernel::Persist: return "gemm_nt_dma_persist_kernel";
        case GemmKernel::PersistTrail: return "chol_trailing_update_persist_kernel";
        case GemmKernel::Ticket: return "gemm_nt_dma_ticket_kernel";
        case GemmKernel::TicketTrail: return "chol_trailing_update_ticket_kernel";
    }
    return "?";
}

// the kernels of the 128-tile LDS-DMA family (they take a TilePlan; the roofline figures are theirs)
inline bool gemm_kernel_is_dma(GemmKernel k) { return k >= GemmKernel::Dma4; }

// What the decision depends on, and nothing else.
struct GemmRouteIn {
    int64_t M = 0, N = 0, K = 0;
    int mode = 0, lower = 0;
    int64_t diag_off = 0;
    bool has_row_map = false;                   // the launch has a device row map ...
    const int32_t* row_ncols_host = nullptr;    // ... its host copy (or null) ...
    int row_bands = 0;                          // ... of this many bands
    int row_block_tiles = 1;
    bool b_blocks = false;                      // B is a table of row blocks ...
    int64_t b_block_rows = 0;                   // ... of this many rows each
    int role = 0;                               // 1: Cholesky trailing update
    GemmTuning tune;
    Sharing sharing;
    // resident workgroups the device offers (0: no pool).  GROUPS_NOT_ASKED: gemm_route answers asks_groups instead of
    // a kernel when -- and only when -- the launch wants a resident form, so that only such a launch creates the pool
    int groups = 0;
};
constexpr int GROUPS_NOT_ASKED = -1;

struct GemmRoute {
    GemmKernel kernel = GemmKernel::Invalid;
    bool asks_groups = false;   // see GemmRouteIn::groups: call again with the pool's group count
    TilePlan plan;              // LDS-DMA family: the plan to launch with
    unsigned grid = 0;          // workgroups (first generation: 0, the supertile loop of gemm_nt.hip: plan sets it)
    size_t lds = 0;             // dynamic LDS, bytes
};

constexpr int64_t GEMM_FEW_TILES = 128;            // from half a round of 128 x 128 tiles up: the LDS-DMA family; below: 64 x 64 tiles
constexpr int64_t GEMM_PERSIST_MIN_K = 256;        // a K loop long enough to draw the successor tile in
constexpr size_t GEMM_DMA_LDS = (size_t)3 * (PLAN_TILE + PLAN_TILE) * 8 * 16;     // three stages of A and B tile, 16 columns each: 96 KiB
constexpr size_t GEMM_TALL_LDS = (size_t)2 * (2 * PLAN_TILE + PLAN_TILE) * 8 * 16;   // two stages of two A tiles and a B tile: 96 KiB
constexpr size_t GEMM_SMALL_STAGE = (size_t)(64 + 64) * 8 * 16;                   // one stage of the 64 x 64 ring: 16 KiB
constexpr size_t gemm_reg_lds(int TM, int TN) { return (size_t)2 * (8 * TM + 8 * TN) * 16; }   // first generation: two stages

inline void gemm_route(const GemmRouteIn& in, GemmRoute& r) {
    const GemmTuning& tn = in.tune;
    r.asks_groups = false;
    auto done = [&r](GemmKernel k, unsigned grid, size_t lds) { r.kernel = k; r.grid = grid; r.lds = lds; };
    if (in.M <= 0 || in.N <= 0 || in.K <= 0) return done(GemmKernel::Nothing, 0, 0);
    if (in.M % 128 || in.N % 64 || in.K % 16) return done(GemmKernel::Invalid, 0, 0);
    // the LDS-DMA family subtracts whole 128 x 128 tiles and keeps two K steps in flight
    const bool dma_ok = in.mode == 0 && in.N % 128 == 0 && in.K >= 32;
    if (in.b_blocks && !dma_ok) return done(GemmKernel::Invalid, 0, 0);       // only that family reads B through a block table
    const int low = tn.gemm_dbg & 0xff;
    const bool few = (in.M / 128) * ((in.N + 127) / 128) < GEMM_FEW_TILES;
    if (!in.b_blocks && !(tn.gemm_use_dma && (!tn.gemm_dbg || tn.gemm_dbg >= 256) && dma_ok && !few)) {
        // few tiles: one 128 x 128 tile keeps a CU busy for 1.8 us per 64 of K while the rest of the chip idles --
        // 64 x 64 tiles finish 4x sooner (panel-internal updates, diagonal blocks)
        if (tn.gemm_small_tiles && !tn.gemm_dbg && few) {
            if (tn.gemm_small_dma && in.mode == 0 && !in.has_row_map)
                return in.sharing.small_lds ? done(GemmKernel::Small3, (unsigned)((in.M / 64) * (in.N / 64)), 3 * GEMM_SMALL_STAGE)
                                            : done(GemmKernel::Small8, (unsigned)((in.M / 64) * (in.N / 64)), 8 * GEMM_SMALL_STAGE);
            return done(GemmKernel::Reg64, 0, gemm_reg_lds(64, 64));
        }
        if (in.N % 128) return done(GemmKernel::Reg128x64, 0, gemm_reg_lds(128, 64));
        return done(tn.gemm_dbg ? GemmKernel::Reg128Probe : GemmKernel::Reg128, 0, gemm_reg_lds(128, 128));
    }
    if (in.b_blocks && (in.b_block_rows <= 0 || in.b_block_rows % 128)) return done(GemmKernel::Invalid, 0, 0);
    const int64_t Tm = in.M / 128, Tn = in.N / 128;
    auto plan = [&](bool balance, bool pair) {
        return plan_tiles(r.plan, Tm, Tn, in.lower, in.diag_off, in.has_row_map, in.row_ncols_host, in.row_bands,
                          in.row_block_tiles, 0, balance, pair);
    };
    // first as a resident form wants it (widest supertiles: resident workgroups take over each other's tails), which
    // also decides whether one is used
    if (!plan(false, false)) return done(GemmKernel::Invalid, 0, 0);
    if (r.plan.nsuper == 0) return done(GemmKernel::Nothing, 0, 0);
    const bool eight = tn.gemm_dma_waves == 8;
    const bool want_ticket = eight && !low && (tn.gemm_ticket >= 2 || (tn.gemm_ticket == 1 && in.role == 1 && in.sharing.chip_shared));
    // persistent form: launches with at least two rounds of tiles and a K loop long enough to draw the successor in --
    // and the chip to themselves: resident workgroups (216 registers per lane, two waves per SIMD) leave no room on a
    // CU for the panel kernels of the other stream, which would then wait for the whole launch instead of a tile
    // (lookahead with both forms: N = 16384 fit + predict 39.8 against 42.9 ms)
    const bool want_persist = eight && !low && tn.gemm_persist && in.K >= GEMM_PERSIST_MIN_K && !in.sharing.chip_shared;
    if (want_ticket || want_persist) {
        if (in.groups == GROUPS_NOT_ASKED) { r.asks_groups = true; return; }
        const bool trail = in.role == 1;
        if (want_ticket && in.groups > 0 && r.plan.nblocks >= in.groups)
            return done(trail ? GemmKernel::TicketTrail : GemmKernel::Ticket, (unsigned)in.groups, GEMM_DMA_LDS + 16);     // ring + mailbox
        if (want_persist && in.groups > 0 && r.plan.nblocks >= 2 * in.groups)
            return done(trail ? GemmKernel::PersistTrail : GemmKernel::Persist, (unsigned)in.groups, GEMM_DMA_LDS + 16);
    }
    // one workgroup per block (no pool, or too few blocks for a resident form: the same bits): the supertile edge is
    // chosen with the static deal of blocks to the XCDs in mind.  256 x 128 blocks, as a pair plan with the same
    // supertiles, for launches of the 8-wave kernel with enough live tiles (the bar: tall_min_tiles, or the lower
    // tall_min_tiles_slack where no panel chain waits for the longer workgroups)
    const bool balance = tn.gemm_balance != 0;
    const int tall_bar = in.sharing.panel_slack ? tn.tall_min_tiles_slack : tn.tall_min_tiles;
    const bool tall = eight && tn.gemm_tall &&
                      plan_live_tiles(Tm, Tn, in.lower, in.diag_off, in.row_ncols_host, in.row_bands, in.row_block_tiles) >= tall_bar;
    if ((balance || tall) && !plan(balance, tall)) return done(GemmKernel::Invalid, 0, 0);
    const GemmKernel trail_or = !eight ? GemmKernel::Dma4 : in.role == 1 ? (tall ? GemmKernel::TallTrail : GemmKernel::Dma8Trail)
                                                                         : (tall ? GemmKernel::Tall : GemmKernel::Dma8);
    const GemmKernel probe = !eight ? GemmKernel::Dma4Probe : tall ? GemmKernel::TallProbe : GemmKernel::Dma8Probe;
    return done(low ? probe : trail_or, (unsigned)r.plan.nblocks, tall ? GEMM_TALL_LDS : GEMM_DMA_LDS);
}

inline GemmRoute gemm_route(const GemmRouteIn& in) {
    GemmRoute r;
    gemm_route(in, r);
    return r;
}

}  // namespace gpmi
