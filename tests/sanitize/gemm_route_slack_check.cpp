// TEST INFRASTRUCTURE: gemm_route (gaussian_process_amd/csrc/gpmi_route.h) asked from the command line like
// gemm_route_check.cpp, with the third sharing flag in front, built with g++ -fsanitize=address,undefined by
// tests/test_gemm_route_slack_cpu.py.  One query per line of standard input:
//     panel_slack  groups small_lds chip_shared role  nopts (name value)*  M N K lower diag_off row_block_tiles host_copy b_block_rows  nreach reach*
// The answer is one line: the kernel's name.  For an answer of the LDS-DMA family the plan and the grid are held against
// plan_tiles: a pair plan for the 256 x 128 form and only for it, grid = the plan's blocks for one workgroup per block.
#include <cstdio>
#include <iostream>
#include <sstream>
#include <string>
#include <vector>

#include "gpmi_route.h"

using namespace gpmi;

static int* option(GemmTuning& t, const std::string& name) {
    if (name == "gemm_dma") return &t.gemm_use_dma;
    if (name == "gemm_small_tiles") return &t.gemm_small_tiles;
    if (name == "gemm_small_dma") return &t.gemm_small_dma;
    if (name == "gemm_persist") return &t.gemm_persist;
    if (name == "gemm_ticket") return &t.gemm_ticket;
    if (name == "gemm_balance") return &t.gemm_balance;
    if (name == "gemm_dma_waves") return &t.gemm_dma_waves;
    if (name == "gemm_tall") return &t.gemm_tall;
    if (name == "tall_min_tiles") return &t.tall_min_tiles;
    if (name == "tall_min_tiles_slack") return &t.tall_min_tiles_slack;
    if (name == "gemm_dbg") return &t.gemm_dbg;
    return nullptr;
}

int main() {
    std::string line;
    while (std::getline(std::cin, line)) {
        if (line.empty()) continue;
        std::istringstream is(line);
        GemmRouteIn in;
        int p = 0, s = 0, b = 0, nopts = 0, host = 0, nreach = 0;
        is >> p >> in.groups >> s >> b >> in.role >> nopts;
        in.sharing.panel_slack = p != 0;
        in.sharing.small_lds = s != 0;
        in.sharing.chip_shared = b != 0;
        for (int i = 0; i < nopts; ++i) {
            std::string name;
            int value = 0;
            is >> name >> value;
            int* f = option(in.tune, name);
            if (!f) { fprintf(stderr, "FAIL: no option %s\n", name.c_str()); return 2; }
            *f = value;
        }
        is >> in.M >> in.N >> in.K >> in.lower >> in.diag_off >> in.row_block_tiles >> host >> in.b_block_rows >> nreach;
        std::vector<int32_t> reach((size_t)nreach);
        for (int32_t& v : reach) is >> v;
        if (!is) { fprintf(stderr, "FAIL: cannot read query: %s\n", line.c_str()); return 2; }
        in.has_row_map = nreach > 0;
        if (in.has_row_map && host) { in.row_ncols_host = reach.data(); in.row_bands = nreach; }
        in.b_blocks = in.b_block_rows != 0;
        const int groups = in.groups;
        in.groups = GROUPS_NOT_ASKED;
        GemmRoute r = gemm_route(in);
        if (r.asks_groups) {
            in.groups = groups;
            r = gemm_route(in);
        }
        if (r.asks_groups) { fprintf(stderr, "FAIL: asked for the groups twice: %s\n", line.c_str()); return 1; }
        if (gemm_kernel_is_dma(r.kernel)) {
            const bool resident = r.kernel >= GemmKernel::Persist;
            const bool tall = r.kernel == GemmKernel::Tall || r.kernel == GemmKernel::TallProbe || r.kernel == GemmKernel::TallTrail;
            TilePlan want;
            const bool ok = plan_tiles(want, in.M / 128, in.N / 128, in.lower, in.diag_off, in.has_row_map, in.row_ncols_host,
                                       in.row_bands, in.row_block_tiles, 0, resident ? false : in.tune.gemm_balance != 0, tall);
            const unsigned grid = resident ? (unsigned)groups : (unsigned)want.nblocks;
            if (!ok || want.pair != r.plan.pair || want.nblocks != r.plan.nblocks || want.nsuper != r.plan.nsuper || want.S != r.plan.S ||
                r.grid != grid || r.grid == 0 || r.lds != (size_t)96 * 1024 + (resident ? 16 : 0)) {
                fprintf(stderr, "FAIL: %s: plan, grid %u (want %u) or LDS %zu of %s\n", line.c_str(), r.grid, grid, r.lds,
                        gemm_kernel_name(r.kernel));
                return 1;
            }
        }
        printf("%s\n", gemm_kernel_name(r.kernel));
    }
    return 0;
}
