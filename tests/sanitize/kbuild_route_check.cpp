// TEST INFRASTRUCTURE: rbf_route and rbf_tri_tile (gaussian_process_amd/csrc/gpmi_kroute.h) asked from the command
// line, built with g++ -fsanitize=address,undefined by tests/test_kbuild_route_cpu.py.  One query per line of standard
// input:
//     kind d nA nB nrows ncols symmetric row0 coef max_sq rbf_blocks
// (coef and max_sq as C hexadecimal floats).  The answer is one line:
//     kernel's name|tri strip nitems grid lds nocheck  interior edge diag skipped
// the last four being the tiles of each form the launch computes and the work items of the register kernel without a
// live tile.  On the way every answer is held against a direct count: the tiles a launch must compute are those of the
// Tm x Tn rectangle that reach the lower triangle (all of them when the launch is not symmetric); walking the grid the
// way the kernels do (rbf.hip: rbf_map_tile for one workgroup per tile, the persistent item loop of rbf_regs_kernel)
// must produce each of them exactly once and nothing else, and strip, nitems and the grid must be what their
// definitions say.  The line "tri" instead checks the triangular enumeration by brute force for every Tm <= 1024.
// A failure prints FAIL and exits non-zero.
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <iostream>
#include <sstream>
#include <string>
#include <vector>

#include "gpmi_kroute.h"

using namespace gpmi;

static int fail(const std::string& line, const char* what) {
    fprintf(stderr, "FAIL: %s: %s\n", line.c_str(), what);
    return 1;
}

// every s < Tm (Tm + 1) / 2 gives a tile of the lower triangle, in row-major order: each exactly once
static int check_tri() {
    const int T = 1024;
    int s = 0;
    for (int ti = 0; ti < T; ++ti)
        for (int tj = 0; tj <= ti; ++tj, ++s) {
            int gi = -1, gj = -1;
            rbf_tri_tile(s, gi, gj);
            if (gi != ti || gj != tj) {
                fprintf(stderr, "FAIL: rbf_tri_tile(%d) = (%d, %d), want (%d, %d)\n", s, gi, gj, ti, tj);
                return 1;
            }
        }
    // the prefix of the first Tm rows is the whole enumeration of a Tm-tile launch: its length is Tm (Tm + 1) / 2
    for (int Tm = 1; Tm <= T; ++Tm) {
        int gi, gj;
        rbf_tri_tile(Tm * (Tm + 1) / 2 - 1, gi, gj);
        if (gi != Tm - 1 || gj != Tm - 1) { fprintf(stderr, "FAIL: last tile of Tm = %d\n", Tm); return 1; }
    }
    printf("tri ok %d\n", s);
    return 0;
}

int main() {
    std::string line;
    while (std::getline(std::cin, line)) {
        if (line.empty()) continue;
        if (line == "tri") {
            if (check_tri()) return 1;
            continue;
        }
        std::istringstream is(line);
        int kind = 0, symmetric = 0, rbf_blocks = 0;
        long long d = 0, nA = 0, nB = 0, nrows = 0, ncols = 0, row0 = 0;
        std::string coef_s, max_sq_s;
        is >> kind >> d >> nA >> nB >> nrows >> ncols >> symmetric >> row0 >> coef_s >> max_sq_s >> rbf_blocks;
        if (!is) return fail(line, "cannot read the query");
        const double coef = strtod(coef_s.c_str(), nullptr), max_sq = strtod(max_sq_s.c_str(), nullptr);
        const RbfRoute r = rbf_route(kind, d, nrows, ncols, symmetric, row0, coef, max_sq, rbf_blocks);
        char name[48];
        rbf_kernel_name(r, name);
        if (r.kernel == RbfKernel::Nothing || r.kernel == RbfKernel::Invalid) {
            printf("%s|0 0 0 0 0 0  0 0 0 0\n", name);
            continue;
        }
        const int Tm = (int)(nrows / RBF_TILE), Tn = (int)(ncols / RBF_TILE);
        if (r.Tm != Tm || r.Tn != Tn) return fail(line, "Tm, Tn");
        const int tri = (symmetric && row0 == 0 && Tm == Tn) ? 1 : 0;
        if (r.tri != tri) return fail(line, "tri");
        // the tiles the launch owes
        auto live = [&](int ti, int tj) { return !symmetric || (long long)tj * RBF_TILE <= row0 + (long long)ti * RBF_TILE; };
        std::vector<int> seen((size_t)Tm * Tn, 0);
        long long nlive = 0;
        for (int ti = 0; ti < Tm; ++ti)
            for (int tj = 0; tj < Tn; ++tj) nlive += live(ti, tj);
        const long long nblk = tri ? (long long)Tm * (Tm + 1) / 2 : (long long)Tm * Tn;
        if (tri && nblk != nlive) return fail(line, "a triangular launch owes exactly the triangle");
        long long skipped = 0;
        if (r.kernel == RbfKernel::Regs) {
            const int strip = nblk >= 4096 ? 4 : 1;
            const int strips = (Tm + strip - 1) / strip;
            if (r.strip != strip || r.nitems != strips * Tn) return fail(line, "strip or nitems");
            if (r.grid != (unsigned)std::min<long long>(r.nitems, rbf_blocks) || r.grid == 0) return fail(line, "grid");
            if (r.lds != 0 || r.D != (int)d) return fail(line, "D or LDS");
            // rbf_regs_kernel's item loop, block by block
            const int row_tile0 = (int)(row0 / RBF_TILE);
            for (unsigned b = 0; b < r.grid; ++b)
                for (int item = (int)b; item < r.nitems; item += (int)r.grid) {
                    const int sy = item / Tn, tj = item - sy * Tn;
                    int ta = sy * r.strip;
                    const int tb = std::min(ta + r.strip, Tm);
                    if (symmetric) ta = std::max(ta, tj - row_tile0);
                    if (ta >= tb) { ++skipped; continue; }
                    for (int ti = ta; ti < tb; ++ti) ++seen[(size_t)ti * Tn + tj];
                }
        } else {
            if (r.grid != (unsigned)nblk) return fail(line, "grid");
            const size_t lds = r.kernel == RbfKernel::Lds ? (size_t)2 * RBF_TILE * (size_t)d * 8 : 0;
            if (r.lds != lds || lds > 64 * 1024) return fail(line, "LDS");
            // rbf_map_tile, workgroup by workgroup
            for (unsigned s = 0; s < r.grid; ++s) {
                int ti, tj;
                if (tri) rbf_tri_tile((int)s, ti, tj);
                else { ti = (int)s / Tn; tj = (int)s - ti * Tn; }
                if (ti < 0 || ti >= Tm || tj < 0 || tj >= Tn) return fail(line, "a workgroup maps outside the launch");
                if (live(ti, tj)) ++seen[(size_t)ti * Tn + tj];
            }
        }
        long long interior = 0, edge = 0, diag = 0;
        for (int ti = 0; ti < Tm; ++ti)
            for (int tj = 0; tj < Tn; ++tj) {
                if (seen[(size_t)ti * Tn + tj] != (live(ti, tj) ? 1 : 0)) return fail(line, "a tile computed twice, a live tile missed or a dead one computed");
                if (!live(ti, tj)) continue;
                const long long grow0 = row0 + (long long)ti * RBF_TILE, gcol0 = (long long)tj * RBF_TILE;
                const bool inside = grow0 + RBF_TILE <= nA && gcol0 + RBF_TILE <= nB;
                const bool on_diag = symmetric && gcol0 + RBF_TILE > grow0;
                if (on_diag) ++diag;
                else if (inside) ++interior;
                else ++edge;
            }
        printf("%s|%d %d %d %u %zu %d  %lld %lld %lld %lld\n", name, r.tri, r.strip, r.nitems, r.grid, r.lds, r.nocheck, interior, edge,
               diag, skipped);
    }
    return 0;
}
