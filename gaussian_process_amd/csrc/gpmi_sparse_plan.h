// The arithmetic of gpmi_sparse_fit that depends on the shapes alone: how the training rows are cut into slabs, how the
// Gram kernel (sparse.hip: gram_tn_kernel) cuts a slab's rows over workgroups, and how large the workspaces are that
// both need.  Host-only, no HIP types (plain g++ compiles it; tests/sanitize/sparse_plan_check.cpp holds it to brute
// force and prints the plan of a shape on request).
#pragma once
#include <algorithm>
#include <cstdint>

namespace gpmi {

constexpr int64_t SPARSE_TILE = 128;
constexpr int64_t GRAM_TARGET_GROUPS = 1024;   // workgroups a launch aims at: four per CU of a 256-CU chip
constexpr int64_t SPARSE_DEFAULT_SLAB = 16384;

// The launch plan of the Gram kernel, a function of the shapes alone: the slab's rows are cut into nsplit chunks of
// `chunk` rows (a multiple of 128; the last may be shorter) so that tiles x splits reaches GRAM_TARGET_GROUPS where the
// slab has the rows for it.  One lower tile (m <= 128) and a slab of 256 rows already give two splits.
struct GramPlan { int64_t ntiles, nsplit, chunk; };
inline GramPlan gram_plan(int64_t rows, int64_t mp) {
    const int64_t nt = mp / SPARSE_TILE, units = rows / SPARSE_TILE;
    GramPlan p;
    p.ntiles = nt * (nt + 1) / 2;
    const int64_t want = (GRAM_TARGET_GROUPS + p.ntiles - 1) / p.ntiles;
    int64_t ns = std::min(units, want);
    const int64_t cu = (units + ns - 1) / ns;
    p.nsplit = (units + cu - 1) / cu;
    p.chunk = cu * SPARSE_TILE;
    return p;
}

// doubles of the partial tiles one launch writes: a 128 x 128 tile per (lower tile, split)
inline int64_t gram_plan_doubles(int64_t rows, int64_t mp) {
    const GramPlan p = gram_plan(rows, mp);
    return p.ntiles * p.nsplit * SPARSE_TILE * SPARSE_TILE;
}

// The slabs of a fit of N training rows (Np padded) with m_p padded inducing columns under option "sparse_slab"
// (0: by size): nslabs - 1 slabs of S rows and one of last_rows <= S.
struct SparseSlabs {
    int64_t Np = 0, S = 0, nslabs = 0, last_rows = 0;
    int64_t part_doubles = 0;   // the Gram kernel's partial tiles, enough for every slab of the fit
    int64_t gemv_doubles = 0;   // the scratch of the transposed matrix-vector product (solve.hip: launch_gemv_t) on a slab
};
inline SparseSlabs sparse_slabs(int64_t N, int64_t slab_opt, int64_t mp) {
    auto up = [](int64_t x) { return (x + SPARSE_TILE - 1) / SPARSE_TILE * SPARSE_TILE; };
    SparseSlabs s;
    s.Np = up(N);
    s.S = std::min(s.Np, slab_opt ? up(slab_opt) : SPARSE_DEFAULT_SLAB);
    s.nslabs = (s.Np + s.S - 1) / s.S;
    // the last slab is shorter, and a shorter slab can have MORE splits than a full one (the chunk length is rounded)
    s.last_rows = s.Np % s.S ? s.Np % s.S : s.S;
    s.part_doubles = std::max(gram_plan_doubles(s.S, mp), gram_plan_doubles(s.last_rows, mp));
    s.gemv_doubles = ((s.S + 63) / 64) * mp;
    return s;
}

}  // namespace gpmi
