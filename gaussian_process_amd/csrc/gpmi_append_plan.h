// The arithmetic of gpmi_append: which rows of the resident factor an append of k points touches, which route builds
// them, whether the resident allocation takes them, and how many bytes move.  Host-only, no HIP types (plain g++ compiles
// it; tests/sanitize/append_plan_check.cpp holds it to brute force).
//
// The factor of a leading principal submatrix is the leading block of the factor, and everything is stored in 128 x 128
// tiles with identity padding: with N0 = floor(N / 128) 128 the rows and columns below N0 of a fit of N points are those
// of a fit of N + k points bit for bit.  The BORDER is what is left: rows [N0, Np'), Np' = ceil((N + k) / 128) 128 --
// the old tail rows (their columns left of N0 are final too, their own tile is not: the new points change its padding),
// the new rows and the new padding.
//
//   W = K(border, X[0:N0]) L0^-T          skinny: only the k new rows, by the <= 16-row sweep kernel; padded: all
//                                          border rows, by the 128-row TRSM sweep
//   S = K_bb + noise I - W W^T,  m_b = y_b - m_0 W^T      one rank-N0 update of the border block and the y row
//   L_bb = chol(S) with the y row carried
//
// Storage: A is `rows_cap` rows of `ld` doubles; columns [0, ld - ld_pad) are the factor's (option "reserve" makes them
// more than Np), the y row's 128-row block follows the last row of the factor.  An append works in place when Np'
// columns and Np' + 128 rows fit; otherwise A is allocated anew with the layout a fresh fit of N + k points would choose
// and the leading N0 x N0 square (whole tiles: the stored 16 x 16 inverses travel with it) moves with one 2-D copy.
#pragma once
#include <cstdint>

namespace gpmi {

constexpr int64_t APPEND_TILE = 128;
constexpr int64_t APPEND_SKINNY_MAX = 16;      // rows of the skinny sweep kernel (one MFMA operand)

struct AppendPlan {
    int64_t N1 = 0;            // N + k
    int64_t N0 = 0;            // leading rows / columns that stay as they are
    int64_t Np = 0, Np1 = 0;   // padded sizes before and after
    int64_t border = 0;        // Np1 - N0 rows (and columns) are rebuilt or added
    bool skinny = false;       // W through the <= 16-row kernel (new rows only) instead of the padded 128-row sweep
    bool in_place = false;     // the resident allocation takes the result at its leading dimension
    bool yrow_moves = false;   // the y row leaves row yrow for row Np1
    int64_t ld = 0, rows = 0;  // layout afterwards: leading dimension, rows of A (y block included)
    int64_t yrow = 0;          // = Np1
    int64_t keep_rows = 0;     // a reallocation copies rows [0, keep_rows) x columns [0, N0): N0, or N when the old tail rows stay
    // traffic, for the rate script and the documents
    int64_t copy_bytes = 0;    // the 2-D copy of a reallocation (0 in place)
    int64_t sweep_bytes = 0;   // L streamed once by the sweep: the lower triangle of N0 x N0, whole 128 x 128 blocks
    int64_t build_rows = 0;    // rows of K(., X[0:N0]) built: k (skinny) or border (padded)
};

inline int64_t append_round_up(int64_t x) { return (x + APPEND_TILE - 1) / APPEND_TILE * APPEND_TILE; }

// N, k: resident and new points.  ld, rows_cap, yrow: the resident layout (the standard one has yrow == Np).  ld_pad,
// reserve: the context's options.  fused: the resident factor carries the 16 x 16 inverses (the skinny kernel needs
// them).  skinny_opt: option "append_skinny", -1 by size, 0 never, 1 whenever allowed.
inline AppendPlan append_plan(int64_t N, int64_t k, int64_t ld, int64_t rows_cap, int64_t yrow, int64_t ld_pad,
                              int64_t reserve, int fused, int skinny_opt) {
    AppendPlan p;
    p.N1 = N + k;
    p.Np = append_round_up(N);
    p.Np1 = append_round_up(p.N1);
    p.N0 = N / APPEND_TILE * APPEND_TILE;
    p.border = p.Np1 - p.N0;
    const bool allowed = k <= APPEND_SKINNY_MAX && fused && p.N0 > 0;
    // by size: the skinny route wherever it is allowed (profiles/r14_append_rate.txt: it wins at every measured size)
    p.skinny = allowed && skinny_opt != 0;
    p.in_place = p.Np1 <= ld - ld_pad && p.Np1 + APPEND_TILE <= rows_cap;
    p.yrow = p.Np1;
    p.yrow_moves = p.yrow != yrow;
    if (p.in_place) {
        p.ld = ld;
        p.rows = rows_cap;
    } else {
        const int64_t cap = append_round_up(p.N1 + reserve);
        p.ld = cap + ld_pad;
        p.rows = cap + APPEND_TILE;
        p.keep_rows = p.skinny ? N : p.N0;
        p.copy_bytes = p.keep_rows * p.N0 * 8;
    }
    const int64_t nblk = p.N0 / APPEND_TILE;
    p.sweep_bytes = nblk * (nblk + 1) / 2 * APPEND_TILE * APPEND_TILE * 8;
    p.build_rows = p.skinny ? k : p.border;
    return p;
}

}  // namespace gpmi
