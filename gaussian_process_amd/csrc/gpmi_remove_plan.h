// The arithmetic of gpmi_remove: which indices each sweep takes out, where a sweep starts, how many launches it is, where
// the y row goes and how many bytes move.  Host-only, no HIP types (plain g++ compiles it;
// tests/sanitize/remove_plan_check.cpp holds it to brute force).
//
// Taking index j out of a fit leaves the rows and columns before j as they are, drops row j, and turns the trailing factor
// into chol(L33 L33^T + l l^T) with l the part of column j below the diagonal: a POSITIVE rank-one update.  With
// J0 = floor(min(idx) / 128) 128 the leading J0 x J0 square of the factor (whole 128 x 128 tiles, their stored 16 x 16
// inverses included) is the resident one bit for bit; everything from J0 on is rewritten, shifted up and left by the
// number of removed indices in front of it.
//
// One sweep carries at most REMOVE_MAX = 16 removed columns as active vectors.  More indices are taken in DESCENDING
// groups of the sorted list -- the 16 largest first, the remainder (the smallest) last: positions of indices still
// pending stay valid while larger ones go, and each sweep starts as late (J0 as large) as possible.
//
// Storage: the result keeps the resident allocation's leading dimension and rows (a removal never shrinks it, so a
// remove-k / append-k cycle stops reallocating once the append has grown it); every sweep writes out of place into a
// second buffer of the same shape; the y row moves to row Np' = ceil(N' / 128) 128 of it.
#pragma once
#include <algorithm>
#include <cstdint>
#include <vector>

namespace gpmi {

constexpr int64_t REMOVE_TILE = 128;
constexpr int64_t REMOVE_MAX = 16;          // active vectors of one sweep (registers of a lane)

struct RemoveSweep {
    int64_t first = 0, count = 0;    // the sweep removes sorted[first .. first + count)
    int64_t N_in = 0, N_out = 0;     // points before and after
    int64_t Np_in = 0, Np_out = 0;   // padded sizes
    int64_t J0 = 0;                  // rows and columns below J0 move with one 2-D copy
    int64_t blocks = 0;              // old 128-column blocks from J0 on: (Np_in - J0) / 128
    int64_t launches = 0;            // blocks + 1: one per block and the one that finishes the y row
    int64_t yrow_in = 0, yrow_out = 0;
    bool yrow_moves = false;         // Np_out != the row the y row came from
    int64_t copy_bytes = 0;          // the 2-D copy: J0 x J0 doubles
    int64_t stream_bytes = 0;        // the old trailing trapezoid, rows [J0, Np_in), whole 128 x 128 blocks, read once
};

struct RemovePlan {
    bool ok = false;
    const char* why = "";            // the refusal's text when !ok
    std::vector<int64_t> sorted;     // the indices, ascending
    std::vector<RemoveSweep> sweeps; // in the order they run
    int64_t N_out = 0, Np_out = 0, yrow_out = 0;
    int64_t ld = 0, rows = 0;        // layout afterwards: the resident one
    int64_t first_tile = 0;          // J0 / 16: the 16 x 16 diagonal tiles from here on get new inverses (the sweep writes
                                     // lower triangles only, so the tiles between J0 and min(idx) are among them)
    int64_t J0 = 0;                  // floor(min(idx) / 128) 128: the bit-exact part of the whole call
};

inline int64_t remove_round_up(int64_t x) { return (x + REMOVE_TILE - 1) / REMOVE_TILE * REMOVE_TILE; }

// N: resident points.  idx, k: the positions to remove, any order.  ld, rows_cap, yrow: the resident layout.  ld_pad:
// the context's option (the factor's columns are those left of the pad).
inline RemovePlan remove_plan(int64_t N, const int64_t* idx, int64_t k, int64_t ld, int64_t rows_cap, int64_t yrow,
                              int64_t ld_pad) {
    RemovePlan p;
    if (!idx) { p.why = "gpmi_remove: null index list"; return p; }
    if (k < 1) { p.why = "gpmi_remove: k must be at least 1"; return p; }
    if (k >= N) { p.why = "gpmi_remove: k must be smaller than N (at least one point stays)"; return p; }
    p.sorted.assign(idx, idx + k);
    std::sort(p.sorted.begin(), p.sorted.end());
    if (p.sorted.front() < 0 || p.sorted.back() >= N) { p.why = "gpmi_remove: an index outside [0, N)"; p.sorted.clear(); return p; }
    for (int64_t i = 1; i < k; ++i)
        if (p.sorted[(size_t)i] == p.sorted[(size_t)i - 1]) { p.why = "gpmi_remove: a duplicate index"; p.sorted.clear(); return p; }
    if (remove_round_up(N) > ld - ld_pad || remove_round_up(N) + REMOVE_TILE > rows_cap) {
        p.why = "gpmi_remove: the resident layout does not hold the resident fit";
        p.sorted.clear();
        return p;
    }
    p.ok = true;
    p.ld = ld;
    p.rows = rows_cap;
    p.J0 = p.sorted.front() / REMOVE_TILE * REMOVE_TILE;
    p.first_tile = p.J0 / 16;
    int64_t n = N, yr = yrow, end = k;
    while (end > 0) {
        RemoveSweep s;
        s.count = std::min(end, REMOVE_MAX);
        s.first = end - s.count;
        s.N_in = n;
        s.N_out = n - s.count;
        s.Np_in = remove_round_up(s.N_in);
        s.Np_out = remove_round_up(s.N_out);
        s.J0 = p.sorted[(size_t)s.first] / REMOVE_TILE * REMOVE_TILE;
        s.blocks = (s.Np_in - s.J0) / REMOVE_TILE;
        s.launches = s.blocks + 1;
        s.yrow_in = yr;
        s.yrow_out = s.Np_out;
        s.yrow_moves = s.yrow_out != s.yrow_in;
        s.copy_bytes = s.J0 * s.J0 * 8;
        const int64_t b0 = s.J0 / REMOVE_TILE, b1 = s.Np_in / REMOVE_TILE;
        s.stream_bytes = (b1 * (b1 + 1) / 2 - b0 * (b0 + 1) / 2) * REMOVE_TILE * REMOVE_TILE * 8;
        p.sweeps.push_back(s);
        n = s.N_out;
        yr = s.yrow_out;
        end = s.first;
    }
    p.N_out = n;
    p.Np_out = remove_round_up(n);
    p.yrow_out = yr;
    return p;
}

}  // namespace gpmi
