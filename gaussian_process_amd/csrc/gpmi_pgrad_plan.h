// The arithmetic of gpmi_predict_grad_resident: which route forms W = V L^-1 (row i: w_i = L^-T v_i = K_y^-1 k*_i) for
// the variance's gradient, how large its buffer is and what the route streams.  Host-only, no HIP types (plain g++
// compiles it; tests/sanitize/pgrad_plan_check.cpp holds it to brute force).
//
//   sweep route     a copy of v swept backwards by launch_back_sweep: O(N^2 n), one launch per 128 columns, L's lower
//                   triangle streamed once per 16-row group.  Needs the 16 x 16 tile inverses: a fused factor only.
//   inverse route   U = L^-T by the forward sweep on the identity (N^3 / 3, the gradients' buffer), W = V U^T by the
//                   routed GEMM.  Serves a first-generation factor, and large n.
//   none            dvar was not asked for: nothing is swept, no buffer.
#pragma once
#include <cstdint>

namespace gpmi {

constexpr int64_t PGRAD_TILE = 128;
constexpr int64_t PGRAD_GROUP = 16;            // rows of one MFMA operand: a row group of the backward sweep
// Largest n that takes the sweep route under "by size": the largest measured n at which the sweep is the faster route
// at N = 16384, d = 8 (profiles/r17_predgrad_rate.txt, ms, sweep / inverse: n = 16 3.02 / 31.8, 128 4.05 / 31.9, 1024
// 16.9 / 37.9, 4096 62.2 / 62.7 -- a margin of 0.8 % there; at N = 65536 the sweep wins 947 / 1922 at n = 4096, at
// N = 4096 it loses 4.79 / 3.80 at n = 4096 and wins below).  Nothing beyond n = 4096 is measured: the inverse route.
constexpr int64_t PGRAD_SWEEP_MAX_DEFAULT = 4096;
constexpr int PGRAD_MAXD = 32;                 // a row's 2 d sums live in registers

enum class PgradRoute { None = 0, Sweep = 1, Inverse = 2 };

struct PgradPlan {
    PgradRoute route = PgradRoute::None;
    int64_t np = 0;            // n rounded up to 128: rows of W
    int64_t ldw = 0;           // leading dimension of W: Np + ld_pad
    int64_t w_bytes = 0;       // np * ldw * 8 (0: no W)
    int64_t groups = 0;        // sweep: 16-row groups
    int64_t launches = 0;      // sweep: Np / 128
    int64_t stream_bytes = 0;  // sweep: L's lower triangle in whole 128 x 128 blocks, once per group
    int64_t u_bytes = 0;       // inverse: Np * ldA * 8 for U
};

// n, Np: test points and padded training columns.  ldA, ld_pad: the factor's leading dimension and the context's padding.
// fused: the resident factor carries the 16 x 16 inverses.  want_dvar: dvar was asked for.  sweep_opt: option
// "pgrad_sweep", -1 by size, 0 the inverse route always, 1 the sweep route whenever allowed.  sweep_max: option
// "pgrad_sweep_max".
inline PgradPlan pgrad_plan(int64_t n, int64_t Np, int64_t ldA, int64_t ld_pad, int fused, bool want_dvar, int sweep_opt,
                            int64_t sweep_max) {
    PgradPlan p;
    p.np = (n + PGRAD_TILE - 1) / PGRAD_TILE * PGRAD_TILE;
    if (!want_dvar) return p;
    const bool allowed = fused != 0;
    const bool sweep = allowed && (sweep_opt == 1 || (sweep_opt < 0 && n <= sweep_max));
    p.route = sweep ? PgradRoute::Sweep : PgradRoute::Inverse;
    p.ldw = Np + ld_pad;
    p.w_bytes = p.np * p.ldw * 8;
    if (sweep) {
        const int64_t nblk = Np / PGRAD_TILE;
        p.groups = (n + PGRAD_GROUP - 1) / PGRAD_GROUP;
        p.launches = nblk;
        p.stream_bytes = p.groups * (nblk * (nblk + 1) / 2) * PGRAD_TILE * PGRAD_TILE * 8;
    } else {
        p.u_bytes = Np * ldA * 8;
    }
    return p;
}

}  // namespace gpmi
