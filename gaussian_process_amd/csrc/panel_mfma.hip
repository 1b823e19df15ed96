// Second-generation panel kernels: the latency chain of a block step on the matrix pipe.
//
//   potrf128_kernel   Cholesky of a 128 x 128 diagonal block by ONE workgroup (8 waves).
//   trsm128_kernel    X (m x 128) <- X * L^-T for the rows below it, 16 rows per wave, chip-wide.
//
// They replace the chains potf2_64 -> trsm_rlt64 -> rank-64 GEMM (two of each per 128 columns, all
// latency-bound launches; the substitution kernels were fp64 VALU) behind np.linalg.cholesky and the
// LU-based np.linalg.solve of the reference (GP_regression.py:138-139, 144).
//
// Everything except the 16 x 16 diagonal blocks runs on v_mfma_f64_16x16x4_f64.  The 16 x 16 blocks are
// factored AND inverted by one wave with the rows in registers (v_readlane broadcasts, no LDS, no barrier);
// with W_jj = L_jj^-1 at hand, "rows below" is a matrix product  L_ij = S_ij * W_jj^T  and so is every update.
// Only 16 x 16 inverses are ever formed (cond(L_jj) of a 16 x 16 diagonal block, never of the panel).
//
// Register layout of a 16 x 16 tile X (rows n, columns c) -- "X layout": lane (fr = lane & 15, fg = lane >> 4)
// holds x[v] = X[fr][kap(fg, v)],  kap(g, v) = 2g + (v & 1) + 8 (v >> 1): two 16-byte pieces of row fr.
// This IS the B-operand layout of the MFMA up to a permutation of the summation index (which both
// operands share), and -- with the rows of the A operand permuted by rho(g + 4v) = kap(g, v) -- also the
// layout the MFMA writes its result in.  So a tile that has just been produced feeds the next products
// straight from its accumulator registers: no shuffles, no LDS round trip for X.
//   Y[c][n] = sum_k M[c][k] X[n][k]:   acc = mfma(a_v, x[v], acc), v = 0..3,
//   a_v(lane) = M[rho(lane & 15)][kap(lane >> 4, v)],   new x[v] = acc[v].
// The A operands (W_jj, -L_kj) live in LDS as 16 rows x 128 bytes, row i' = M[rho(i')][:], 16-byte slots
// XOR-swizzled by (i' >> 1) & 7: both ds_read_b128 of a fragment are conflict-free (brute-force checked).
#include "gpmi_internal.h"
#include <utility>

namespace gpmi {

typedef double d4 __attribute__((ext_vector_type(4)));
typedef double d2 __attribute__((ext_vector_type(2)));

namespace {

constexpr int PB = 128;                 // panel block width
constexpr int NT = PB / 16;             // 16 x 16 tiles per side
constexpr int TILE_BYTES = 16 * 128;
constexpr int NTILES = NT * (NT + 1) / 2;
constexpr int POTRF_TILES = NT + 1;     // potrf128 keeps only the current step's operand tiles in LDS (18 KiB)
constexpr int TRSM_ROWS = 64;            // rows per trsm128 workgroup pass (4 waves x 16)
constexpr int SCR_LD = 18;              // doubles per scratch row (16-byte aligned rows, conflict-free row reads)

__device__ __forceinline__ int kap(int g, int v) { return 2 * g + (v & 1) + 8 * (v >> 1); }
// LDS row that holds matrix row n: rho^-1(n)
__device__ __forceinline__ int rho_inv(int n) { return ((n >> 1) & 3) + 4 * (n & 1) + 8 * (n >> 3); }

__device__ __forceinline__ double readlane_d(double v, int lane) {
    int lo = __double2loint(v), hi = __double2hiint(v);
    lo = __builtin_amdgcn_readlane(lo, lane);
    hi = __builtin_amdgcn_readlane(hi, lane);
    return __hiloint2double(hi, lo);
}

__device__ __forceinline__ double rcp_newton(double p) {
    double y = __builtin_amdgcn_rcp(p);
    double e = fma(-p, y, 1.0);
    y = fma(y, e, y);
    e = fma(-p, y, 1.0);
    return fma(y, e, y);
}

// address (in d2 units) of slot s of row i' inside a tile
__device__ __forceinline__ int tslot(int row, int s) { return row * 8 + (s ^ ((row >> 1) & 7)); }

// A-operand fragments of a tile for this lane: a[v] = M[rho(lane & 15)][kap(lane >> 4, v)]
__device__ __forceinline__ void load_afrag(const d2* tile, int lane, double (&a)[4]) {
    const int i = lane & 15, kk = lane >> 4;
    const d2 lo = tile[tslot(i, kk)], hi = tile[tslot(i, 4 + kk)];
    a[0] = lo.x; a[1] = lo.y; a[2] = hi.x; a[3] = hi.y;
}

// publish a tile held in X layout (element (fr, kap(fg, v))) as an A operand, scaled by sgn
__device__ __forceinline__ void publish_tile(d2* tile, int lane, const double (&x)[4], double sgn) {
    const int row = rho_inv(lane & 15), fg = lane >> 4;
    tile[tslot(row, fg)] = d2{sgn * x[0], sgn * x[1]};
    tile[tslot(row, 4 + fg)] = d2{sgn * x[2], sgn * x[3]};
}

// y = M * X^T in X layout (see the file header); acc_in is the C operand
__device__ __forceinline__ void tile_mma(const double (&a)[4], const double (&b)[4], double (&c)[4]) {
    d4 acc = d4{c[0], c[1], c[2], c[3]};
#pragma unroll
    for (int v = 0; v < 4; ++v) acc = __builtin_amdgcn_mfma_f64_16x16x4f64(a[v], b[v], acc, 0, 0, 0);
    c[0] = acc[0]; c[1] = acc[1]; c[2] = acc[2]; c[3] = acc[3];
}

__device__ __forceinline__ void load_xtile(const double* p, int64_t ld, int lane, double (&x)[4]) {
    const double* r = p + (int64_t)(lane & 15) * ld + 2 * (lane >> 4);
    const d2 lo = *reinterpret_cast<const d2*>(r), hi = *reinterpret_cast<const d2*>(r + 8);
    x[0] = lo.x; x[1] = lo.y; x[2] = hi.x; x[3] = hi.y;
}
__device__ __forceinline__ void store_xtile(double* p, int64_t ld, int lane, const double (&x)[4]) {
    double* r = p + (int64_t)(lane & 15) * ld + 2 * (lane >> 4);
    *reinterpret_cast<d2*>(r) = d2{x[0], x[1]};
    *reinterpret_cast<d2*>(r + 8) = d2{x[2], x[3]};
}

// ---------------------------------------------------------------------------
// Cholesky AND inverse of a 16 x 16 block by one wave, rows in registers, no LDS, no barrier.
// Lanes 0..15: lane r holds row r of the symmetric positive definite block in v[0..15] (entries k <= r are
// read).  Lanes 16..31: lane 16 + c holds column c of the identity.  Right-looking sweep, column c:
//     p = v[c] of lane c;  v[c] *= 1/sqrt(p);  v[k] -= L[k][c] * v[c]  for k > c,  L[k][c] = v[c] of lane k.
// The same instructions run the forward substitution W = L^-1 on lanes 16..31 (both need the scalar L[k][c],
// one v_readlane pair per (c, k)), so the inverse costs no instruction of its own.  The chain pivot ->
// 1/sqrt -> scale -> next pivot is software-pipelined by hand: column c + 1's reciprocal square root runs
// stage by stage between the updates of column c (the order below is pinned with scheduling barriers; left to
// itself the compiler splits the loop in two and spills the scalars).
// Afterwards: lane r holds L[r][k] in v[k] (k <= r); lane 16 + c holds W[r][c] in v[r] (zero for r < c).
// Returns the first non-positive pivot (16 if none).
// ---------------------------------------------------------------------------
struct RsqChain {      // 1/sqrt(p) and sqrt(p) in stages (v_rsq_f64 + two coupled Newton steps + residual fix)
    double p, y, g, h, r;
    __device__ __forceinline__ void stage(int i) {
        switch (i) {
            case 0: y = __builtin_amdgcn_rsq(p); break;
            case 1: g = p * y; h = 0.5 * y; break;
            case 2: r = fma(-h, g, 0.5); break;
            case 3: g = fma(g, r, g); h = fma(h, r, h); break;
            case 4: r = fma(-h, g, 0.5); break;
            case 5: g = fma(g, r, g); h = fma(h, r, h); break;
            case 6: r = fma(-g, g, p); break;
            case 7: g = fma(r, h, g); h = h + h; break;        // g = sqrt(p), h = 1/sqrt(p)
            default: break;
        }
    }
};
constexpr int RSQ_STAGES = 8;
#define PANEL_FENCE() __builtin_amdgcn_sched_barrier(0)

__device__ __forceinline__ int factor16_packed(double (&v)[16], int lane) {
    int bad = 16;
    RsqChain ch;
    ch.p = readlane_d(v[0], 0);
#pragma unroll
    for (int i = 0; i < RSQ_STAGES; ++i) ch.stage(i);
#pragma unroll
    for (int c = 0; c < 16; ++c) {
        // a pivot that is not positive needs no special case beyond its index: 1/sqrt of a negative number is NaN, of a
        // zero +-inf and p * inf = NaN, so g and h are NaN and everything after this column is
        if (!(ch.p > 0.0) && bad == 16) bad = c;
        v[c] = (lane == c) ? ch.g : v[c] * ch.h;
        PANEL_FENCE();
        int st = 0;
        if (c < 15) {
            const double l1 = readlane_d(v[c], c + 1);
            v[c + 1] = fma(-l1, v[c], v[c + 1]);
            PANEL_FENCE();
            ch.p = readlane_d(v[c + 1], c + 1);          // next pivot: its chain overlaps the updates below
            ch.stage(st++);
            PANEL_FENCE();
        }
        // the scalars of the whole column first (a v_readlane result is not usable for ~10 cycles), then the
        // updates, one chain stage of the next pivot between every two of them
        double lk[16];
#pragma unroll
        for (int k = c + 2; k < 16; ++k) lk[k] = readlane_d(v[c], k);
        PANEL_FENCE();
#pragma unroll
        for (int k = c + 2; k < 16; ++k) {
            v[k] = fma(-lk[k], v[c], v[k]);
            if (st < RSQ_STAGES && ((k - c) & 1)) { PANEL_FENCE(); ch.stage(st++); PANEL_FENCE(); }
        }
        PANEL_FENCE();
        if (c < 15) {
#pragma unroll
            for (int i = 0; i < RSQ_STAGES; ++i)
                if (i >= st) ch.stage(i);
            PANEL_FENCE();
        }
    }
    return bad;
}

// lane 16 + c holds column c of W (v[r] = W[r][c]): write it as an A-operand tile
__device__ __forceinline__ void publish_w(double* tile, int lane, const double (&v)[16]) {
    if (lane >= 16 && lane < 32) {
        const int c = lane - 16;
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const int row = rho_inv(r);
            tile[2 * tslot(row, c >> 1) + (c & 1)] = v[r];
        }
    }
}

// Phase 1 of a potrf128 step, one copy of the code for all eight steps (everything it touches is behind
// pointers): the diagonal tile sits row-major in `scratch`; factor + invert; to memory: L_jj on and below the
// diagonal of the tile and W_jj TRANSPOSED strictly above it (tile[c][r] = W[r][c], r > c; the diagonal of W is
// 1 / diag(L)) -- the strict upper triangles of the diagonal 16 x 16 tiles are storage nothing else reads, and
// every later triangular solve with this block (trsm128, the backward solve) finds its inverse there instead
// of recomputing it; W_jj as an A operand to its LDS tile; a non-positive pivot to *info.
__device__ __noinline__ void factor_diag_tile(const double* scratch, double* Ajj, int64_t ld, double* wtile,
                                              int64_t col0, int64_t* info) {
    const int lane = threadIdx.x & 63;
    double v[16];
#pragma unroll
    for (int k = 0; k < 16; k += 2) {
        const d2 t = *reinterpret_cast<const d2*>(scratch + (lane & 15) * SCR_LD + k);
        v[k] = (lane < 16) ? t.x : ((lane - 16 == k) ? 1.0 : 0.0);
        v[k + 1] = (lane < 16) ? t.y : ((lane - 16 == k + 1) ? 1.0 : 0.0);
    }
    const int bad = factor16_packed(v, lane);
    if (bad < 16 && lane == 0) atomicMin((unsigned long long*)info, (unsigned long long)(col0 + bad));
    if (lane < 32) {
        double* row = Ajj + (int64_t)(lane & 15) * ld;
#pragma unroll
        for (int k = 0; k < 16; ++k) {
            const bool mine = (lane < 16) ? (k <= lane) : (k > lane - 16);
            if (mine) row[k] = v[k];
        }
    }
    publish_w(wtile, lane, v);
}

// Staging of a diagonal tile in trsm128: W_jj as an A operand from the factored tile G at Ljj -- W[n][k] =
// G[k][n] for k < n (stored transposed above the diagonal by factor_diag_tile), 1 / G[n][n] on the diagonal.
__device__ __forceinline__ void stage_w_tile(const double* Ljj, int64_t ldl, d2* wtile, int lane) {
    const int n = lane & 15, fg = lane >> 4;
    double x[4];
#pragma unroll
    for (int q = 0; q < 4; ++q) {
        const int k = kap(fg, q);
        double val = 0.0;
        if (k < n) val = Ljj[(int64_t)k * ldl + n];
        else if (k == n) val = rcp_newton(Ljj[(int64_t)n * ldl + n]);
        x[q] = val;
    }
    publish_tile(wtile, lane, x, 1.0);
}

}  // namespace

// ---------------------------------------------------------------------------
// potrf128: A (128 x 128, lower, leading dimension ld) <- its Cholesky factor, one workgroup of 8 waves.
// Wave i owns block row i (tiles (i, 0..i)) in registers for the whole kernel.  Step j:
//   1  wave j       factors + inverts its diagonal tile, writes L_jj to memory and W_jj to LDS
//   2  waves i > j  L_ij = S_ij W_jj^T (4 MFMAs), to memory and, negated, to LDS
//   3  waves i > j  S_ik -= L_ij L_kj^T for k = j+1..i (4 MFMAs per tile), the diagonal chain first
// Two barriers per step; a wave's tiles never leave its registers.  LDS holds only the operands of the current
// step (8 tile slots + W_jj + the scratch tile, 20 KiB).  Beside a trailing update (lookahead) the workgroup still waits
// for an empty CU -- 123 registers at two waves per SIMD do not fit next to an update workgroup's 2 x 144 -- which was
// measured to be the better deal: a 94-register variant that does fit and starts at once runs its serial 16 x 16
// factors so much slower on SIMDs shared with the update's MFMA stream that the panel stream gets longer (DESIGN.md
// section 7 item 2).
// ---------------------------------------------------------------------------
__device__ __forceinline__ void potrf128_body(double* A, int64_t ld, int64_t col_offset, int64_t* info,
                                              unsigned long long* stamps, char* smem) {
    d2* tiles = reinterpret_cast<d2*>(smem);          // slot i: -L_ij of the current step j (block row i), slot 8: W_jj
    double* scratch = reinterpret_cast<double*>(smem + POTRF_TILES * TILE_BYTES);    // 16 x SCR_LD doubles
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int fr = lane & 15, fg = lane >> 4;

    double xt[NT][4];
#pragma unroll
    for (int k = 0; k < NT; ++k) {
        if (k <= wave) load_xtile(A + (int64_t)(16 * wave) * ld + 16 * k, ld, lane, xt[k]);
        else { xt[k][0] = xt[k][1] = xt[k][2] = xt[k][3] = 0.0; }
    }

    // diagnostic (gpmi_probe_panel): stamps[6 j + q] = clock at the q-th boundary of step j, as seen by wave j
    // (phase 1 begin / end) and wave min(j + 1, 7) (after barrier, after phase 2, after barrier, after phase 3)
#define PANEL_STAMP(cond, idx) if (stamps && (cond) && lane == 0) stamps[idx] = __builtin_amdgcn_s_memtime()
    PANEL_STAMP(wave == 0, 48);
#pragma unroll
    for (int j = 0; j < NT; ++j) {
        PANEL_STAMP(wave == j, 6 * j);
        if (wave == j) {
            // X layout -> one row per lane through the scratch tile
#pragma unroll
            for (int v = 0; v < 4; ++v) scratch[fr * SCR_LD + kap(fg, v)] = xt[j][v];
            __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
            __builtin_amdgcn_wave_barrier();
            factor_diag_tile(scratch, A + (int64_t)(16 * j) * ld + 16 * j, ld,
                             reinterpret_cast<double*>(tiles + NT * 128), col_offset + 16 * j, info);
        }
        PANEL_STAMP(wave == j, 6 * j + 1);
        __syncthreads();
        PANEL_STAMP(wave == (j < 7 ? j + 1 : 7), 6 * j + 2);
        if (wave > j) {
            double a[4], z[4] = {0., 0., 0., 0.};
            load_afrag(tiles + NT * 128, lane, a);
            tile_mma(a, xt[j], z);
#pragma unroll
            for (int v = 0; v < 4; ++v) xt[j][v] = z[v];
            publish_tile(tiles + wave * 128, lane, xt[j], -1.0);
            store_xtile(A + (int64_t)(16 * wave) * ld + 16 * j, ld, lane, xt[j]);
        }
        PANEL_STAMP(wave == (j < 7 ? j + 1 : 7), 6 * j + 3);
        __syncthreads();
        PANEL_STAMP(wave == (j < 7 ? j + 1 : 7), 6 * j + 4);
        if (wave > j) {
#pragma unroll
            for (int k = j + 1; k < NT; ++k) {
                if (k <= wave) {
                    double a[4];
                    load_afrag(tiles + k * 128, lane, a);
                    tile_mma(a, xt[j], xt[k]);
                }
            }
        }
        PANEL_STAMP(wave == (j < 7 ? j + 1 : 7), 6 * j + 5);
    }
    PANEL_STAMP(wave == 7, 49);
#undef PANEL_STAMP
}

__global__ __launch_bounds__(512) void potrf128_kernel(double* A, int64_t ld, int64_t col_offset, int64_t* info,
                                                        unsigned long long* stamps) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    potrf128_body(A, ld, col_offset, info, stamps, smem);
}

// ---------------------------------------------------------------------------
// trsm128: X (m x 128) <- X * L^-T, L 128 x 128 lower (its upper triangle is not read).
// Workgroup = 4 waves, two workgroups per CU; staging: the 28 off-diagonal tiles of L go to LDS negated, the 8
// diagonal tiles contribute their stored inverses -- every workgroup does this for itself (72 KiB out of L2,
// behind the load of its first rows), then walks slabs of 64 rows, 16 rows per wave, all 128 columns of a row
// in 64 registers:
//   for j = 0..7:  X_j <- X_j W_jj^T;   X_k -= X_j L_kj^T  for k > j         (144 MFMAs per 16 rows)
// ---------------------------------------------------------------------------
// PHASE -1: the whole solve in one launch (36 operand tiles, 72 KiB of LDS).
// PHASE 0 / 1: the same solve as two launches -- columns 0..63 plus their updates of columns 64..127 (26 tiles,
// 52 KiB), then columns 64..127 (10 tiles, 20 KiB) -- for launches that run beside a trailing update
// (lookahead): its workgroups hold 96 KiB of every CU's 160 KiB, so only kernels with <= 64 KiB start at once.
template <int PHASE>
__device__ __forceinline__ constexpr int trsm_slot(int j, int k) {      // k <= j
    if (PHASE == 0) return j < 4 ? j * (j + 1) / 2 + k : 10 + (j - 4) * 4 + k;
    if (PHASE == 1) return (j - 4) * (j - 3) / 2 + (k - 4);
    return j * (j + 1) / 2 + k;
}
template <int PHASE> constexpr int trsm_tiles() { return PHASE == 0 ? 26 : PHASE == 1 ? 10 : NTILES; }

// Staging of a 128 x 128 factored diagonal block as A operands (4 waves): the off-diagonal tiles of this phase,
// negated, round-robin over the waves, and the stored inverses of the diagonal tiles.  A wave first REQUESTS all of its
// tiles (up to seven off-diagonal ones and two diagonal ones, 36 registers) and only then publishes them: one memory
// round trip instead of one per tile (the first form, a load-and-publish per tile under a per-wave test, took 12.4k
// cycles of a 12 us launch).  The tile list of a phase is a compile-time table, (j << 4) | k in launch order.
template <int PHASE> struct StageList {
    static constexpr int J0 = PHASE == 1 ? 4 : 0, J1 = PHASE == 0 ? 4 : NT;
    static constexpr int count() {
        int n = 0;
        for (int j = 1; j < NT; ++j)
            for (int k = 0; k < j; ++k)
                if (k >= J0 && k < J1) ++n;
        return n;
    }
    static constexpr int entry(int t) {
        int n = 0;
        for (int j = 1; j < NT; ++j)
            for (int k = 0; k < j; ++k)
                if (k >= J0 && k < J1) {
                    if (n == t) return (j << 4) | k;
                    ++n;
                }
        return 0;
    }
};
template <int PHASE, int... T>
__device__ __forceinline__ int stage_entry(int t, std::integer_sequence<int, T...>) {
    // a switch the compiler turns into a scalar table lookup: t is wave-uniform
    constexpr int tab[] = {StageList<PHASE>::entry(T)...};
    return tab[t];
}

template <int PHASE>
__device__ __forceinline__ void stage_l_tiles_batched(const double* L, int64_t ldl, d2* tiles, int lane, int wave,
                                                      unsigned long long* stamps) {
    constexpr int J0 = StageList<PHASE>::J0, J1 = StageList<PHASE>::J1;
    constexpr int NOFF = StageList<PHASE>::count();
    constexpr int PER = (NOFF + 3) / 4;                 // off-diagonal tiles per wave
    constexpr int NW = (J1 - J0 + 3) / 4;               // diagonal tiles per wave
    const int n = lane & 15, fg = lane >> 4;
    double x[PER][4], w[NW][4];
    int slot[PER];
    // ---- requests
#pragma unroll
    for (int i = 0; i < PER; ++i) {
        const int t = 4 * i + wave;
        const int e = stage_entry<PHASE>(t < NOFF ? t : NOFF - 1, std::make_integer_sequence<int, NOFF>{});
        const int jj = e >> 4, kk = e & 15;
        slot[i] = t < NOFF ? (PHASE == 0 ? (jj < 4 ? jj * (jj + 1) / 2 + kk : 10 + (jj - 4) * 4 + kk)
                                         : PHASE == 1 ? (jj - 4) * (jj - 3) / 2 + (kk - 4) : jj * (jj + 1) / 2 + kk)
                           : -1;
        load_xtile(L + (int64_t)(16 * jj) * ldl + 16 * kk, ldl, lane, x[i]);
    }
#pragma unroll
    for (int r = 0; r < NW; ++r) {
        const int j = J0 + wave + 4 * r;
        const double* Ljj = L + (int64_t)(16 * (j < J1 ? j : J0)) * (ldl + 1);
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            const int k = kap(fg, q);
            w[r][q] = (k <= n) ? Ljj[(int64_t)k * ldl + n] : 0.0;     // W^T above the diagonal, L's diagonal on it
        }
    }
    // ---- publication
#pragma unroll
    for (int i = 0; i < PER; ++i)
        if (slot[i] >= 0) publish_tile(tiles + slot[i] * 128, lane, x[i], -1.0);
    if (stamps && wave == 0 && lane == 0) stamps[57] = __builtin_amdgcn_s_memtime();
#pragma unroll
    for (int r = 0; r < NW; ++r) {
        const int j = J0 + wave + 4 * r;
        if (j < J1) {
#pragma unroll
            for (int q = 0; q < 4; ++q)
                if (kap(fg, q) == n) w[r][q] = rcp_newton(w[r][q]);        // diag(W) = 1 / diag(L)
            publish_tile(tiles + trsm_slot<PHASE>(j, j) * 128, lane, w[r], 1.0);
        }
    }
}

// The two-launch forms (PHASE 0 / 1) run beside a trailing update, where what counts is that two workgroups fit on a CU
// next to an update workgroup (<= 112 registers): they keep the one-tile-at-a-time staging (108 / 68 registers against
// 138 / 74 batched); the one-launch form, which has the CU to itself, stages batched (154 registers).
template <int PHASE>
__device__ __forceinline__ void stage_l_tiles(const double* L, int64_t ldl, d2* tiles, int lane, int wave,
                                              unsigned long long* stamps) {
    if constexpr (PHASE == -1) {
        stage_l_tiles_batched<PHASE>(L, ldl, tiles, lane, wave, stamps);
    } else {
        constexpr int J0 = PHASE == 1 ? 4 : 0, J1 = PHASE == 0 ? 4 : NT;
        int t = 0;
#pragma unroll
        for (int j = 1; j < NT; ++j)
#pragma unroll
            for (int k = 0; k < j; ++k) {
                if (k >= J0 && k < J1) {
                    if ((t & 3) == wave) {
                        double x[4];
                        load_xtile(L + (int64_t)(16 * j) * ldl + 16 * k, ldl, lane, x);
                        publish_tile(tiles + trsm_slot<PHASE>(j, k) * 128, lane, x, -1.0);
                    }
                    ++t;
                }
            }
        if (stamps && wave == 0 && lane == 0) stamps[57] = __builtin_amdgcn_s_memtime();
#pragma unroll
        for (int j = J0; j < J1; ++j)
            if (((j - J0) & 3) == wave)
                stage_w_tile(L + (int64_t)(16 * j) * ldl + 16 * j, ldl, tiles + trsm_slot<PHASE>(j, j) * 128, lane);
    }
}

template <int PHASE>
__global__ __launch_bounds__(256, 2) void trsm128_kernel(const double* L, int64_t ldl, double* X, int64_t ldx,
                                                          int64_t nslabs, unsigned long long* stamps) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    d2* tiles = reinterpret_cast<d2*>(smem);
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    constexpr int J0 = PHASE == 1 ? 4 : 0;             // first / one past last column tile this launch solves
    constexpr int J1 = PHASE == 0 ? 4 : NT;
    constexpr int T0 = PHASE == 1 ? 4 : 0;             // first column tile this launch touches
#define PANEL_STAMP(cond, idx) if (stamps && (cond) && lane == 0) stamps[idx] = __builtin_amdgcn_s_memtime()
    PANEL_STAMP(blockIdx.x == 0 && wave == 0, 56);

    // the first slab's rows are requested before L is staged: their latency hides behind the staging
    double xt[NT][4];
    int64_t slab = blockIdx.x;
    if (slab < nslabs) {
        const double* Xr = X + (slab * TRSM_ROWS + 16 * wave) * ldx;
#pragma unroll
        for (int k = T0; k < NT; ++k) load_xtile(Xr + 16 * k, ldx, lane, xt[k]);
    }
    stage_l_tiles<PHASE>(L, ldl, tiles, lane, wave, blockIdx.x == 0 ? stamps : nullptr);
    PANEL_STAMP(blockIdx.x == 0 && wave == 0, 58);
    __syncthreads();
    PANEL_STAMP(blockIdx.x == 0 && wave == 0, 59);

    for (; slab < nslabs; slab += gridDim.x) {
        double* Xr = X + (slab * TRSM_ROWS + 16 * wave) * ldx;
        if (slab != (int64_t)blockIdx.x) {
#pragma unroll
            for (int k = T0; k < NT; ++k) load_xtile(Xr + 16 * k, ldx, lane, xt[k]);
        }
        if (stamps) asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        PANEL_STAMP(blockIdx.x == 0 && wave == 0 && slab == blockIdx.x, 60);
#pragma unroll
        for (int j = J0; j < J1; ++j) {
            double a[4], z[4] = {0., 0., 0., 0.};
            load_afrag(tiles + trsm_slot<PHASE>(j, j) * 128, lane, a);
            tile_mma(a, xt[j], z);
#pragma unroll
            for (int v = 0; v < 4; ++v) xt[j][v] = z[v];
#pragma unroll
            for (int k = j + 1; k < NT; ++k) {
                double b[4];
                load_afrag(tiles + trsm_slot<PHASE>(k, j) * 128, lane, b);
                tile_mma(b, xt[j], xt[k]);
            }
            __builtin_amdgcn_sched_barrier(0);      // one step's operand fragments at a time (register pressure)
        }
        PANEL_STAMP(blockIdx.x == 0 && wave == 0 && slab == blockIdx.x, 61);
#pragma unroll
        for (int k = T0; k < NT; ++k) store_xtile(Xr + 16 * k, ldx, lane, xt[k]);
    }
    PANEL_STAMP(blockIdx.x == 0 && wave == 0, 62);
#undef PANEL_STAMP
}

// ---------------------------------------------------------------------------
// vinv128: for every 128 x 128 diagonal block of a fused factor, V = L_kk^-1, stored TRANSPOSED in the block's
// upper triangle (G[c][r] = V[r][c], r > c) -- the convention of the 16 x 16 diagonal tiles (W_jj^T strictly above
// the diagonal, diag(V) = 1 / diag(L) implied) carried to the whole block: the strict block-upper tiles are storage
// nothing else reads.  One workgroup per block; wave w takes tile rows w and 4 + w of the identity through the
// trsm128 recurrence (I L^-T = V^T), skipping the column tiles left of its own (they stay zero).
// The backward solve (solve.hip) then gets x_k = V^T r_k as a matrix-vector product instead of 8 dependent
// 16 x 16 solve-and-update rounds.  Only ever used for vectors (alpha); the factorisation itself and the
// predictive solves keep to 16 x 16 inverses.
// ---------------------------------------------------------------------------
// vside (may be null): additionally V itself, row-major 128 x 128 per block with zeros above the diagonal and
// diag(V) = 1 / diag(L) in place, block b at vside + b * 128 * 128 -- the single-launch backward solve (solve.hip)
// streams it like one more block of L.  The caller zero-fills vside first (column tiles left of a wave's own are
// never written).
__global__ __launch_bounds__(256, 2) void vinv128_kernel(double* A, int64_t ld, double* vside) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    d2* tiles = reinterpret_cast<d2*>(smem);
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    double* Lb = A + (int64_t)blockIdx.x * PB * (ld + 1);
    stage_l_tiles<-1>(Lb, ld, tiles, lane, wave, nullptr);
    __syncthreads();
    for (int p = 0; p < 2; ++p) {
        const int i = 4 * p + wave;
        double xt[NT][4];
#pragma unroll
        for (int k = 0; k < NT; ++k)
#pragma unroll
            for (int v = 0; v < 4; ++v) xt[k][v] = (k == i && (lane & 15) == kap(lane >> 4, v)) ? 1.0 : 0.0;
#pragma unroll
        for (int j = 0; j < NT; ++j) {
            if (j >= i) {
                double a[4], z[4] = {0., 0., 0., 0.};
                load_afrag(tiles + trsm_slot<-1>(j, j) * 128, lane, a);
                tile_mma(a, xt[j], z);
#pragma unroll
                for (int v = 0; v < 4; ++v) xt[j][v] = z[v];
#pragma unroll
                for (int k = j + 1; k < NT; ++k) {
                    double b[4];
                    load_afrag(tiles + trsm_slot<-1>(k, j) * 128, lane, b);
                    tile_mma(b, xt[j], xt[k]);
                }
            }
            __builtin_amdgcn_sched_barrier(0);
        }
#pragma unroll
        for (int k = 1; k < NT; ++k)
            if (k > i) store_xtile(Lb + (int64_t)(16 * i) * ld + 16 * k, ld, lane, xt[k]);
        if (vside) {
            // xt[k][v] = V^T[16 i + fr][16 k + kap(fg, v)] = V[16 k + kap(fg, v)][16 i + fr]: 16 lanes (fr) write 128 contiguous bytes
            double* Vb = vside + (int64_t)blockIdx.x * PB * PB + 16 * i + (lane & 15);
#pragma unroll
            for (int k = 0; k < NT; ++k)
                if (k >= i) {
#pragma unroll
                    for (int v = 0; v < 4; ++v) Vb[(16 * k + kap(lane >> 4, v)) * PB] = xt[k][v];
                }
        }
    }
}

// ---------------------------------------------------------------------------
// border_sweep: X (rows <= 16, ncols) <- X * L^-T for a fused factor L (ncols x ncols), the forward sweep of gpmi_append
// for a few new points.  trsm128's recurrence, but the work is reading L (streamed once; the flops are nothing), so
// the grid follows the rows of L: the <= 16 rows of X are the B operand of every MFMA (dead rows fed as zeros, never
// stored), 16 rows of L the A operand, read straight from memory in fragment layout (two 16-byte pieces of a row per
// lane; the four lane groups take a row's 128 bytes between them), and one wave turns a 16 x 128 strip of L into the
// update of a 16 x 16 piece of X.
// One launch per 128-column block t, nblk - t workgroups: workgroup b updates column block t + b of X with the block
// solved by the launch before, X_c -= X_(t-1) L_(c, t-1)^T, wave w its tiles w and 4 + w; workgroup 0 then solves its
// block against L_tt (staged as in trsm128; one wave, 36 tile products), so launch t + 1 finds X_t final.  The order is
// the launch order; no workgroup waits for another, nothing is added atomically: the same bits every run.
// Measured (profiles/r14_append_rate.txt) the chain of launches bounds it, not memory: 12.8 us per launch at 4096
// columns, where there is next to nothing to stream, 15.5 us and 0.35 of the streaming-read rate at 65536.  Not measured:
// how the 12.8 us split between the launch gap and workgroup 0's update and one-wave solve, and what the LDS request adds
// to the rest -- every workgroup asks for SWEEP_LDS though only workgroup 0 uses it, which holds the streaming
// workgroups to one per CU.
// Reads of L: the tiles below the block diagonal, and of the diagonal 128 x 128 blocks the lower 16 x 16 tiles and the
// diagonal tiles whole (their stored inverses) -- never the block-upper tiles, which hold L_kk^-T after a backward solve.
// ---------------------------------------------------------------------------
constexpr int SWEEP_LDS = NTILES * TILE_BYTES + NT * 64 * 4 * 8;     // the staged block and the eight tiles of X_t

__device__ __forceinline__ void load_xtile_rows(const double* p, int64_t ld, int lane, int rows, double (&x)[4]) {
    x[0] = x[1] = x[2] = x[3] = 0.0;
    if ((lane & 15) < rows) load_xtile(p, ld, lane, x);
}
__device__ __forceinline__ void store_xtile_rows(double* p, int64_t ld, int lane, int rows, const double (&x)[4]) {
    if ((lane & 15) < rows) store_xtile(p, ld, lane, x);
}
// A-operand fragments of -M for the 16 x 16 tile M at `tile` in memory: what load_afrag reads from a published tile
__device__ __forceinline__ void load_afrag_neg(const double* tile, int64_t ld, int lane, double (&a)[4]) {
    const int i = lane & 15, kk = lane >> 4;
    const int row = kap(i & 3, i >> 2);                     // rho(i)
    const double* r = tile + (int64_t)row * ld + 2 * kk;
    const d2 lo = *reinterpret_cast<const d2*>(r), hi = *reinterpret_cast<const d2*>(r + 8);
    a[0] = -lo.x; a[1] = -lo.y; a[2] = -hi.x; a[3] = -hi.y;
}

__global__ __launch_bounds__(256) void border_sweep_kernel(const double* __restrict__ L, int64_t ldl, double* X, int64_t ldx,
                                                           int rows, int64_t t) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    d2* tiles = reinterpret_cast<d2*>(smem);
    double* xs = reinterpret_cast<double*>(smem + NTILES * TILE_BYTES);
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int64_t cb = t + blockIdx.x;                      // the column block of X (row block of L) of this workgroup
    const bool solver = blockIdx.x == 0;
    if (solver) stage_l_tiles<-1>(L + (int64_t)PB * t * (ldl + 1), ldl, tiles, lane, wave, nullptr);

    double* Xc = X + (int64_t)PB * cb;
    double acc[2][4];
#pragma unroll
    for (int p = 0; p < 2; ++p) load_xtile_rows(Xc + 16 * (wave + 4 * p), ldx, lane, rows, acc[p]);
    if (t > 0) {
        const double* Xk = X + (int64_t)PB * (t - 1);
        double xk[NT][4];
#pragma unroll
        for (int j = 0; j < NT; ++j) load_xtile_rows(Xk + 16 * j, ldx, lane, rows, xk[j]);
#pragma unroll
        for (int p = 0; p < 2; ++p) {
            const double* Lr = L + ((int64_t)PB * cb + 16 * (wave + 4 * p)) * ldl + (int64_t)PB * (t - 1);
            double a[NT][4];
#pragma unroll
            for (int j = 0; j < NT; ++j) load_afrag_neg(Lr + 16 * j, ldl, lane, a[j]);
#pragma unroll
            for (int j = 0; j < NT; ++j) tile_mma(a[j], xk[j], acc[p]);
        }
    }
    if (!solver) {
#pragma unroll
        for (int p = 0; p < 2; ++p) store_xtile_rows(Xc + 16 * (wave + 4 * p), ldx, lane, rows, acc[p]);
        return;
    }
    // workgroup 0: the updated block to wave 0 through LDS (lane-private slots), then trsm128's steps on it
#pragma unroll
    for (int p = 0; p < 2; ++p)
#pragma unroll
        for (int v = 0; v < 4; ++v) xs[((wave + 4 * p) * 64 + lane) * 4 + v] = acc[p][v];
    __syncthreads();
    if (wave != 0) return;
    double xt[NT][4];
#pragma unroll
    for (int k = 0; k < NT; ++k)
#pragma unroll
        for (int v = 0; v < 4; ++v) xt[k][v] = xs[(k * 64 + lane) * 4 + v];
#pragma unroll
    for (int j = 0; j < NT; ++j) {
        double a[4], z[4] = {0., 0., 0., 0.};
        load_afrag(tiles + trsm_slot<-1>(j, j) * 128, lane, a);
        tile_mma(a, xt[j], z);
#pragma unroll
        for (int v = 0; v < 4; ++v) xt[j][v] = z[v];
#pragma unroll
        for (int k = j + 1; k < NT; ++k) {
            double b[4];
            load_afrag(tiles + trsm_slot<-1>(k, j) * 128, lane, b);
            tile_mma(b, xt[j], xt[k]);
        }
        __builtin_amdgcn_sched_barrier(0);
    }
#pragma unroll
    for (int k = 0; k < NT; ++k) store_xtile_rows(Xc + 16 * k, ldx, lane, rows, xt[k]);
}

// ---------------------------------------------------------------------------
// back_sweep: X (rows, ncols) <- X * L^-1 for a fused factor L (ncols x ncols): row i becomes L^-T x_i, the backward
// counterpart of border_sweep for any number of rows (the predictive variance's gradient wants w = L^-T v for every test
// point).  The product is X L, not X L^T, so the summation index runs down the ROWS of L.  The tile product stays
// tile_mma's, Y[c][n] = sum_k M[c][k] X[n][k], with M = -L_(kc)^T: the <= 16 rows of X remain the B operand and the result
// comes back in X layout (it feeds the next product from its registers), and the A operand is read straight from memory
// TRANSPOSED -- a_v(lane) = -L[kap(lane >> 4, v)][rho(lane & 15)]: one 8-byte load per fragment element, the 16 lanes of
// a group covering one row's 128 bytes between them (a permutation of them), four rows per load instruction.
// One launch per 128-column block t, from the last to the first, t + 1 workgroups per 16-row group (blockIdx.y): workgroup
// b updates column block c = t - b with the block the launch before solved, X_c -= X_(t+1) L_(t+1, c), wave w its tiles w
// and 4 + w; workgroup 0 (c == t) then solves X_t <- X_t L_tt^-1 by the backward recurrence over the eight tiles, for
// j = 7 .. 0:  X_j <- X_j W_jj;  X_k -= X_j L_jk for k < j (one wave, 36 tile products), from operands staged in LDS: the
// transposed off-diagonal tiles, negated, and W_jj^T -- which is the stored diagonal tile as it lies in memory, strict
// upper part, with 1 / diag(L) on the diagonal and zeros below.  Launch t - 1 finds X_t final.  The order is the launch
// order; no workgroup waits for another, nothing is added atomically: the same bits every run.  The chain is ncols / 128
// launches whatever `rows` is; every row group streams L's lower triangle once per chain (groups beyond the first mostly
// out of L2).  Dead rows of the last group are fed as zeros and never stored.
// Reads of L: exactly what border_sweep reads -- the tiles below the block diagonal, and of the diagonal 128 x 128 blocks
// the lower 16 x 16 tiles and the diagonal tiles whole; never the block-upper tiles.
// ---------------------------------------------------------------------------
// x[v] = T[fr][kap(fg, v)] of the TRANSPOSE T of the 16 x 16 tile at p: X layout of L_jk^T for publish_tile
__device__ __forceinline__ void load_xtile_t(const double* p, int64_t ld, int lane, double (&x)[4]) {
    const int fr = lane & 15, fg = lane >> 4;
#pragma unroll
    for (int v = 0; v < 4; ++v) x[v] = p[(int64_t)kap(fg, v) * ld + fr];
}
// A-operand fragments of -M^T for the 16 x 16 tile M at `tile` in memory: a[v] = -M[kap(lane >> 4, v)][rho(lane & 15)]
__device__ __forceinline__ void load_afrag_t_neg(const double* tile, int64_t ld, int lane, double (&a)[4]) {
    const int i = lane & 15, kk = lane >> 4;
    const int col = kap(i & 3, i >> 2);                     // rho(i)
#pragma unroll
    for (int v = 0; v < 4; ++v) a[v] = -tile[(int64_t)kap(kk, v) * ld + col];
}
// slot of tile (j, k), k <= j, of the staged diagonal block
__device__ __forceinline__ constexpr int back_slot(int j, int k) { return j * (j + 1) / 2 + k; }

__global__ __launch_bounds__(256) void back_sweep_kernel(const double* __restrict__ L, int64_t ldl, double* X, int64_t ldx,
                                                         int64_t rows_all, int64_t t, int has_next) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    d2* tiles = reinterpret_cast<d2*>(smem);
    double* xs = reinterpret_cast<double*>(smem + NTILES * TILE_BYTES);
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int64_t cb = t - blockIdx.x;                      // the column block of X (and of L) of this workgroup
    const bool solver = blockIdx.x == 0;
    const int64_t row0 = (int64_t)16 * blockIdx.y;
    const int rows = (int)(rows_all - row0 < 16 ? rows_all - row0 : 16);
    X += row0 * ldx;
    if (solver) {
        // the 28 tiles below the diagonal of L_tt, transposed and negated, round-robin over the waves; the eight
        // diagonal tiles as W^T: the tile as stored above its diagonal, 1 / diag on it, zero below
        const double* Lb = L + (int64_t)PB * t * (ldl + 1);
        int q = 0;
#pragma unroll
        for (int j = 1; j < NT; ++j)
#pragma unroll
            for (int k = 0; k < j; ++k) {
                if ((q & 3) == wave) {
                    double x[4];
                    load_xtile_t(Lb + (int64_t)(16 * j) * ldl + 16 * k, ldl, lane, x);
                    publish_tile(tiles + back_slot(j, k) * 128, lane, x, -1.0);
                }
                ++q;
            }
#pragma unroll
        for (int r = 0; r < 2; ++r) {
            const int j = wave + 4 * r;
            const double* Ljj = Lb + (int64_t)(16 * j) * (ldl + 1);
            const int n = lane & 15, fg = lane >> 4;
            double x[4];
            load_xtile(Ljj, ldl, lane, x);                  // x[v] = G[n][kap(fg, v)]
#pragma unroll
            for (int v = 0; v < 4; ++v) {
                const int k = kap(fg, v);
                x[v] = (k > n) ? x[v] : (k == n) ? rcp_newton(x[v]) : 0.0;
            }
            publish_tile(tiles + back_slot(j, j) * 128, lane, x, 1.0);
        }
    }

    double* Xc = X + (int64_t)PB * cb;
    double acc[2][4];
#pragma unroll
    for (int p = 0; p < 2; ++p) load_xtile_rows(Xc + 16 * (wave + 4 * p), ldx, lane, rows, acc[p]);
    if (has_next) {
        const double* Xk = X + (int64_t)PB * (t + 1);
        double xk[NT][4];
#pragma unroll
        for (int j = 0; j < NT; ++j) load_xtile_rows(Xk + 16 * j, ldx, lane, rows, xk[j]);
#pragma unroll
        for (int p = 0; p < 2; ++p) {
            // rows of block t + 1 of L, the 16 columns of this wave's tile of block cb
            const double* Lr = L + ((int64_t)PB * (t + 1)) * ldl + (int64_t)PB * cb + 16 * (wave + 4 * p);
            double a[NT][4];
#pragma unroll
            for (int j = 0; j < NT; ++j) load_afrag_t_neg(Lr + (int64_t)(16 * j) * ldl, ldl, lane, a[j]);
#pragma unroll
            for (int j = 0; j < NT; ++j) tile_mma(a[j], xk[j], acc[p]);
        }
    }
    if (!solver) {
#pragma unroll
        for (int p = 0; p < 2; ++p) store_xtile_rows(Xc + 16 * (wave + 4 * p), ldx, lane, rows, acc[p]);
        return;
    }
    // workgroup 0: the updated block to wave 0 through LDS (lane-private slots), then the backward recurrence on it
#pragma unroll
    for (int p = 0; p < 2; ++p)
#pragma unroll
        for (int v = 0; v < 4; ++v) xs[((wave + 4 * p) * 64 + lane) * 4 + v] = acc[p][v];
    __syncthreads();
    if (wave != 0) return;
    double xt[NT][4];
#pragma unroll
    for (int k = 0; k < NT; ++k)
#pragma unroll
        for (int v = 0; v < 4; ++v) xt[k][v] = xs[(k * 64 + lane) * 4 + v];
#pragma unroll
    for (int j = NT - 1; j >= 0; --j) {
        double a[4], z[4] = {0., 0., 0., 0.};
        load_afrag(tiles + back_slot(j, j) * 128, lane, a);
        tile_mma(a, xt[j], z);
#pragma unroll
        for (int v = 0; v < 4; ++v) xt[j][v] = z[v];
#pragma unroll
        for (int k = 0; k < j; ++k) {
            double b[4];
            load_afrag(tiles + back_slot(j, k) * 128, lane, b);
            tile_mma(b, xt[j], xt[k]);
        }
        __builtin_amdgcn_sched_barrier(0);
    }
#pragma unroll
    for (int k = 0; k < NT; ++k) store_xtile_rows(Xc + 16 * k, ldx, lane, rows, xt[k]);
}

static hipError_t panel_mfma_attrs() {
    static PerDeviceOnce once;
    return once.run([]() -> hipError_t {
        hipError_t es = hipFuncSetAttribute((const void*)border_sweep_kernel, hipFuncAttributeMaxDynamicSharedMemorySize,
                                            SWEEP_LDS);
        if (es != hipSuccess) return es;
        es = hipFuncSetAttribute((const void*)back_sweep_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, SWEEP_LDS);
        if (es != hipSuccess) return es;
        hipError_t e = hipFuncSetAttribute((const void*)trsm128_kernel<-1>, hipFuncAttributeMaxDynamicSharedMemorySize,
                                           NTILES * TILE_BYTES);
        if (e != hipSuccess) return e;
        return hipFuncSetAttribute((const void*)vinv128_kernel, hipFuncAttributeMaxDynamicSharedMemorySize,
                                   NTILES * TILE_BYTES);
    });
}

hipError_t launch_potrf128(hipStream_t s, double* A, int64_t ld, int64_t col_offset, int64_t* info_dev) {
    if (ld % 2 || (reinterpret_cast<uintptr_t>(A) & 15)) return hipErrorInvalidValue;
    hipError_t e = panel_mfma_attrs();
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(potrf128_kernel, dim3(1), dim3(512), POTRF_TILES * TILE_BYTES + 16 * SCR_LD * 8, s, A, ld, col_offset,
                       info_dev, tuning().panel_stamps);
    return hipGetLastError();
}

hipError_t launch_trsm128(hipStream_t s, const double* L, int64_t ldl, double* X, int64_t ldx, int64_t m) {
    if (m <= 0) return hipSuccess;
    if (m % TRSM_ROWS || ldl % 2 || ldx % 2 || (reinterpret_cast<uintptr_t>(L) & 15) || (reinterpret_cast<uintptr_t>(X) & 15))
        return hipErrorInvalidValue;
    hipError_t e = panel_mfma_attrs();
    if (e != hipSuccess) return e;
    const int64_t nslabs = m / TRSM_ROWS;
    const unsigned grid = (unsigned)std::min<int64_t>(nslabs, 512);     // two workgroups per CU (72 KiB of LDS each)
    if (sharing().small_lds) {            // beside a trailing update: two launches that fit next to its workgroups
        hipLaunchKernelGGL(trsm128_kernel<0>, dim3(grid), dim3(256), trsm_tiles<0>() * TILE_BYTES, s, L, ldl, X, ldx, nslabs,
                           tuning().panel_stamps);
        hipLaunchKernelGGL(trsm128_kernel<1>, dim3(grid), dim3(256), trsm_tiles<1>() * TILE_BYTES, s, L, ldl, X, ldx, nslabs,
                           tuning().panel_stamps);
        return hipGetLastError();
    }
    hipLaunchKernelGGL(trsm128_kernel<-1>, dim3(grid), dim3(256), NTILES * TILE_BYTES, s, L, ldl, X, ldx, nslabs,
                       tuning().panel_stamps);
    return hipGetLastError();
}

hipError_t launch_border_sweep(hipStream_t s, const double* L, int64_t ldl, int64_t ncols, double* X, int64_t ldx,
                               int64_t rows) {
    if (rows < 1 || rows > 16 || ncols < 0 || ncols % PB || ldl % 2 || ldx % 2 || ldl < ncols || ldx < ncols ||
        (reinterpret_cast<uintptr_t>(L) & 15) || (reinterpret_cast<uintptr_t>(X) & 15))
        return hipErrorInvalidValue;
    if (ncols == 0) return hipSuccess;
    hipError_t e = panel_mfma_attrs();
    if (e != hipSuccess) return e;
    const int64_t nblk = ncols / PB;
    for (int64_t t = 0; t < nblk; ++t)
        hipLaunchKernelGGL(border_sweep_kernel, dim3((unsigned)(nblk - t)), dim3(256), SWEEP_LDS, s, L, ldl, X, ldx, (int)rows, t);
    return hipGetLastError();
}

hipError_t launch_back_sweep(hipStream_t s, const double* L, int64_t ldl, int64_t ncols, double* X, int64_t ldx,
                             int64_t rows) {
    if (rows < 1 || (rows + 15) / 16 > 65535 || ncols < 0 || ncols % PB || ldl % 2 || ldx % 2 || ldl < ncols || ldx < ncols ||
        (reinterpret_cast<uintptr_t>(L) & 15) || (reinterpret_cast<uintptr_t>(X) & 15))
        return hipErrorInvalidValue;
    if (ncols == 0) return hipSuccess;
    hipError_t e = panel_mfma_attrs();
    if (e != hipSuccess) return e;
    const int64_t nblk = ncols / PB;
    const unsigned groups = (unsigned)((rows + 15) / 16);
    for (int64_t t = nblk - 1; t >= 0; --t)
        hipLaunchKernelGGL(back_sweep_kernel, dim3((unsigned)(t + 1), groups), dim3(256), SWEEP_LDS, s, L, ldl, X, ldx, rows, t,
                           t + 1 < nblk ? 1 : 0);
    return hipGetLastError();
}

hipError_t launch_vinv128(hipStream_t s, double* A, int64_t ld, int64_t n, double* vside) {
    if (n <= 0 || n % PB || ld % 2 || (reinterpret_cast<uintptr_t>(A) & 15) || (reinterpret_cast<uintptr_t>(vside) & 15))
        return hipErrorInvalidValue;
    hipError_t e = panel_mfma_attrs();
    if (e != hipSuccess) return e;
    if (vside) {
        e = hipMemsetAsync(vside, 0, (size_t)n * PB * sizeof(double), s);
        if (e != hipSuccess) return e;
    }
    hipLaunchKernelGGL(vinv128_kernel, dim3((unsigned)(n / PB)), dim3(256), NTILES * TILE_BYTES, s, A, ld, vside);
    return hipGetLastError();
}

}  // namespace gpmi
