// gpmi_remove: k observations out of the resident regression factorisation in O(N^2 k) -- a positive rank-k update of
// the trailing factor instead of a new fit.  The plan (which indices each sweep takes, where it starts, where the y row
// goes) is remove_plan of gpmi_remove_plan.h; this file carries it out.
//
// With S the surviving indices, the rows S of the resident factor L satisfy L_S L_S^T = K_y[S, S]: L_S is lower
// trapezoidal with one extra column per removed index j, which is zero down to row j.  Plane rotations of the surviving
// columns against the extra ones, left to right, make it lower triangular again -- the factor of the surviving points.
// One pass over the old columns c >= J0 carries the extra columns as up to 16 ACTIVE VECTORS:
//   removed column c     not rotated, not written: its part below the diagonal (the y row's entry included) becomes
//                        the next active vector; row c is dropped
//   surviving column c   for each active vector i, in index order:  r = sqrt(d d + v_i[c]^2), cs = d / r, sn = v_i[c] / r,
//                        the diagonal d becomes r, and in every row below (the y row included)
//                        t = fma(cs, L_rc, sn v_ri);  v_ri = fma(cs, v_ri, -(sn L_rc));  L_rc = t
// Rows are independent; only the rotations are a chain (128 x (active vectors) dependent steps per diagonal block).
// tests/remove_ref.py states the same order in NumPy.
//
// Launches (the pattern of border_sweep_kernel, panel_mfma.hip): one per old 128-column block t from J0 on.  Workgroup
// b of launch t applies block t - 1's rotations -- read from a small device buffer the launch before wrote -- to the 128
// rows of row block t + b; workgroup 0 then takes the diagonal block t itself: column by column the lane that owns the
// diagonal row makes the rotations, the lanes below apply them.  The last workgroup of every launch is the y row's, and
// a last launch finishes it.  No workgroup waits for another and nothing is added atomically: the launch order is the
// order and every run gives the same bits.  Inside a workgroup L is read in 128-byte row pieces (16 columns of 128
// rows) and transposed through LDS, so that a lane owns a row with its <= 16 vector entries in registers; between
// launches these live in a side buffer of rows x 16 doubles.
//
// Every sweep is OUT OF PLACE: it reads the old buffer (never the strict block-upper 16 x 16 tiles of the diagonal
// 128-blocks, which hold L_kk^-T after a backward solve; diagonal 16 x 16 tiles masked to their lower triangle) and
// writes the surviving rows and columns, already shifted up and left, into a second buffer of the same shape.
#include "gpmi_remove_plan.h"
#include "gpmi_ctx.h"

namespace gpmi {

namespace {

constexpr int RB = 128;            // rows of a workgroup, columns of a launch
constexpr int RC = 16;             // columns of a piece: 128 bytes of a row
constexpr int RLD = RC + 1;        // LDS row stride of a piece (a lane reads its own row: no bank conflicts)
constexpr int RMAX = (int)REMOVE_MAX;

struct SweepArgs {
    const double* src;     // the old buffer
    double* dst;           // the new one, same leading dimension
    int64_t ld;
    int64_t N;             // old points
    int64_t J0;            // first old column the sweep touches (multiple of 128)
    int64_t nb;            // old 128-column blocks from J0 on
    int64_t yrow_src, yrow_dst;
    double* vbuf;          // (128 nb + 1) x 16: the active vectors' entries of old row J0 + slot; the last slot is the y row's
    double* rot;           // 2 x 128 x 16 x 2: (cs, sn) of a block's columns, two blocks alternating
    int q;                 // removed indices of this sweep
    int64_t idx[RMAX];     // ... ascending
};

// removed indices in front of position p (the shift of a surviving row or column)
__device__ __forceinline__ int below(const SweepArgs& a, int64_t p) {
    int n = 0;
#pragma unroll
    for (int i = 0; i < RMAX; ++i) n += (i < a.q && a.idx[i] < p) ? 1 : 0;
    return n;
}
__device__ __forceinline__ bool removed(const SweepArgs& a, int64_t p) {
    bool r = false;
#pragma unroll
    for (int i = 0; i < RMAX; ++i) r |= (i < a.q && a.idx[i] == p);
    return r;
}

// Per workgroup, once: rownew[rr] is the new row of piece row rr (-1: removed, padding, or no row at all), and per
// 128-column block colinfo[j] says of old column cbase + j how many removed indices lie in front of it (bits 0-7, the
// number of active vectors there and its shift to the left), whether it is removed itself (COL_GONE) or padding (COL_PAD)
// -- so that no lane counts indices per element.
constexpr int COL_GONE = 0x100, COL_PAD = 0x200;

struct Rows {
    int64_t base;          // old row of piece row 0; the y row's workgroup has base < 0 and one row
    int64_t yrow;
    __device__ __forceinline__ int64_t old_row(int rr) const { return base >= 0 ? base + rr : (rr == 0 ? yrow : -1); }
};

__device__ __forceinline__ void column_table(const SweepArgs& a, int64_t cbase, int* colinfo) {
    const int64_t c = cbase + threadIdx.x;
    colinfo[threadIdx.x] = c >= a.N ? COL_PAD : (below(a, c) | (removed(a, c) ? COL_GONE : 0));
}

// A 128 x 16 piece between memory and LDS, 128 threads: thread (tid & 15) takes a column, (tid >> 4) + 8 k the rows;
// `tri`: only c <= row is read or written (a diagonal block).
__device__ __forceinline__ void piece_load(const SweepArgs& a, const Rows& rows, const int64_t* rownew, int ci, int64_t c0,
                                           bool tri, double* tile) {
    const int cc = threadIdx.x & 15;
    const int64_t c = c0 + cc;
#pragma unroll 4
    for (int k = 0; k < RB / 8; ++k) {
        const int rr = (threadIdx.x >> 4) + 8 * k;
        const int64_t r = rows.old_row(rr);
        double v = 0.0;
        if (rownew[rr] >= 0 && !(ci & COL_PAD) && (!tri || c <= r)) v = a.src[r * a.ld + c];
        tile[rr * RLD + cc] = v;
    }
}

__device__ __forceinline__ void piece_store(const SweepArgs& a, const Rows& rows, const int64_t* rownew, int ci, int64_t c0,
                                            bool tri, const double* tile) {
    const int cc = threadIdx.x & 15;
    const int64_t c = c0 + cc;
    if (ci & (COL_PAD | COL_GONE)) return;
    const int64_t cn = c - (ci & 0xff);
#pragma unroll 4
    for (int k = 0; k < RB / 8; ++k) {
        const int rr = (threadIdx.x >> 4) + 8 * k;
        const int64_t rn = rownew[rr];
        if (rn < 0 || (tri && c > rows.old_row(rr))) continue;
        a.dst[rn * a.ld + cn] = tile[rr * RLD + cc];
    }
}

// one rotation on a lane's pair (L_rc, v_ri)
__device__ __forceinline__ void rotate(double cs, double sn, double& l, double& v) {
    const double t = fma(cs, l, sn * v);
    v = fma(cs, v, -(sn * l));
    l = t;
}

__global__ __launch_bounds__(RB) void remove_sweep_kernel(SweepArgs a, int64_t t) {
    __shared__ double tile[RB * RLD];
    __shared__ double srot[RB * RMAX * 2];      // a block's (cs, sn): the one being applied, then the one being made
    __shared__ int64_t rownew[RB];
    __shared__ int colinfo[RB];
    const int tid = threadIdx.x;
    const bool yrow_wg = (int64_t)blockIdx.x == a.nb - t;
    const int64_t rb = t + blockIdx.x;                                   // row block (from J0) of a factor workgroup
    if (t == 0 && !yrow_wg && blockIdx.x != 0) return;                    // nothing in front of the first block
    Rows rows;
    rows.base = yrow_wg ? -1 : a.J0 + rb * RB;
    rows.yrow = a.yrow_src;
    const int64_t r = rows.old_row(tid);                                  // this lane's old row
    const bool live = yrow_wg ? tid == 0 : (r < a.N && !removed(a, r));   // ... and whether it survives
    const int64_t slot = yrow_wg ? a.nb * RB : rb * RB + tid;
    rownew[tid] = !live ? -1 : (yrow_wg ? a.yrow_dst : r - below(a, r));

    double v[RMAX];
#pragma unroll
    for (int i = 0; i < RMAX; ++i) v[i] = 0.0;
    if (t > 0 && live) {
#pragma unroll
        for (int i = 0; i < RMAX; ++i)
            if (i < a.q) v[i] = a.vbuf[slot * RMAX + i];
    }

    // ---- block t - 1's rotations on this workgroup's rows
    if (t > 0) {
        const int64_t cbase = a.J0 + (t - 1) * RB;
        const double* rot = a.rot + ((t - 1) & 1) * (RB * RMAX * 2);
        for (int e = tid; e < RB * RMAX * 2; e += RB) srot[e] = rot[e];
        column_table(a, cbase, colinfo);
        __syncthreads();
        for (int ch = 0; ch < RB / RC; ++ch) {
            const int64_t c0 = cbase + RC * ch;
            if (c0 >= a.N) break;                                         // uniform: the padding's columns
            const int my_ci = colinfo[RC * ch + (tid & 15)];
            piece_load(a, rows, rownew, my_ci, c0, false, tile);
            __syncthreads();
            if (live) {
                double x[RC];
#pragma unroll
                for (int cc = 0; cc < RC; ++cc) x[cc] = tile[tid * RLD + cc];
#pragma unroll
                for (int cc = 0; cc < RC; ++cc) {
                    const int ci = __builtin_amdgcn_readfirstlane(colinfo[RC * ch + cc]);
                    const int na = ci & 0xff;
                    if (ci & COL_PAD) continue;
                    if (ci & COL_GONE) {
#pragma unroll
                        for (int i = 0; i < RMAX; ++i)
                            if (i == na) v[i] = x[cc];
                    } else {
                        const double* rc = srot + (RC * ch + cc) * (RMAX * 2);
#pragma unroll
                        for (int i = 0; i < RMAX; ++i)
                            if (i < na) rotate(rc[2 * i], rc[2 * i + 1], x[cc], v[i]);
                    }
                }
#pragma unroll
                for (int cc = 0; cc < RC; ++cc) tile[tid * RLD + cc] = x[cc];
            }
            __syncthreads();
            piece_store(a, rows, rownew, my_ci, c0, false, tile);
            __syncthreads();
        }
    }
    if (yrow_wg || blockIdx.x != 0) {
        if (live) {
#pragma unroll
            for (int i = 0; i < RMAX; ++i)
                if (i < a.q) a.vbuf[slot * RMAX + i] = v[i];
        }
        return;
    }

    // ---- workgroup 0: the diagonal block t, its rotations made and applied column by column
    const int64_t cbase = a.J0 + t * RB;
    double* rot = a.rot + (t & 1) * (RB * RMAX * 2);
    column_table(a, cbase, colinfo);                     // every lane is past its last read of the table of block t - 1
    __syncthreads();
    for (int ch = 0; ch < RB / RC; ++ch) {
        const int64_t c0 = cbase + RC * ch;
        if (c0 >= a.N) break;
        const int my_ci = colinfo[RC * ch + (tid & 15)];
        piece_load(a, rows, rownew, my_ci, c0, true, tile);
        __syncthreads();
        double x[RC];
#pragma unroll
        for (int cc = 0; cc < RC; ++cc) x[cc] = tile[tid * RLD + cc];
#pragma unroll
        for (int cc = 0; cc < RC; ++cc) {
            const int64_t c = c0 + cc;
            const int ci = __builtin_amdgcn_readfirstlane(colinfo[RC * ch + cc]);
            const int na = ci & 0xff;
            if (ci & COL_PAD) continue;                                   // uniform
            if (ci & COL_GONE) {                                          // uniform
                if (live && r > c) {
#pragma unroll
                    for (int i = 0; i < RMAX; ++i)
                        if (i == na) v[i] = x[cc];
                }
                continue;
            }
            if (na == 0) continue;                                        // uniform: no vector is active yet
            if (r == c) {                                                 // the diagonal row's lane: the chain
                double d = x[cc];
#pragma unroll
                for (int i = 0; i < RMAX; ++i)
                    if (i < na) {
                        const double h = sqrt(fma(d, d, v[i] * v[i]));
                        const double cs = d / h, sn = v[i] / h;
                        srot[((RC * ch + cc) * RMAX + i) * 2] = cs;
                        srot[((RC * ch + cc) * RMAX + i) * 2 + 1] = sn;
                        d = h;
                    }
                x[cc] = d;
            }
            __syncthreads();
            if (live && r > c) {
#pragma unroll
                for (int i = 0; i < RMAX; ++i)
                    if (i < na) rotate(srot[((RC * ch + cc) * RMAX + i) * 2], srot[((RC * ch + cc) * RMAX + i) * 2 + 1], x[cc], v[i]);
            }
        }
        __syncthreads();
#pragma unroll
        for (int cc = 0; cc < RC; ++cc) tile[tid * RLD + cc] = x[cc];
        __syncthreads();
        piece_store(a, rows, rownew, my_ci, c0, true, tile);
        __syncthreads();
    }
    // the block's rotations for the next launch, in one go (a store per column would put a trip to memory in front of
    // every barrier of the chain); entries of removed columns and of inactive vectors are never read
    for (int e = tid; e < RB * RMAX * 2; e += RB) rot[e] = srot[e];
}

// the surviving rows from J0 on (and the y row): their columns below J0 are final and only move up
__global__ __launch_bounds__(256) void remove_shift_rows_kernel(SweepArgs a) {
    const int64_t nrows = a.N - a.J0;                       // blockIdx.x == nrows: the y row
    const bool yr = (int64_t)blockIdx.x == nrows;
    const int64_t r = yr ? a.yrow_src : a.J0 + blockIdx.x;
    if (!yr && removed(a, r)) return;
    const int64_t rn = yr ? a.yrow_dst : r - below(a, r);
    const double* s = a.src + r * a.ld;
    double* d = a.dst + rn * a.ld;
    for (int64_t c = (int64_t)blockIdx.y * 256 + threadIdx.x; c < a.J0; c += (int64_t)gridDim.y * 256) d[c] = s[c];
}

// The new buffer from J0 on before the sweep writes into it: block b zeroes the diagonal 128 x 128 block of new row block
// J0 / 128 + b (the sweep writes lower triangles only), puts the identity on the padding's diagonal and zeroes the
// padding rows' columns in front of the block.
__global__ __launch_bounds__(RB) void remove_prepare_kernel(double* dst, int64_t ld, int64_t J0, int64_t N_out) {
    const int64_t b0 = J0 + (int64_t)blockIdx.x * RB;
    for (int rr = 0; rr < RB; ++rr) {
        const int64_t row = b0 + rr;
        double* p = dst + row * ld;
        p[b0 + threadIdx.x] = (row >= N_out && threadIdx.x == rr) ? 1.0 : 0.0;
        if (row >= N_out)
            for (int64_t c = threadIdx.x; c < b0; c += RB) p[c] = 0.0;
    }
}

// W_jj = L_jj^-1 of the 16 x 16 diagonal tiles from tile0 on, TRANSPOSED strictly above the diagonal (tile[c][r] =
// W[r][c], r > c; the diagonal of W stays implied: the convention of factor_diag_tile, panel_mfma.hip).  One wave per
// tile; lane c < 16 solves L w = e_c by forward substitution.
__global__ __launch_bounds__(64) void remove_tile_inverse_kernel(double* A, int64_t ld, int64_t tile0) {
    const int64_t o = (tile0 + blockIdx.x) * 16;
    double* T = A + o * ld + o;
    const int c = threadIdx.x;
    if (c >= 16) return;
    double w[16];
#pragma unroll
    for (int r = 0; r < 16; ++r) {
        double s = 0.0;
#pragma unroll
        for (int k = 0; k < 16; ++k)
            if (k < r && k >= c) s = fma(T[(int64_t)r * ld + k], w[k], s);
        const double d = T[(int64_t)r * ld + r];
        w[r] = r < c ? 0.0 : (r == c ? 1.0 / d : -s / d);
    }
#pragma unroll
    for (int r = 0; r < 16; ++r)
        if (r > c) T[(int64_t)c * ld + r] = w[r];
}

// out[i][:] = in[keep[i]][:] for a row-major n_out x d array
__global__ __launch_bounds__(256) void remove_gather_kernel(const double* in, const int64_t* keep, int64_t n_out, int64_t d,
                                                            double* out) {
    const int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (e >= n_out * d) return;
    const int64_t i = e / d, k = e - i * d;
    out[e] = in[keep[i] * d + k];
}

struct Holder {                // a buffer until the context owns it
    DevBuf b;
    ~Holder() { b.release(); }
};

hipError_t run_sweep(gpmi_ctx* c, const RemovePlan& p, const RemoveSweep& sw, const double* src, double* dst) {
    hipStream_t s = c->stream;
    const int64_t ld = p.ld;
    SweepArgs a;
    a.src = src; a.dst = dst; a.ld = ld; a.N = sw.N_in; a.J0 = sw.J0; a.nb = sw.blocks;
    a.yrow_src = sw.yrow_in; a.yrow_dst = sw.yrow_out;
    a.vbuf = c->rem.as<double>();
    a.rot = a.vbuf + (sw.blocks * RB + 1) * RMAX;
    a.q = (int)sw.count;
    for (int i = 0; i < RMAX; ++i) a.idx[i] = i < a.q ? p.sorted[(size_t)(sw.first + i)] : -1;
    hipError_t e;
    // ---- what only moves, and the new buffer's padding
    size_t sp = c->span_begin(GPMI_T_KS);
    if (sw.J0 > 0) {
        e = hipMemcpy2DAsync(dst, (size_t)ld * 8, src, (size_t)ld * 8, (size_t)sw.J0 * 8, (size_t)sw.J0, hipMemcpyDeviceToDevice, s);
        if (e != hipSuccess) return e;
    }
    if (sw.Np_out > sw.J0) {
        hipLaunchKernelGGL(remove_prepare_kernel, dim3((unsigned)((sw.Np_out - sw.J0) / RB)), dim3(RB), 0, s, dst, ld, sw.J0, sw.N_out);
        if ((e = hipGetLastError()) != hipSuccess) return e;
    }
    // the y block's 128 rows are zeroed first and then carry m'
    if ((e = launch_fill_rows(s, dst + sw.yrow_out * ld, ld, TILE, sw.Np_out, 0.0)) != hipSuccess) return e;
    if (sw.J0 > 0) {
        const unsigned gy = (unsigned)std::min<int64_t>((sw.J0 + 255) / 256, 64);
        hipLaunchKernelGGL(remove_shift_rows_kernel, dim3((unsigned)(sw.N_in - sw.J0 + 1), gy), dim3(256), 0, s, a);
        if ((e = hipGetLastError()) != hipSuccess) return e;
    }
    c->span_end(sp);
    // ---- the sweep
    sp = c->span_begin(GPMI_T_SOLVE_V);
    if ((e = hipMemsetAsync(a.vbuf, 0, (size_t)(sw.blocks * RB + 1) * RMAX * 8, s)) != hipSuccess) return e;
    for (int64_t t = 0; t <= sw.blocks; ++t) {
        hipLaunchKernelGGL(remove_sweep_kernel, dim3((unsigned)(sw.blocks - t + 1)), dim3(RB), 0, s, a, t);
        if ((e = hipGetLastError()) != hipSuccess) return e;
    }
    c->span_end(sp);
    return hipSuccess;
}

}  // namespace

int remove_impl(gpmi_ctx* c, const int64_t* idx, int64_t k, double* lml) {
    if (!c->res.regression()) return fail_arg("gpmi_remove: no factorisation resident");
    const int64_t N = c->N, d = c->d;
    const RemovePlan p = remove_plan(N, idx, k, c->ldA, c->rows_cap, c->yrow, c->ld_pad);
    if (!p.ok) return fail_arg(p.why);
    const int64_t N1 = p.N_out;
    const int fused = c->res.factor_fused;
    hipStream_t s = c->stream;

    // ---- everything that can fail for want of memory, before anything of the resident fit changes
    const size_t bytes = (size_t)p.rows * p.ld * sizeof(double);
    Holder other;                                           // the second buffer: the spare one when it has the shape
    if (c->spareA.cap >= bytes) {
        other.b = c->spareA;
        c->spareA = DevBuf();
    } else {
        c->spareA.release();
        const hipError_t e = other.b.ensure(bytes);
        if (e != hipSuccess) {
            (void)hipGetLastError();
            return fail_runtime(e, "gpmi_remove: the second factor buffer");
        }
    }
    Holder Xn, yn, Xzn;                                     // the compacted training set, at the old buffers' capacity
    const int64_t Np = round_up(N, TILE);
    const size_t side = (size_t)((Np + 1) * RMAX + 2 * RB * RMAX * 2) * 8, keep_off = round_up((int64_t)side, 16);
    hipError_t e = c->rem.ensure(keep_off + (size_t)N1 * 8);
    if (e == hipSuccess) e = Xn.b.ensure(std::max(c->X.cap, (size_t)N1 * d * 8));
    if (e == hipSuccess) e = yn.b.ensure(std::max(c->y.cap, (size_t)N1 * 8));
    if (e == hipSuccess && c->ard()) e = Xzn.b.ensure(std::max(c->Xz.cap, (size_t)N1 * d * 8));
    if (e != hipSuccess) {
        (void)hipGetLastError();
        if (c->remove_keep_spare) std::swap(c->spareA, other.b);        // nothing changed: the spare one stays kept
        return fail_runtime(e, "gpmi_remove: workspace");
    }

    // ---- the training set: X, y and the scaled copy compacted on the device, order preserved; the lanes' copies are
    // stale.  From here on a failure leaves no fit and the reduced training set, N = N - k at once (gpmi_factorize lays A
    // out anew from N alone); success puts the resident state back, shrunk.  The boxes stay: a box of a superset bounds
    // every squared distance of the subset, and the K build drops its exp domain test only when the BOUND keeps the
    // argument in the domain (gpmi_kroute.h: nocheck needs coef * max_sq >= -690), so a larger bound can only keep a test
    // the exact box would have dropped.
    c->N = N1;
    const Resident before = c->res;
    c->res.drop_fit();
    c->timers_reset({GPMI_T_KS, GPMI_T_SOLVE_V, GPMI_T_CHOL, GPMI_T_LML});
    {
        std::vector<int64_t> keep((size_t)N1);
        size_t ri = 0;
        int64_t o = 0;
        for (int64_t i = 0; i < N; ++i) {
            if (ri < p.sorted.size() && p.sorted[ri] == i) { ++ri; continue; }
            keep[(size_t)o++] = i;
        }
        int64_t* keep_dev = reinterpret_cast<int64_t*>(c->rem.as<char>() + keep_off);
        HIP_TRY(hipMemcpy(keep_dev, keep.data(), (size_t)N1 * 8, hipMemcpyHostToDevice));
        const unsigned gx = (unsigned)((N1 * d + 255) / 256), gy = (unsigned)((N1 + 255) / 256);
        LAUNCH_TRY(remove_gather_kernel, dim3(gx), dim3(256), 0, s, c->X.as<double>(), keep_dev, N1, d, Xn.b.as<double>());
        LAUNCH_TRY(remove_gather_kernel, dim3(gy), dim3(256), 0, s, c->y.as<double>(), keep_dev, N1, (int64_t)1, yn.b.as<double>());
        if (c->ard())
            LAUNCH_TRY(remove_gather_kernel, dim3(gx), dim3(256), 0, s, c->Xz.as<double>(), keep_dev, N1, d, Xzn.b.as<double>());
        HIP_TRY(hipStreamSynchronize(s));
        std::swap(c->X, Xn.b);
        std::swap(c->y, yn.b);
        if (c->ard()) std::swap(c->Xz, Xzn.b);
    }
    for (gpmi_ctx* l : c->lane_ctx) l->res.drop_train();

    // ---- the sweeps, the two buffers alternating
    double* cur = c->A.as<double>();
    double* nxt = other.b.as<double>();
    for (const RemoveSweep& sw : p.sweeps) {
        HIP_TRY(run_sweep(c, p, sw, cur, nxt));
        std::swap(cur, nxt);
    }
    const int64_t ld = p.ld;
    // ---- the stored inverses of the new diagonal tiles (a first-generation factor has none: it stays of one kind)
    if (fused) {
        const size_t sp = c->span_begin(GPMI_T_CHOL);
        const int64_t tile0 = p.first_tile, ntiles = p.Np_out / 16 - tile0;
        if (ntiles > 0) LAUNCH_TRY(remove_tile_inverse_kernel, dim3((unsigned)ntiles), dim3(64), 0, s, cur, ld, tile0);
        c->span_end(sp);
    }
    size_t sp = c->span_begin(GPMI_T_LML);
    HIP_TRY(launch_lml_reduce(s, cur, ld, cur + p.yrow_out * ld, N1, c->red.as<double>()));
    c->span_end(sp);
    double red[2];
    HIP_TRY(hipMemcpyAsync(red, c->red.p, sizeof red, hipMemcpyDeviceToHost, s));
    HIP_TRY(hipStreamSynchronize(s));
    c->timers_collect();

    // ---- the context describes the result; the other buffer is freed or kept for the next removal
    if (cur != c->A.as<double>()) std::swap(c->A, other.b);
    if (c->remove_keep_spare) std::swap(c->spareA, other.b);
    c->Np = p.Np_out; c->Mp = p.Np_out + TILE; c->yrow = p.yrow_out;
    if (lml) *lml = -.5 * red[1] - red[0] - (double)N1 / 2.0 * std::log(2 * M_PI);
    c->res = before;
    c->res.factor_shrunk(fused);
    return GPMI_OK;
}

}  // namespace gpmi
