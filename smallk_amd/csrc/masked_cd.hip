// smallk_amd/csrc/masked_cd.hip -- the kernels of NMF fitted to the stored entries only (masked_cd.cpp): cyclic
// coordinate descent on  1/2 sum over Omega of (a - w_i . h_j)^2 + penalties,  Omega = the stored entries of a sparse matrix, stored
// zeros included; an entry that is not stored is "not measured", not 0.  Both half-iterations are one sweep over one CSC -- CSC(A)
// for H, CSC(A') for W; below, "column" is a column of that CSC, X (KP x ncols) the factor being updated and G (KP x nrows) the
// factor whose rows the entries name.  With a mask the Gram matrix differs from column to column, so none is formed: the sweep keeps
// the residuals r_e = a_e - g_{i_e} . x_j of the column current instead (Gauss-Seidel), and for t = 0 .. k-1 in order
//     grad = -sum_e G[i_e, t] r_e + l1 + l2 x[t],   hess = sum_e G[i_e, t]^2 + l2
//     pg   = x[t] == 0 ? min(0, grad) : grad,       violation += |pg|
//     unless hess == 0:  xn = max(x[t] - grad / hess, 0),  r_e -= G[i_e, t] (xn - x[t]),  x[t] = xn
// Work is cut by the SegPlan of spmm_seg.hip.  A column that fits a segment (<= 64 entries: the driver refuses longer segments)
// belongs to the SIXTEEN-lane group that owns the segment; the group takes the whole columns of its segment one after another, a
// lane holds entries l, l + 16, l + 32, l + 48 of the column and their residuals in registers, x lives in the group's corner of
// LDS.  Per step the two sums are reduced over the sixteen lanes by DPP row operations (group_sum<16>: a fixed tree, the total in
// every lane), so every lane applies the same update to its residuals.  G[i_e, t] is reloaded in chunks of 8 consecutive t (one
// 64-byte line, 16-byte loads) kept for eight steps.  A column longer than a segment belongs to one workgroup; its residuals live
// in `res` (nnz doubles, indexed like the CSC), its sums are reduced lane tree first, then the four waves in index order through
// LDS.  Columns without stored entries follow the same formulas with empty sums (masked_empty_kernel).  No floating-point
// atomics, no fix-up launch: the same bits on every run.  Rows >= k of both factors are selected to zero on the way in, whatever
// they hold, and X's are written as zeros.
#include <algorithm>

#include "common.h"
#include "devutil.h"

namespace smk {

static constexpr unsigned MK_ROW = 0x7FFFFFFFu;          // (bit 31 of the plan's row indices flags the last entry of a column)
static constexpr unsigned MK_NO_PIECE = 0xFFFFFFFFu;
static constexpr int MK_E = 4;                            // entries of a column per lane: 16 lanes x 4 = the longest segment served

int masked_seg_len_max() { return 16 * MK_E; }

// the wave's own LDS traffic has landed and the compiler keeps later LDS accesses behind it (a group never leaves its wave)
__device__ __forceinline__ void mk_lds_settle()
{
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
    __builtin_amdgcn_wave_barrier();
}

// 8 consecutive doubles: one 64-byte line in four 16-byte loads
__device__ __forceinline__ void mk_load8(const double* __restrict__ p, double (&w)[8])
{
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const f64x2_t v = *(const f64x2_t*)(p + 2 * i);
        w[2 * i] = v[0];
        w[2 * i + 1] = v[1];
    }
}

// the coordinate step every lane takes alike: returns the new value, adds |pg| to viol, *d = new - old (0 where hess == 0)
__device__ __forceinline__ double mk_step(double xt, double g, double h, double l1, double l2, double& viol, double* d)
{
    const double grad = __builtin_fma(l2, xt, l1 - g), hess = h + l2;
    const double pg = xt == 0.0 ? fmin(grad, 0.0) : grad;
    viol += fabs(pg);
    const double xn = hess != 0.0 ? fmax(xt - grad / hess, 0.0) : xt;
    *d = xn - xt;
    return xn;
}

// The entries [cs, cs + cl) of one column (cl <= 64) over the sixteen lanes of a group: lane l takes cs + l + 16 u.  off: the
// offset of the entry's row in G (an entry past the column: that of the column's first entry, loaded and not used), r: the
// residual against the x in xs (rows >= k of G are not relied on; xs holds zeros there); an entry past the column gets r = a = 0.
template <int KP>
__device__ __forceinline__ void mk_column_residual(const unsigned* __restrict__ rowflag, const double* __restrict__ val,
                                                   const double* __restrict__ G, const double* xs, int k, i64 cs, int cl, int l,
                                                   i64 (&off)[MK_E], bool (&act)[MK_E], double (&a)[MK_E], double (&r)[MK_E])
{
#pragma unroll
    for (int u = 0; u < MK_E; ++u) {
        const int q = l + 16 * u;
        act[u] = q < cl;
        const i64 p = cs + (act[u] ? q : 0);
        off[u] = (i64)(rowflag[p] & MK_ROW) * KP;
        const double v = val[p];
        a[u] = act[u] ? v : 0.0;
        r[u] = 0.0;
    }
    for (int t0 = 0; t0 < k; t0 += 8) {
        double x[8];
#pragma unroll
        for (int tt = 0; tt < 8; ++tt) x[tt] = xs[t0 + tt];
#pragma unroll
        for (int u = 0; u < MK_E; ++u) {
            if (16 * u < cl) {              // (uniform over the group: a column of <= 16 entries fills one slot per lane, not four)
                double w[8];
                mk_load8(G + off[u] + t0, w);
#pragma unroll
                for (int tt = 0; tt < 8; ++tt) r[u] = __builtin_fma(t0 + tt < k ? w[tt] : 0.0, x[tt], r[u]);
            }
        }
    }
#pragma unroll
    for (int u = 0; u < MK_E; ++u) r[u] = act[u] ? a[u] - r[u] : 0.0;
}

// the columns that fit a segment: a group of sixteen lanes per segment, sixteen segments per workgroup; viol_partials[blockIdx.x]
template <int KP>
__global__ __launch_bounds__(256) void masked_sweep_kernel(const i64* __restrict__ seg_p0, const unsigned* __restrict__ seg_len,
                                                           const unsigned* __restrict__ seg_col, const unsigned* __restrict__ seg_piece,
                                                           i64 nseg, const i64* __restrict__ colptr, const unsigned* __restrict__ rowflag,
                                                           const double* __restrict__ val, const double* __restrict__ G, double* X, int k,
                                                           double l1, double l2, double* __restrict__ viol_partials)
{
    __shared__ __attribute__((aligned(16))) double xs_all[16][KP];
    __shared__ double sh[4];
    const i64 sg = (i64)blockIdx.x * 16 + threadIdx.x / 16;
    const int l = threadIdx.x % 16;
    double* xs = xs_all[threadIdx.x / 16];
    double viol = 0.0;
    if (sg < nseg && seg_piece[sg] == MK_NO_PIECE) {          // (uniform over the group; the pieces of long columns: masked_long_kernel)
        i64 cs = seg_p0[sg];
        const i64 pend = cs + seg_len[sg];
        i64 j = seg_col[sg];
        while (cs < pend) {
            while (colptr[j + 1] <= cs) ++j;                  // columns without stored entries
            const i64 ce = colptr[j + 1];
            const int cl = (int)(ce - cs);
#pragma unroll
            for (int c = 0; c < (KP + 15) / 16; ++c) {
                const int row = l + 16 * c;
                if (row < KP) { const double v = X[j * KP + (row < k ? row : 0)]; xs[row] = row < k ? v : 0.0; }
            }
            mk_lds_settle();
            i64 off[MK_E];
            bool act[MK_E];
            double a[MK_E], r[MK_E];
            mk_column_residual<KP>(rowflag, val, G, xs, k, cs, cl, l, off, act, a, r);
            for (int t0 = 0; t0 < k; t0 += 8) {
                double w[MK_E][8];
#pragma unroll
                for (int u = 0; u < MK_E; ++u) {
                    if (16 * u < cl) {                         // (uniform over the group: a slot no lane fills is not loaded)
                        mk_load8(G + off[u] + t0, w[u]);
#pragma unroll
                        for (int tt = 0; tt < 8; ++tt) w[u][tt] = act[u] ? w[u][tt] : 0.0;
                    } else {
#pragma unroll
                        for (int tt = 0; tt < 8; ++tt) w[u][tt] = 0.0;
                    }
                }
#pragma unroll
                for (int tt = 0; tt < 8; ++tt) {
                    const int t = t0 + tt;
                    if (t < k) {
                        double g = 0.0, h = 0.0;
#pragma unroll
                        for (int u = 0; u < MK_E; ++u) {
                            if (16 * u < cl) {
                                g = __builtin_fma(w[u][tt], r[u], g);
                                h = __builtin_fma(w[u][tt], w[u][tt], h);
                            }
                        }
                        g = group_sum<16>(g);
                        h = group_sum<16>(h);
                        double d;
                        const double xn = mk_step(xs[t], g, h, l1, l2, viol, &d);
#pragma unroll
                        for (int u = 0; u < MK_E; ++u)
                            if (16 * u < cl) r[u] = __builtin_fma(-w[u][tt], d, r[u]);
                        if (l == 0) xs[t] = xn;
                    }
                }
            }
            mk_lds_settle();
#pragma unroll
            for (int c = 0; c < (KP + 15) / 16; ++c) {
                const int row = l + 16 * c;
                if (row < KP) X[j * KP + row] = row < k ? xs[row] : 0.0;
            }
            mk_lds_settle();                                  // the next column overwrites xs
            cs = ce;
            ++j;
        }
    }
    const double tot = block_sum(l == 0 ? viol : 0.0, sh);    // (every lane of a group holds the same viol: one of them counts)
    if (threadIdx.x == 0) viol_partials[blockIdx.x] = tot;
}

// a column longer than a segment: one workgroup.  Thread i takes the entries cs + i, cs + i + 256, ..; their residuals live in res.
// The update of step t - 1 is applied to a residual on the way into step t: one pass over the column per step.
template <int KP>
__global__ __launch_bounds__(256) void masked_long_kernel(const unsigned* __restrict__ long_col, const i64* __restrict__ colptr,
                                                          const unsigned* __restrict__ rowflag, const double* __restrict__ val,
                                                          const double* __restrict__ G, double* X, int k, double l1, double l2,
                                                          double* __restrict__ res, double* __restrict__ viol_partials)
{
    __shared__ double xs[KP], xnew[KP];
    __shared__ double sh[2][4][2];
    const i64 j = long_col[blockIdx.x];
    const i64 cs = colptr[j], ce = colptr[j + 1];
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    for (int row = threadIdx.x; row < KP; row += 256) {
        const double v = X[j * KP + (row < k ? row : 0)];
        xs[row] = xnew[row] = row < k ? v : 0.0;
    }
    __syncthreads();
    for (i64 p = cs + threadIdx.x; p < ce; p += 256) {
        const double* __restrict__ gr = G + (i64)(rowflag[p] & MK_ROW) * KP;
        double acc = 0.0;
        for (int t0 = 0; t0 < k; t0 += 8) {
            double w[8];
            mk_load8(gr + t0, w);
#pragma unroll
            for (int tt = 0; tt < 8; ++tt) acc = __builtin_fma(t0 + tt < k ? w[tt] : 0.0, xs[t0 + tt], acc);
        }
        res[p] = val[p] - acc;
    }
    double viol = 0.0, dprev = 0.0;
    for (int t = 0; t < k; ++t) {
        double g = 0.0, h = 0.0;
        for (i64 p = cs + threadIdx.x; p < ce; p += 256) {
            const double* __restrict__ gr = G + (i64)(rowflag[p] & MK_ROW) * KP;
            double r = res[p];
            if (t > 0) { r = __builtin_fma(-gr[t - 1], dprev, r); res[p] = r; }
            const double wt = gr[t];
            g = __builtin_fma(wt, r, g);
            h = __builtin_fma(wt, wt, h);
        }
        g = wave_sum(g);
        h = wave_sum(h);
        const int par = t & 1;              // two slots: a wave may write step t + 1 while another still reads step t
        if (lane == 0) { sh[par][wv][0] = g; sh[par][wv][1] = h; }
        __syncthreads();
        g = ((sh[par][0][0] + sh[par][1][0]) + sh[par][2][0]) + sh[par][3][0];
        h = ((sh[par][0][1] + sh[par][1][1]) + sh[par][2][1]) + sh[par][3][1];
        const double xn = mk_step(xs[t], g, h, l1, l2, viol, &dprev);
        if (threadIdx.x == 0) xnew[t] = xn;
    }
    __syncthreads();
    for (int row = threadIdx.x; row < KP; row += 256) X[j * KP + row] = row < k ? xnew[row] : 0.0;
    if (threadIdx.x == 0) viol_partials[blockIdx.x] = viol;
}

// columns without stored entries: both sums are empty, the coordinates do not couple -- untouched when l2 == 0, shrunk otherwise
__global__ __launch_bounds__(256) void masked_empty_kernel(const i64* __restrict__ colptr, i64 ncols, double* __restrict__ X, int KP, int k,
                                                           double l1, double l2, double* __restrict__ viol_partials)
{
    __shared__ double sh[4];
    const i64 stride = (i64)gridDim.x * blockDim.x;
    double viol = 0.0;
    for (i64 j = (i64)blockIdx.x * blockDim.x + threadIdx.x; j < ncols; j += stride) {
        if (colptr[j + 1] != colptr[j]) continue;
        for (int t = 0; t < KP; ++t) {
            double d, xn = 0.0;
            if (t < k) xn = mk_step(X[j * KP + t], 0.0, 0.0, l1, l2, viol, &d);
            X[j * KP + t] = xn;
        }
    }
    const double tot = block_sum(viol, sh);
    if (threadIdx.x == 0) viol_partials[blockIdx.x] = tot;
}

// sum over Omega of (a - g_i . x_j)^2 and of a^2: a group of sixteen lanes per segment, whole columns or one piece of a long one;
// per segment to segpart[2 sg], segpart[2 sg + 1] (the columns of the segment in order); with col_r: per column, a piece to
// piecepart[2 piece], [2 piece + 1]
template <int KP>
__global__ __launch_bounds__(256) void masked_residual_kernel(const i64* __restrict__ seg_p0, const unsigned* __restrict__ seg_len,
                                                              const unsigned* __restrict__ seg_col, const unsigned* __restrict__ seg_piece,
                                                              i64 nseg, const i64* __restrict__ colptr, const unsigned* __restrict__ rowflag,
                                                              const double* __restrict__ val, const double* __restrict__ G,
                                                              const double* __restrict__ X, int k, double* __restrict__ segpart,
                                                              double* __restrict__ col_r, double* __restrict__ col_a, double* __restrict__ piecepart)
{
    __shared__ __attribute__((aligned(16))) double xs_all[16][KP];
    const i64 sg = (i64)blockIdx.x * 16 + threadIdx.x / 16;
    const int l = threadIdx.x % 16;
    double* xs = xs_all[threadIdx.x / 16];
    if (sg >= nseg) return;
    const unsigned piece = seg_piece[sg];
    i64 cs = seg_p0[sg];
    const i64 pend = cs + seg_len[sg];
    i64 j = seg_col[sg];
    double tr = 0.0, ta = 0.0;
    while (cs < pend) {
        i64 ce = pend;
        if (piece == MK_NO_PIECE) {
            while (colptr[j + 1] <= cs) ++j;
            ce = colptr[j + 1];
        }
#pragma unroll
        for (int c = 0; c < (KP + 15) / 16; ++c) {
            const int row = l + 16 * c;
            if (row < KP) { const double v = X[j * KP + (row < k ? row : 0)]; xs[row] = row < k ? v : 0.0; }
        }
        mk_lds_settle();
        i64 off[MK_E];
        bool act[MK_E];
        double a[MK_E], r[MK_E];
        mk_column_residual<KP>(rowflag, val, G, xs, k, cs, (int)(ce - cs), l, off, act, a, r);
        double sr = 0.0, sa = 0.0;
#pragma unroll
        for (int u = 0; u < MK_E; ++u) { sr = __builtin_fma(r[u], r[u], sr); sa = __builtin_fma(a[u], a[u], sa); }
        sr = group_sum<16>(sr);
        sa = group_sum<16>(sa);
        tr += sr;
        ta += sa;
        if (col_r && l == 0) {
            if (piece == MK_NO_PIECE) { col_r[j] = sr; col_a[j] = sa; }
            else { piecepart[2 * (i64)piece] = sr; piecepart[2 * (i64)piece + 1] = sa; }
        }
        mk_lds_settle();
        cs = ce;
        ++j;
    }
    if (l == 0) { segpart[2 * sg] = tr; segpart[2 * sg + 1] = ta; }
}

// the per-column sums of the long columns: their pieces in piece order
__global__ __launch_bounds__(256) void masked_residual_long_kernel(const unsigned* __restrict__ long_col, const i64* __restrict__ long_piece0,
                                                                   i64 nlong, const double* __restrict__ piecepart, double* __restrict__ col_r,
                                                                   double* __restrict__ col_a)
{
    const i64 c = (i64)blockIdx.x * blockDim.x + threadIdx.x;
    if (c >= nlong) return;
    double sr = 0.0, sa = 0.0;
    for (i64 q = long_piece0[c]; q < long_piece0[c + 1]; ++q) { sr += piecepart[2 * q]; sa += piecepart[2 * q + 1]; }
    col_r[long_col[c]] = sr;
    col_a[long_col[c]] = sa;
}

// the segments' sums in index order (thread t takes t, t + 1024, .., then a tree over the 1024 threads); out3[2] = |Omega|
__global__ __launch_bounds__(1024) void masked_residual_total_kernel(const double* __restrict__ segpart, i64 nseg, double count,
                                                                     double* __restrict__ out3, double* host_out)
{
    __shared__ double sh[1024][2];
    double r = 0.0, a = 0.0;
    for (i64 b = threadIdx.x; b < nseg; b += 1024) { r += segpart[2 * b]; a += segpart[2 * b + 1]; }
    sh[threadIdx.x][0] = r;
    sh[threadIdx.x][1] = a;
    __syncthreads();
    for (int w = 512; w > 0; w >>= 1) {
        if ((int)threadIdx.x < w) { sh[threadIdx.x][0] += sh[threadIdx.x + w][0]; sh[threadIdx.x][1] += sh[threadIdx.x + w][1]; }
        __syncthreads();
    }
    if (threadIdx.x == 0) {
        const double r3[3] = {sh[0][0], sh[0][1], count};
        for (int i = 0; i < 3; ++i) {
            out3[i] = r3[i];
            if (host_out) host_out[i] = r3[i];
        }
    }
}

static int mk_empty_blocks(const SegPlan& sp) { return sp.has_empty ? (int)std::min<i64>((sp.ncols + 255) / 256, 64) : 0; }
static int mk_sweep_blocks(const SegPlan& sp) { return (int)((sp.nseg + 15) / 16); }

int masked_sweep_partials(const SegPlan& sp) { return mk_sweep_blocks(sp) + (int)sp.nlong + mk_empty_blocks(sp); }

int launch_masked_sweep(const SegPlan& sp, const i64* colptr, const double* val, const double* G, double* X, int k, double l1, double l2,
                        double* res, double* viol_partials, hipStream_t st)
{
    if (k < 1 || k > 128) { set_error("launch_masked_sweep: k in [1, 128]"); return -3; }
    if (sp.nlong > 0 && !res) { set_error("launch_masked_sweep: the plan has long columns and no buffer for their residuals"); return -3; }
    const int KPv = kp_of(k);
    const int nb = mk_sweep_blocks(sp), ne = mk_empty_blocks(sp);
    if (nb > 0) {
        KP_DISPATCH128(KPv, (masked_sweep_kernel<KP><<<nb, 256, 0, st>>>(sp.seg_p0, sp.seg_len, sp.seg_col, sp.seg_piece, sp.nseg, colptr, sp.rowflag,
                                                                         val, G, X, k, l1, l2, viol_partials)));
        SMK_HIP(hipGetLastError());
    }
    if (sp.nlong > 0) {
        KP_DISPATCH128(KPv, (masked_long_kernel<KP><<<(unsigned)sp.nlong, 256, 0, st>>>(sp.long_col, colptr, sp.rowflag, val, G, X, k, l1, l2, res,
                                                                                        viol_partials + nb)));
        SMK_HIP(hipGetLastError());
    }
    if (ne > 0) {
        masked_empty_kernel<<<ne, 256, 0, st>>>(colptr, sp.ncols, X, KPv, k, l1, l2, viol_partials + nb + sp.nlong);
        SMK_HIP(hipGetLastError());
    }
    return 0;
}

size_t masked_residual_scratch_elems(const SegPlan& sp) { return (size_t)2 * (size_t)(sp.nseg + sp.npieces + 1); }

int launch_masked_residual(const SegPlan& sp, const i64* colptr, const double* val, const double* G, const double* X, int k, double* scratch,
                           double* col_r, double* col_a, double* out3, double* host_out, hipStream_t st)
{
    if (k < 1 || k > 128) { set_error("launch_masked_residual: k in [1, 128]"); return -3; }
    if ((col_r == nullptr) != (col_a == nullptr)) { set_error("launch_masked_residual: both per-column outputs or neither"); return -3; }
    const int KPv = kp_of(k);
    double* segpart = scratch;
    double* piecepart = scratch + 2 * sp.nseg;
    if (col_r && sp.has_empty) {
        SMK_HIP(hipMemsetAsync(col_r, 0, (size_t)sp.ncols * sizeof(double), st));
        SMK_HIP(hipMemsetAsync(col_a, 0, (size_t)sp.ncols * sizeof(double), st));
    }
    if (sp.nseg > 0) {
        const unsigned grid = (unsigned)mk_sweep_blocks(sp);
        KP_DISPATCH128(KPv, (masked_residual_kernel<KP><<<grid, 256, 0, st>>>(sp.seg_p0, sp.seg_len, sp.seg_col, sp.seg_piece, sp.nseg, colptr,
                                                                              sp.rowflag, val, G, X, k, segpart, col_r, col_a, piecepart)));
        SMK_HIP(hipGetLastError());
        if (col_r && sp.nlong > 0) {
            masked_residual_long_kernel<<<(unsigned)((sp.nlong + 255) / 256), 256, 0, st>>>(sp.long_col, sp.long_piece0, sp.nlong, piecepart, col_r, col_a);
            SMK_HIP(hipGetLastError());
        }
    }
    masked_residual_total_kernel<<<1, 1024, 0, st>>>(segpart, sp.nseg, (double)sp.nnz, out3, host_out);
    SMK_HIP(hipGetLastError());
    return 0;
}

}  // namespace smk
