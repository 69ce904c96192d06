// smallk_amd/csrc/kl.hip -- the kernels of KL-divergence NMF on a sparse matrix (kl.cpp): scikit-learn's multiplicative
// update for beta_loss = 1.  Both half-iterations are one sweep over the stored entries of one CSC -- CSC(A) for the H step, CSC(A')
// for the W step; below, "column" is a column of that CSC, X (KP x ncols) the factor being updated and G (KP x nrows) the factor
// whose rows the entries name.  Per stored entry (i, j, a):
//     d = g_i . x_j,   q = a / max(d, EPS),   num_j += q g_i
// and per column   x_j[t] *= num_j[t] / den[t],   den[t] = base[t] (+ l1 if > 0) (+ l2 x_j[t] if > 0), 0 -> EPS, base[t] = sum_i G[t, i].
// g_i is gathered ONCE: the registers that took part in the dot product are scaled by the quotient and accumulated.
//
// Work is cut as in spmm_seg.hip: a lane group owns one segment of the SegPlan (<= spmm_seg_len() consecutive entries: whole
// columns, or one piece of a longer column), the last entry of a column carries bit 31 of its row index, columns without entries
// are skipped through colptr, a piece leaves its partial numerator in `pieces` and kl_fixup_kernel joins the pieces of a column
// in a fixed order and applies the update.  The group is SIXTEEN lanes that split the rank (lane l: rows l, l + 16, ...; KU of
// them), as in residual_sddmm_kernel, not the KP / 2 lanes of the gather: the quotient needs the complete dot product in every
// lane before anything can be accumulated, which the xor butterfly delivers in four steps at every KP (a DPP row sum would need a
// broadcast behind it, and at KP = 8 / 16 its groups of 4 / 8 lanes leave a lane 2 values against 1 here: less gathers in flight).
// Every sum has a fixed order (storage order inside a column, piece order across pieces, lane order in the butterfly): the same
// bits on every run, no floating-point atomics.  Rows >= k of both factors are selected to zero on the way in, whatever they
// hold, and X's are written as zeros.
#include <algorithm>

#include "common.h"
#include "devutil.h"
#include "kl_dev.h"

namespace smk {

static constexpr unsigned KL_LAST = 0x80000000u;
static constexpr unsigned KL_NO_PIECE = 0xFFFFFFFFu;
// (KL_EPS, KL_EPS64 and kl_update, the multiplicative update of one entry: kl_dev.h, shared with kl_dense.hip)

__device__ __forceinline__ double kl_group_total(double v)
{
    v += __shfl_xor(v, 8, 64);
    v += __shfl_xor(v, 4, 64);
    v += __shfl_xor(v, 2, 64);
    v += __shfl_xor(v, 1, 64);
    return v;
}

// DIV = false: the quotient gather with the update as its epilogue.  DIV = true: the same traversal without the accumulate; per
// segment sum a log(a / max(d, EPS)) and sum a over its entries with a > EPS, to divpart[2 sg], divpart[2 sg + 1]; X is only read.
template <int KU, bool DIV>
__global__ __launch_bounds__(256) void kl_quotient_gather_kernel(const i64* __restrict__ seg_p0, const unsigned* __restrict__ seg_len,
                                                                 const unsigned* __restrict__ seg_col, const unsigned* __restrict__ seg_piece,
                                                                 i64 nseg, const i64* __restrict__ colptr, const unsigned* __restrict__ rowflag,
                                                                 const double* __restrict__ val, const double* __restrict__ G, double* X,
                                                                 int KP, int k, const double* __restrict__ base, int unit, double l1, double l2,
                                                                 int flush, double* __restrict__ pieces, double* __restrict__ divpart)
{
    constexpr int U = 4;
    const i64 sg = (i64)blockIdx.x * 16 + threadIdx.x / 16;
    const int l = threadIdx.x % 16;
    if (sg >= nseg) return;
    const i64 p0 = seg_p0[sg];
    const unsigned len = seg_len[sg];
    i64 j = seg_col[sg];
    const unsigned piece = seg_piece[sg];
    const unsigned* __restrict__ rf = rowflag + p0;
    const double* __restrict__ vv = val + p0;
    int idx[KU];           // the rows of this lane, clamped into [0, k) for the loads
    bool live[KU];
#pragma unroll
    for (int c = 0; c < KU; ++c) { live[c] = l + 16 * c < k; idx[c] = live[c] ? l + 16 * c : k - 1; }
    double h[KU], acc[KU];
    auto load_col = [&](i64 col) {
#pragma unroll
        for (int c = 0; c < KU; ++c) { const double v = X[col * KP + idx[c]]; h[c] = live[c] ? v : 0.0; }
    };
    load_col(j);
#pragma unroll
    for (int c = 0; c < KU; ++c) acc[c] = 0.0;
    double t = 0.0, s = 0.0;
    for (unsigned e = 0; e < len; e += U) {
        unsigned ri[U];
        double v[U], w[U][KU];
#pragma unroll
        for (int u = 0; u < U; ++u) {
            const unsigned q = e + u < len ? e + u : len - 1;
            ri[u] = rf[q];
            v[u] = vv[q];
        }
#pragma unroll
        for (int u = 0; u < U; ++u)
#pragma unroll
            for (int c = 0; c < KU; ++c) { const double g = G[(i64)(ri[u] & ~KL_LAST) * KP + idx[c]]; w[u][c] = live[c] ? g : 0.0; }
        // (the gathers do not depend on the column; each dot product below is taken against the h of the entry's own column)
#pragma unroll
        for (int u = 0; u < U; ++u) {
            if (e + u < len) {
                double d = 0.0;
#pragma unroll
                for (int c = 0; c < KU; ++c) d = __builtin_fma(w[u][c], h[c], d);
                d = kl_group_total(d);
                const double dd = d < KL_EPS ? KL_EPS : d;
                if constexpr (DIV) {
                    if (v[u] > KL_EPS) { t = __builtin_fma(v[u], log(v[u] / dd), t); s += v[u]; }
                } else {
                    const double q = v[u] / dd;
#pragma unroll
                    for (int c = 0; c < KU; ++c) acc[c] = __builtin_fma(q, w[u][c], acc[c]);
                }
                if ((ri[u] & KL_LAST) && piece == KL_NO_PIECE) {
                    if constexpr (!DIV) {
#pragma unroll
                        for (int c = 0; c < KU; ++c) {
                            if (l + 16 * c < KP) X[j * KP + l + 16 * c] = live[c] ? kl_update(h[c], acc[c], base[idx[c]], unit, l1, l2, flush) : 0.0;
                            acc[c] = 0.0;
                        }
                    }
                    ++j;
                    if (e + u + 1 < len) {
                        const i64 nxt = p0 + e + u + 1;
                        while (colptr[j + 1] <= nxt) ++j;          // columns without stored entries
                        load_col(j);
                    }
                }
            }
        }
    }
    if constexpr (DIV) {
        if (l == 0) { divpart[2 * sg] = t; divpart[2 * sg + 1] = s; }
    } else if (piece != KL_NO_PIECE) {
#pragma unroll
        for (int c = 0; c < KU; ++c)
            if (l + 16 * c < KP) pieces[(i64)piece * KP + l + 16 * c] = acc[c];
    }
}

// columns longer than a segment: a wave per column.  Its four groups of sixteen lanes take every fourth piece each, in piece order
// and with four loads in flight (the longest row of the Reuters shape is 125 pieces: with one group per column the W side cost
// 0.067 ms there, 0.051 ms this way), then the four sums are joined by two butterfly steps -- (g0 + g1) + (g2 + g3), a fixed order --
// and the update is applied
__global__ __launch_bounds__(256) void kl_fixup_kernel(const unsigned* __restrict__ long_col, const i64* __restrict__ long_piece0, i64 nlong,
                                                       const double* __restrict__ pieces, double* __restrict__ X, int KP, int k,
                                                       const double* __restrict__ base, int unit, double l1, double l2, int flush)
{
    const i64 c = (i64)blockIdx.x * 4 + (threadIdx.x >> 6);
    const int lane = threadIdx.x & 63, g = lane / 16, l = lane % 16;
    if (c >= nlong) return;
    const i64 q0 = long_piece0[c], q1 = long_piece0[c + 1];
    const i64 col = long_col[c];
    for (int r = l; r < KP; r += 16) {
        double num = 0.0;
        for (i64 q = q0 + g; q < q1; q += 16) {
            double p[4];
#pragma unroll
            for (int u = 0; u < 4; ++u) p[u] = pieces[(q + 4 * u < q1 ? q + 4 * u : q1 - 1) * KP + r];
#pragma unroll
            for (int u = 0; u < 4; ++u) if (q + 4 * u < q1) num += p[u];
        }
        num += __shfl_xor(num, 16, 64);
        num += __shfl_xor(num, 32, 64);
        if (g == 0) X[col * KP + r] = r < k ? kl_update(X[col * KP + r], num, base[r], unit, l1, l2, flush) : 0.0;
    }
}

// columns without stored entries: their numerator is zero, and so are they after the update
__global__ __launch_bounds__(256) void kl_zero_empty_kernel(const i64* __restrict__ colptr, i64 ncols, double* __restrict__ X, int KP)
{
    const i64 stride = (i64)gridDim.x * blockDim.x;
    for (i64 i = (i64)blockIdx.x * blockDim.x + threadIdx.x; i < ncols * KP; i += stride) {
        const i64 j = i / KP;
        if (colptr[j + 1] == colptr[j]) X[i] = 0.0;
    }
}

// the row sums of a factor (KP x N): workgroup b takes the columns [b cpb, (b + 1) cpb), thread (g, r) every (256 / KP)-th of them
// for row r, then the sub-sums are added in g order; part[b][r].  kl_sums_finish_kernel adds the workgroups' in b order.
__global__ __launch_bounds__(256) void kl_factor_sums_kernel(const double* __restrict__ X, int KP, int k, i64 N, i64 cpb, double* __restrict__ part)
{
    __shared__ double sh[256];
    const int r = threadIdx.x % KP, g = threadIdx.x / KP, ng = 256 / KP;
    const i64 c0 = (i64)blockIdx.x * cpb, c1 = c0 + cpb < N ? c0 + cpb : N;
    double v = 0.0;
    if (r < k)
        for (i64 j = c0 + g; j < c1; j += ng) v += X[j * KP + r];
    sh[threadIdx.x] = v;
    __syncthreads();
    if (g == 0) {
        double tot = 0.0;
        for (int gg = 0; gg < ng; ++gg) tot += sh[gg * KP + r];
        part[(i64)blockIdx.x * KP + r] = tot;
    }
}

__global__ __launch_bounds__(128) void kl_sums_finish_kernel(const double* __restrict__ part, int nblk, int KP, double* __restrict__ out)
{
    const int r = threadIdx.x;
    if (r >= KP) return;
    double tot = 0.0;
    for (int b = 0; b < nblk; ++b) tot += part[(i64)b * KP + r];
    out[r] = tot;
}

// the segments' sums in index order (thread t takes t, t + 1024, ..., then a tree over the 1024 threads), sum WH from the row sums:
// out[0] = D = sum a log(a / d) + (sum WH - sum a), out[1] = sum a log(a / d), out[2] = sum WH, out[3] = sum a; host_out: pinned or null
__global__ __launch_bounds__(1024) void kl_divergence_total_kernel(const double* __restrict__ divpart, i64 nseg, const double* __restrict__ sums_a,
                                                                   const double* __restrict__ sums_b, int k, double* __restrict__ out,
                                                                   double* host_out)
{
    __shared__ double sh[1024][2];
    double t = 0.0, s = 0.0;
    for (i64 b = threadIdx.x; b < nseg; b += 1024) { t += divpart[2 * b]; s += divpart[2 * b + 1]; }
    sh[threadIdx.x][0] = t;
    sh[threadIdx.x][1] = s;
    __syncthreads();
    for (int w = 512; w > 0; w >>= 1) {
        if ((int)threadIdx.x < w) { sh[threadIdx.x][0] += sh[threadIdx.x + w][0]; sh[threadIdx.x][1] += sh[threadIdx.x + w][1]; }
        __syncthreads();
    }
    if (threadIdx.x == 0) {
        double swh = 0.0;
        for (int r = 0; r < k; ++r) swh = __builtin_fma(sums_a[r], sums_b[r], swh);
        const double r4[4] = {sh[0][0] + (swh - sh[0][1]), sh[0][0], swh, sh[0][1]};
        for (int i = 0; i < 4; ++i) {
            out[i] = r4[i];
            if (host_out) host_out[i] = r4[i];
        }
    }
}

static int kl_ku(int KPv) { return KPv <= 16 ? 1 : KPv / 16; }

#define SMK_KL_GATHER(KU, DIV, ...) kl_quotient_gather_kernel<KU, DIV><<<grid, 256, 0, st>>>(__VA_ARGS__)
#define SMK_KL_DISPATCH(DIV, ...)                                  \
    switch (kl_ku(KPv)) {                                          \
        case 1: SMK_KL_GATHER(1, DIV, __VA_ARGS__); break;         \
        case 2: SMK_KL_GATHER(2, DIV, __VA_ARGS__); break;         \
        case 4: SMK_KL_GATHER(4, DIV, __VA_ARGS__); break;         \
        default: SMK_KL_GATHER(8, DIV, __VA_ARGS__); break;        \
    }

int launch_kl_step(const SegPlan& sp, const i64* colptr, const double* val, const double* G, double* X, int k, const double* base, int unit,
                   double l1, double l2, int flush, double* pieces, hipStream_t st)
{
    if (k < 1 || k > 128) { set_error("launch_kl_step: k in [1, 128]"); return -3; }
    if (sp.npieces > 0 && !pieces) { set_error("launch_kl_step: the plan has pieces and no buffer for them"); return -3; }
    const int KPv = kp_of(k);
    if (sp.ncols <= 0) return 0;
    if (sp.has_empty) {
        const i64 tot = sp.ncols * KPv;
        kl_zero_empty_kernel<<<(unsigned)std::min<i64>((tot + 255) / 256, 4096), 256, 0, st>>>(colptr, sp.ncols, X, KPv);
        SMK_HIP(hipGetLastError());
    }
    if (sp.nseg == 0) return 0;
    const unsigned grid = (unsigned)((sp.nseg + 15) / 16);
    SMK_KL_DISPATCH(false, sp.seg_p0, sp.seg_len, sp.seg_col, sp.seg_piece, sp.nseg, colptr, sp.rowflag, val, G, X, KPv, k, base, unit, l1, l2,
                    flush, pieces, nullptr);
    SMK_HIP(hipGetLastError());
    if (sp.nlong > 0) {
        kl_fixup_kernel<<<(unsigned)((sp.nlong + 3) / 4), 256, 0, st>>>(sp.long_col, sp.long_piece0, sp.nlong, pieces, X, KPv, k, base, unit, l1,
                                                                          l2, flush);
        SMK_HIP(hipGetLastError());
    }
    return 0;
}

int launch_kl_divergence(const SegPlan& sp, const i64* colptr, const double* val, const double* G, const double* X, int k, const double* sums_g,
                         const double* sums_x, double* divpart, double* out4, double* host_out, hipStream_t st)
{
    if (k < 1 || k > 128) { set_error("launch_kl_divergence: k in [1, 128]"); return -3; }
    const int KPv = kp_of(k);
    if (sp.nseg > 0) {
        const unsigned grid = (unsigned)((sp.nseg + 15) / 16);
        SMK_KL_DISPATCH(true, sp.seg_p0, sp.seg_len, sp.seg_col, sp.seg_piece, sp.nseg, colptr, sp.rowflag, val, G, const_cast<double*>(X), KPv, k,
                        nullptr, 0, 0.0, 0.0, 0, nullptr, divpart);
        SMK_HIP(hipGetLastError());
    }
    kl_divergence_total_kernel<<<1, 1024, 0, st>>>(divpart, sp.nseg, sums_g, sums_x, k, out4, host_out);
    SMK_HIP(hipGetLastError());
    return 0;
}
#undef SMK_KL_DISPATCH
#undef SMK_KL_GATHER

int kl_sums_blocks(i64 N) { return (int)std::min<i64>((N + 255) / 256, 1024); }

int launch_kl_factor_sums(const double* X, int k, i64 N, double* part, double* out, hipStream_t st)
{
    if (k < 1 || k > 128 || N < 1) { set_error("launch_kl_factor_sums: k in [1, 128] and N >= 1"); return -3; }
    const int KPv = kp_of(k), nblk = kl_sums_blocks(N);
    const i64 cpb = (N + nblk - 1) / nblk;
    kl_factor_sums_kernel<<<nblk, 256, 0, st>>>(X, KPv, k, N, cpb, part);
    SMK_HIP(hipGetLastError());
    kl_sums_finish_kernel<<<1, 128, 0, st>>>(part, nblk, KPv, out);
    SMK_HIP(hipGetLastError());
    return 0;
}

}  // namespace smk
