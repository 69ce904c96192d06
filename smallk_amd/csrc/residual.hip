// smallk_amd/csrc/residual.hip -- the reconstruction error ||A - W H||_F^2 and ||A||_F^2 of a resident matrix, per column and
// in total.  fp64 throughout against the STORED values of A (exact in fp64): the result differs from a host
// fp64 computation by summation order only, and it is the same bits on every run (no floating-point atomics; every sum has
// a fixed order).
//
// Dense: one streaming read of A.  A workgroup owns a 64-column tile and a SPAN of 64-row tiles; per tile it forms (W H)_tile
// on the fp64 matrix cores (v_mfma_f64_16x16x4_f64, contraction over the rank -- an outer-product GEMM whose m x n result is
// never stored), subtracts it from the widened stored entries, squares and adds per column.  One partial per (span, column).
// Sparse: sum_e a_e^2 - 2 sum_e a_e (w_i(e) . h_j(e)) + sum_j h_j' (W'W) h_j over the stored entries e: a sampled dense-dense
// product on the entry-balanced segments of the matrix (common.h: SegPlan) and a k x k quadratic form per column.
#include "common.h"
#include "devutil.h"

namespace smk {

static constexpr int RES_T = 64;              // rows and columns of a tile, factor rows per group
static constexpr int RES_FP = 65;             // doubles per factor row of a slab in LDS (odd: the transposing stores are conflict free)
static constexpr int RES_AP = 68;             // floats per column of the A tile in LDS (4 l15 + l4 covers 64 banks)
static constexpr unsigned RES_LAST = 0x80000000u, RES_NO_PIECE = 0xFFFFFFFFu;     // as in spmm_seg.hip

// D of v_mfma_f64_16x16x4_f64: column = lane & 15, row = (lane >> 4) + 4 reg (NOT the map of the other matrix instructions).
// Here the A operand is W (D rows = rows of A), the B operand is H (D columns = columns of A): every result of a lane lies in
// ONE column of A, so a lane keeps one running sum of squares per output and the tile never leaves the registers.
// NQ: contraction steps of 4 factor rows per group (1, 2, 4, 8, 16), a template parameter so that the step loop unrolls and the LDS
// reads of later steps are in flight under the matrix instructions of earlier ones (with a run-time bound every step waited for
// its own five reads: 12.9 TFLOP/s at C3's shape); the slabs hold kr = 4 NQ rows, those from k on as zeros.
template <int EBYTES, int NQ>
__global__ __launch_bounds__(256) void residual_dense_kernel(const unsigned char* __restrict__ A, i64 lda_bytes, i64 m, i64 n,
                                                             const double* __restrict__ Wt, const double* __restrict__ H, int ldf,
                                                             int k, i64 row_tiles, i64 tiles_per_span, int S, i64 ncols_pad,
                                                             double* __restrict__ part_r, double* __restrict__ part_a)
{
    constexpr int kr = 4 * NQ;
    extern __shared__ __attribute__((aligned(16))) unsigned char res_lds[];
    double* Ws = (double*)res_lds;                        // [kr][RES_FP]: W of the tile's rows, one group of factor rows
    double* Hs = Ws + kr * RES_FP;                        // [kr][RES_FP]: H of the tile's columns
    float* As = (float*)(Hs + kr * RES_FP);               // [64 columns][RES_AP]
    const i64 bid = blockIdx.x;                           // 1-D grid, 64-bit tile arithmetic
    const i64 ct = bid / S;
    const int sp = (int)(bid % S);
    const i64 rt0 = (i64)sp * tiles_per_span;
    i64 rt1 = rt0 + tiles_per_span;
    if (rt1 > row_tiles) rt1 = row_tiles;
    const i64 c0 = ct * RES_T;
    // the wave index as a scalar: every global address below is then a scalar base (tile, column / row of the wave's trip) plus ONE
    // per-lane offset, instead of sixteen 64-bit addresses per operand held in vector registers across the tile loop
    const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6), l15 = lane & 15, l4 = lane >> 4;
    const int ng = (k + RES_T - 1) / RES_T;
    typedef __attribute__((ext_vector_type(4))) double f64x4;
    f64x4 acc[4];
    double racc = 0.0, aacc = 0.0;
    // the A tile and the first group of W rows of tile rt + 1 are loaded into registers while the matrix cores work on tile rt.
    // Everything outside the matrix (rows >= m, columns >= n) and factor rows >= k are read as zero HERE: neither the padding
    // of A nor the pad rows of a factor buffer are relied on.  Trip i of a wave: column / row 4 i + wave, the lane = the row of A /
    // the factor row.
    // Every load is UNCONDITIONAL at a clamped address (last row / column / factor row of the matrix) and its value masked
    // afterwards: a load under a branch is followed by a wait for it before the branch closes, which serialised the 32 loads of a
    // tile (one memory latency each: 5.2 ms at C3's shape, 13 TFLOP/s, whatever the rank).
    float bv[16];
    double wv[16];
    const int kc = lane < k ? lane : k - 1;               // this lane's factor row, clamped
    auto fetch = [&](i64 rt) {
        const i64 r0 = rt * RES_T;
        const bool row_in = r0 + lane < m;
        const i64 rl = row_in ? r0 + lane : m - 1;
#pragma unroll
        for (int i = 0; i < 16; ++i) {
            const i64 c = c0 + 4 * i + wave;
            const unsigned char* col = A + (c < n ? c : n - 1) * lda_bytes;      // scalar
            float v;
            if constexpr (EBYTES == 2) v = bf16_bits_to_f32(__builtin_nontemporal_load((const unsigned short*)col + rl));
            else v = __builtin_nontemporal_load((const float*)col + rl);
            bv[i] = (row_in && c < n) ? v : 0.f;
        }
#pragma unroll
        for (int i = 0; i < 16; ++i) {
            const i64 r = r0 + 4 * i + wave;
            const double* row = Wt + (r < m ? r : m - 1) * ldf;                  // scalar
            wv[i] = row[kc];                    // masked when it is stored to LDS (below): a select here would be turned back into a branch around the load
        }
    };
    // keeps the sixteen loads above it in flight together: the values become opaque here, so no load can sink into the branch
    // that masks it
    auto pin = [&](double (&t)[16]) {
#pragma unroll
        for (int i = 0; i < 16; ++i) asm volatile("" : "+v"(t[i]));
    };
    // a later group of W rows / a group of H columns: global (L2) -> registers -> LDS
    auto load_w = [&](i64 rt, int k0) {
        const i64 r0 = rt * RES_T;
        const int kcg = k0 + lane < k ? k0 + lane : k - 1;
        double t[16];
#pragma unroll
        for (int i = 0; i < 16; ++i) {
            const i64 r = r0 + 4 * i + wave;
            t[i] = Wt[(r < m ? r : m - 1) * ldf + kcg];
        }
        pin(t);
        if (lane < kr) {
#pragma unroll
            for (int i = 0; i < 16; ++i) Ws[lane * RES_FP + 4 * i + wave] = (r0 + 4 * i + wave < m && k0 + lane < k) ? t[i] : 0.0;
        }
    };
    auto load_h = [&](int k0) {
        const int kcg = k0 + lane < k ? k0 + lane : k - 1;
        double t[16];
#pragma unroll
        for (int i = 0; i < 16; ++i) {
            const i64 c = c0 + 4 * i + wave;
            t[i] = H[(c < n ? c : n - 1) * ldf + kcg];
        }
        pin(t);
        if (lane < kr) {
#pragma unroll
            for (int i = 0; i < 16; ++i) Hs[lane * RES_FP + 4 * i + wave] = (c0 + 4 * i + wave < n && k0 + lane < k) ? t[i] : 0.0;
        }
    };
    auto mfma_group = [&]() {
#pragma unroll
        for (int q = 0; q < NQ; ++q) {
            const double b = Hs[(4 * q + l4) * RES_FP + 16 * wave + l15];
#pragma unroll
            for (int t = 0; t < 4; ++t) acc[t] = __builtin_amdgcn_mfma_f64_16x16x4f64(Ws[(4 * q + l4) * RES_FP + 16 * t + l15], b, acc[t], 0, 0, 0);
        }
    };
    if (rt0 < rt1) fetch(rt0);
    if (ng == 1) load_h(0);                    // one group: the tile's columns of H stay in LDS for the whole span
    for (i64 rt = rt0; rt < rt1; ++rt) {
#pragma unroll
        for (int t = 0; t < 4; ++t) acc[t] = f64x4{0.0, 0.0, 0.0, 0.0};
#pragma unroll
        for (int i = 0; i < 16; ++i) {
            As[(4 * i + wave) * RES_AP + lane] = bv[i];
            if (lane < kr) Ws[lane * RES_FP + 4 * i + wave] = (rt * RES_T + 4 * i + wave < m && lane < k) ? wv[i] : 0.0;
        }
        if (ng > 1) load_h(0);
        __syncthreads();
        if (rt + 1 < rt1) fetch(rt + 1);
        mfma_group();
        for (int g = 1; g < ng; ++g) {         // k > 64: the tile keeps its accumulators across the groups, A is still read once
            __syncthreads();
            load_w(rt, g * RES_T);
            load_h(g * RES_T);
            __syncthreads();
            mfma_group();
        }
#pragma unroll
        for (int t = 0; t < 4; ++t)
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const double av = (double)As[(16 * wave + l15) * RES_AP + 16 * t + l4 + 4 * r];
                const double d = av - acc[t][r];
                racc = __builtin_fma(d, d, racc);
                aacc = __builtin_fma(av, av, aacc);
            }
        __syncthreads();
    }
    // the four lanes of a column, fixed order; one partial per (span, column)
    racc += __shfl_xor(racc, 16, 64);
    racc += __shfl_xor(racc, 32, 64);
    aacc += __shfl_xor(aacc, 16, 64);
    aacc += __shfl_xor(aacc, 32, 64);
    if (l4 == 0) {
        part_r[(i64)sp * ncols_pad + c0 + 16 * wave + l15] = racc;
        part_a[(i64)sp * ncols_pad + c0 + 16 * wave + l15] = aacc;
    }
}

// sum of the `cnt` pairs a workgroup holds in LDS, in index order, by thread 0
__device__ __forceinline__ void residual_block_partial(const double (*sh)[2], int cnt, double* __restrict__ blockpart, i64 slot)
{
    if (threadIdx.x == 0) {
        double r = 0.0, a = 0.0;
        for (int i = 0; i < cnt; ++i) { r += sh[i][0]; a += sh[i][1]; }
        blockpart[2 * slot] = r;
        blockpart[2 * slot + 1] = a;
    }
}

// dense: the spans of a column in span order; 256 columns per workgroup, whose sums go to blockpart in column order
__global__ __launch_bounds__(256) void residual_colsum_kernel(const double* __restrict__ part_r, const double* __restrict__ part_a,
                                                              int S, i64 ncols_pad, i64 n, double* __restrict__ col_r,
                                                              double* __restrict__ col_a, double* __restrict__ blockpart)
{
    __shared__ double sh[256][2];
    const i64 j = (i64)blockIdx.x * 256 + threadIdx.x;
    double r = 0.0, a = 0.0;
    if (j < n) {
        for (int s = 0; s < S; ++s) { r += part_r[(i64)s * ncols_pad + j]; a += part_a[(i64)s * ncols_pad + j]; }
        col_r[j] = r;
        col_a[j] = a;
    }
    sh[threadIdx.x][0] = r;
    sh[threadIdx.x][1] = a;
    __syncthreads();
    // 16 sums of 16, then their sum: the order is fixed, the chains are short
    double r2 = 0.0, a2 = 0.0;
    if (threadIdx.x < 16)
        for (int i = 0; i < 16; ++i) { r2 += sh[16 * threadIdx.x + i][0]; a2 += sh[16 * threadIdx.x + i][1]; }
    __syncthreads();
    if (threadIdx.x < 16) { sh[threadIdx.x][0] = r2; sh[threadIdx.x][1] = a2; }
    __syncthreads();
    residual_block_partial(sh, 16, blockpart, blockIdx.x);
}

// the per-workgroup sums in index order: thread t takes entries t, t + 1024, ..., then the 1024 threads are joined by a tree
__global__ __launch_bounds__(1024) void residual_total_kernel(const double* __restrict__ blockpart, i64 nblk, double* __restrict__ out2)
{
    __shared__ double sh[1024][2];
    double r = 0.0, a = 0.0;
    for (i64 b = threadIdx.x; b < nblk; b += 1024) { r += blockpart[2 * b]; a += blockpart[2 * b + 1]; }
    sh[threadIdx.x][0] = r;
    sh[threadIdx.x][1] = a;
    __syncthreads();
    for (int w = 512; w > 0; w >>= 1) {
        if ((int)threadIdx.x < w) { sh[threadIdx.x][0] += sh[threadIdx.x + w][0]; sh[threadIdx.x][1] += sh[threadIdx.x + w][1]; }
        __syncthreads();
    }
    if (threadIdx.x == 0) { out2[0] = sh[0][0] < 0.0 ? 0.0 : sh[0][0]; out2[1] = sh[0][1]; }
}

// ---- sparse ------------------------------------------------------------------------------------------------------------
// The sampled product: for every stored entry (i, j, a) the dot product of row i of W (contiguous in Wt) with column j of H,
// summed per column as t_j = sum a p and s_j = sum a^2.  Sixteen lanes own a segment (<= spmm_seg_len() consecutive entries:
// whole columns, or one piece of a long column) and split the rank: lane l takes factor rows l, l + 16, ...  (KU of them, held
// in registers for H; KU = 0: any rank, H re-read through the caches).  Four gathers in flight per lane.
template <int KU>
__global__ __launch_bounds__(256) void residual_sddmm_kernel(const i64* __restrict__ seg_p0, const unsigned* __restrict__ seg_len,
                                                             const unsigned* __restrict__ seg_col, const unsigned* __restrict__ seg_piece,
                                                             i64 nseg, const i64* __restrict__ colptr, const unsigned* __restrict__ rowflag,
                                                             const double* __restrict__ val, const double* __restrict__ Wt,
                                                             const double* __restrict__ H, int ldf, int k, double* __restrict__ col_t,
                                                             double* __restrict__ col_s, double* __restrict__ pieces)
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
    double h[KU > 0 ? KU : 1];
    auto load_col = [&](i64 col) {
#pragma unroll
        for (int c = 0; c < KU; ++c) { const double v = H[col * ldf + (l + 16 * c < k ? l + 16 * c : k - 1)]; h[c] = (l + 16 * c < k) ? v : 0.0; }
    };
    load_col(j);
    auto group_total = [&](double v) {
        v += __shfl_xor(v, 8, 64);
        v += __shfl_xor(v, 4, 64);
        v += __shfl_xor(v, 2, 64);
        v += __shfl_xor(v, 1, 64);
        return v;
    };
    double t = 0.0, s2 = 0.0;
    for (unsigned e = 0; e < len; e += U) {
        unsigned ri[U];
        double v[U];
#pragma unroll
        for (int u = 0; u < U; ++u) {
            const unsigned q = e + u < len ? e + u : len - 1;
            ri[u] = rf[q];
            v[u] = vv[q];
        }
        if constexpr (KU > 0) {
            double w[U][KU];
#pragma unroll
            for (int u = 0; u < U; ++u)
#pragma unroll
                for (int c = 0; c < KU; ++c) w[u][c] = Wt[(i64)(ri[u] & ~RES_LAST) * ldf + (l + 16 * c < k ? l + 16 * c : k - 1)];      // (h is zero from k on)
            // (the gathers do not depend on the column; each dot product below is taken against the h of the entry's own column)
#pragma unroll
            for (int u = 0; u < U; ++u) {
                if (e + u < len) {
                    double d = 0.0;
#pragma unroll
                    for (int c = 0; c < KU; ++c) d = __builtin_fma(w[u][c], h[c], d);
                    t = __builtin_fma(v[u], d, t);
                    s2 = __builtin_fma(v[u], v[u], s2);
                    if ((ri[u] & RES_LAST) && piece == RES_NO_PIECE) {
                        const double tt = group_total(t);
                        if (l == 0) { col_t[j] = tt; col_s[j] = s2; }
                        t = s2 = 0.0;
                        ++j;
                        if (e + u + 1 < len) {
                            const i64 nxt = p0 + e + u + 1;
                            while (colptr[j + 1] <= nxt) ++j;          // columns without stored entries
                            load_col(j);
                        }
                    }
                }
            }
        } else {
            for (int u = 0; u < U; ++u) {
                if (e + u < len) {
                    const double* wr = Wt + (i64)(ri[u] & ~RES_LAST) * ldf;
                    const double* hc = H + j * ldf;
                    double d0 = 0.0, d1 = 0.0;
                    int kk = l;
                    for (; kk + 16 < k; kk += 32) { d0 = __builtin_fma(wr[kk], hc[kk], d0); d1 = __builtin_fma(wr[kk + 16], hc[kk + 16], d1); }
                    if (kk < k) d0 = __builtin_fma(wr[kk], hc[kk], d0);
                    t = __builtin_fma(v[u], d0 + d1, t);
                    s2 = __builtin_fma(v[u], v[u], s2);
                    if ((ri[u] & RES_LAST) && piece == RES_NO_PIECE) {
                        const double tt = group_total(t);
                        if (l == 0) { col_t[j] = tt; col_s[j] = s2; }
                        t = s2 = 0.0;
                        ++j;
                        if (e + u + 1 < len) {
                            const i64 nxt = p0 + e + u + 1;
                            while (colptr[j + 1] <= nxt) ++j;
                        }
                    }
                }
            }
        }
    }
    if (piece != RES_NO_PIECE) {
        const double tt = group_total(t);
        if (l == 0) { pieces[2 * (i64)piece] = tt; pieces[2 * (i64)piece + 1] = s2; }
    }
}

// columns longer than a segment: their pieces in piece order, one thread per column
__global__ __launch_bounds__(256) void residual_fixup_kernel(const unsigned* __restrict__ long_col, const i64* __restrict__ long_piece0,
                                                             i64 nlong, const double* __restrict__ pieces, double* __restrict__ col_t,
                                                             double* __restrict__ col_s)
{
    const i64 c = (i64)blockIdx.x * 256 + threadIdx.x;
    if (c >= nlong) return;
    double t = 0.0, s = 0.0;
    for (i64 q = long_piece0[c]; q < long_piece0[c + 1]; ++q) { t += pieces[2 * q]; s += pieces[2 * q + 1]; }
    col_t[long_col[c]] = t;
    col_s[long_col[c]] = s;
}

// per column: q_j = h_j' G h_j with G = W'W (sixteen lanes per column, lane l the rows l, l + 16, ... of G h_j; G is symmetric,
// so row b of it serves as column b and the lanes read consecutive words), then r_j = max(0, s_j - 2 t_j + q_j) -- cancellation
// at a near-exact fit is expected -- and the workgroup's sums for the total.  G in LDS up to rank 64 (lds_g != 0).
__global__ __launch_bounds__(256) void residual_sparse_finish_kernel(const double* __restrict__ H, int ldf, int k,
                                                                    const double* __restrict__ G, int ldg, int lds_g, i64 n,
                                                                    const double* __restrict__ col_t, const double* __restrict__ col_s,
                                                                    const double* __restrict__ col_merged, double* __restrict__ col_r,
                                                                    double* __restrict__ col_a, double* __restrict__ blockpart)
{
    extern __shared__ __attribute__((aligned(16))) unsigned char res_lds[];
    double* Gs = (double*)res_lds;
    __shared__ double sh[16][2];
    if (lds_g) {
        for (int idx = threadIdx.x; idx < k * k; idx += 256) Gs[idx] = G[(i64)(idx / k) * ldg + idx % k];
        __syncthreads();
    }
    const int g = threadIdx.x / 16, l = threadIdx.x % 16;
    const i64 nbatch = (n + 15) / 16;
    for (i64 bb = blockIdx.x; bb < nbatch; bb += gridDim.x) {      // 16 columns per trip; the staged G serves every trip
        const i64 j = bb * 16 + g;
        double q = 0.0;
        if (j < n) {
            const double* hc = H + j * ldf;
            for (int a = l; a < k; a += 16) {
                double y = 0.0;
                if (lds_g) for (int b = 0; b < k; ++b) y = __builtin_fma(Gs[b * k + a], hc[b], y);
                else for (int b = 0; b < k; ++b) y = __builtin_fma(G[(i64)b * ldg + a], hc[b], y);
                q = __builtin_fma(hc[a], y, q);
            }
        }
        q += __shfl_xor(q, 8, 64);
        q += __shfl_xor(q, 4, 64);
        q += __shfl_xor(q, 2, 64);
        q += __shfl_xor(q, 1, 64);
        if (l == 0) {
            double r = 0.0, a2 = 0.0;
            if (j < n) {
                a2 = col_merged ? col_merged[j] : col_s[j];
                r = a2 - 2.0 * col_t[j] + q;
                if (r < 0.0) r = 0.0;
                col_r[j] = r;
                col_a[j] = a2;
            }
            sh[g][0] = r;
            sh[g][1] = a2;
        }
        __syncthreads();
        residual_block_partial(sh, 16, blockpart, bb);
        __syncthreads();
    }
}

// ---- launchers ---------------------------------------------------------------------------------------------------------
// spans of row tiles per column tile: enough workgroups for four per CU, never more than 32 (the partials are [S][n] doubles;
// one per row tile would be 2 GB at a 1 M x 1 M matrix's shape), every span non-empty.  (kl_dense.hip cuts its launches by the same rule.)
void residual_dense_shape(i64 m, i64 n, int num_cus, i64* row_tiles, i64* col_tiles, i64* tps, int* S)
{
    const i64 rt = (m + RES_T - 1) / RES_T, ctl = (n + RES_T - 1) / RES_T;
    i64 want = ((i64)4 * num_cus + ctl - 1) / ctl;
    if (want < 1) want = 1;
    if (want > 32) want = 32;
    if (want > rt) want = rt;
    const i64 per = (rt + want - 1) / want;
    *row_tiles = rt; *col_tiles = ctl; *tps = per; *S = (int)((rt + per - 1) / per);
}

size_t residual_dense_scratch_elems(i64 m, i64 n, int num_cus)
{
    i64 rt, ctl, per; int S;
    residual_dense_shape(m, n, num_cus, &rt, &ctl, &per, &S);
    return (size_t)2 * S * ctl * RES_T + (size_t)2 * ((n + 255) / 256);
}

template <int EBYTES, int NQ>
static int residual_dense_launch(unsigned grid, const unsigned char* A, i64 lda_bytes, i64 m, i64 n, const double* Wt, const double* H, int ldf,
                                 int k, i64 rt, i64 per, int S, i64 ncols_pad, double* part_r, double* part_a, hipStream_t st)
{
    constexpr int lds = 2 * 4 * NQ * RES_FP * (int)sizeof(double) + RES_T * RES_AP * (int)sizeof(float);
    if constexpr (lds > 64 * 1024) {
        static std::atomic<unsigned long long> attr_set{0};       // per device (DeviceOnce)
        if (DeviceOnce once{attr_set}) {
            SMK_HIP(hipFuncSetAttribute((const void*)residual_dense_kernel<EBYTES, NQ>, hipFuncAttributeMaxDynamicSharedMemorySize, lds));
            once.done();
        }
    }
    residual_dense_kernel<EBYTES, NQ><<<grid, 256, lds, st>>>(A, lda_bytes, m, n, Wt, H, ldf, k, rt, per, S, ncols_pad, part_r, part_a);
    return 0;
}

int launch_residual_dense(const void* A, int storage, i64 ldA, i64 m, i64 n, const double* Wt, const double* H, int ldf, int k,
                          double* scratch, double* col_r, double* col_a, double* out2, int num_cus, hipStream_t st)
{
    i64 rt, ctl, per; int S;
    residual_dense_shape(m, n, num_cus, &rt, &ctl, &per, &S);
    const i64 ncols_pad = ctl * RES_T;
    if (ctl * S > 0x7FFFFFFFll) { set_error("residual: matrix too wide for one launch"); return -100; }
    double* part_r = scratch;
    double* part_a = part_r + (size_t)S * ncols_pad;
    double* blockpart = part_a + (size_t)S * ncols_pad;
    const int nq = k > 32 ? 16 : k > 16 ? 8 : k > 8 ? 4 : k > 4 ? 2 : 1;
    const unsigned grid = (unsigned)(ctl * S);
    int rc = 0;
#define SMK_RES(EB, NQ) rc = residual_dense_launch<EB, NQ>(grid, (const unsigned char*)A, ldA * EB, m, n, Wt, H, ldf, k, rt, per, S, ncols_pad, part_r, part_a, st)
    if (storage == STORE_BF16) {
        switch (nq) { case 1: SMK_RES(2, 1); break; case 2: SMK_RES(2, 2); break; case 4: SMK_RES(2, 4); break; case 8: SMK_RES(2, 8); break; default: SMK_RES(2, 16); break; }
    } else {
        switch (nq) { case 1: SMK_RES(4, 1); break; case 2: SMK_RES(4, 2); break; case 4: SMK_RES(4, 4); break; case 8: SMK_RES(4, 8); break; default: SMK_RES(4, 16); break; }
    }
#undef SMK_RES
    if (rc) return rc;
    SMK_HIP(hipGetLastError());
    const i64 nblk = (n + 255) / 256;
    residual_colsum_kernel<<<(unsigned)nblk, 256, 0, st>>>(part_r, part_a, S, ncols_pad, n, col_r, col_a, blockpart);
    SMK_HIP(hipGetLastError());
    residual_total_kernel<<<1, 1024, 0, st>>>(blockpart, nblk, out2);
    SMK_HIP(hipGetLastError());
    return 0;
}

size_t residual_sparse_scratch_elems(const SegPlan& sp, i64 n)
{
    return (size_t)2 * n + (size_t)2 * (sp.npieces > 0 ? sp.npieces : 1) + (size_t)2 * ((n + 15) / 16);
}

// G: W'W (ldg doubles per row, complete on `st` before this); col_merged: sum of squares per column of the MERGED entries when the
// matrix stores duplicates, else null
int launch_residual_sparse(const SegPlan& sp, const i64* colptr, const double* val, i64 n, const double* Wt, const double* H, int ldf,
                           int k, const double* G, int ldg, const double* col_merged, double* scratch, double* col_r, double* col_a,
                           double* out2, hipStream_t st)
{
    double* col_t = scratch;
    double* col_s = col_t + n;
    double* pieces = col_s + n;
    double* blockpart = pieces + (size_t)2 * (sp.npieces > 0 ? sp.npieces : 1);
    SMK_HIP(hipMemsetAsync(col_t, 0, (size_t)2 * n * sizeof(double), st));      // columns without stored entries
    if (sp.nseg > 0) {
        const unsigned grid = (unsigned)((sp.nseg + 15) / 16);
        const int ku = k <= 16 ? 1 : k <= 32 ? 2 : k <= 64 ? 4 : 0;
#define SMK_SDDMM(KU) residual_sddmm_kernel<KU><<<grid, 256, 0, st>>>(sp.seg_p0, sp.seg_len, sp.seg_col, sp.seg_piece, sp.nseg, colptr, sp.rowflag, val, \
                                                                     Wt, H, ldf, k, col_t, col_s, pieces)
        switch (ku) { case 1: SMK_SDDMM(1); break; case 2: SMK_SDDMM(2); break; case 4: SMK_SDDMM(4); break; default: SMK_SDDMM(0); break; }
#undef SMK_SDDMM
        SMK_HIP(hipGetLastError());
        if (sp.nlong > 0) {
            residual_fixup_kernel<<<(unsigned)((sp.nlong + 255) / 256), 256, 0, st>>>(sp.long_col, sp.long_piece0, sp.nlong, pieces, col_t, col_s);
            SMK_HIP(hipGetLastError());
        }
    }
    const i64 nblk = (n + 15) / 16;
    const int lds_g = k <= 64 ? 1 : 0;
    residual_sparse_finish_kernel<<<(unsigned)(nblk < 4096 ? nblk : 4096), 256, lds_g ? (size_t)k * k * sizeof(double) : 0, st>>>(H, ldf, k, G, ldg, lds_g, n, col_t, col_s,
                                                                                                         col_merged, col_r, col_a, blockpart);
    SMK_HIP(hipGetLastError());
    residual_total_kernel<<<1, 1024, 0, st>>>(blockpart, nblk, out2);
    SMK_HIP(hipGetLastError());
    return 0;
}

}  // namespace smk
