// smallk_amd/csrc/kl_dense.hip -- the kernels of KL-divergence NMF on a dense stored matrix (kl_dense.cpp): scikit-learn's
// multiplicative update for beta_loss = 1, the iteration of kl.hip over EVERY entry of the matrix.  A half-iteration is one streaming
// read of one stored matrix -- A for the H step, the stored transpose for the W step; below the matrix is `m` x `n` as stored, R
// (KP x m) the factor of its rows and X (KP x n) the factor of its columns, the one being updated.  Per entry (i, j, a):
//     d = r_i . x_j,   q = a / max(d, EPS),   num_j += q r_i
// and per column   x_j[t] *= num_j[t] / den[t]   (kl_dev.h: kl_update).  A stored zero gives q = 0 exactly, so the result is the
// sparse path's on the same data up to summation order.
//
// The structure is residual_dense_kernel's (residual.hip; read its comments: loads under branches, run-time step bounds and
// per-lane 64-bit addresses are its three measured traps, and all three are avoided the same way here).  A workgroup owns a
// 64-column tile and a span of 64-row tiles.  Per tile TWO chained contractions on v_mfma_f64_16x16x4_f64:
//   1. acc = R_tile' X_tile over the rank (A operand R, B operand X), as the residual forms (W H)_tile;
//   2. after acc has become the quotient in place, num[t, c] += sum_r R[r, t] q[r, c] over the 64 rows of the tile.
// The second needs no shuffle and no LDS round trip.  The instruction leaves D[row = 4 reg + (lane >> 4)][col = lane & 15] in
// result register `reg` and wants B[k = lane >> 4][j = lane & 15] as its B operand: register `reg` of the 16-row block t IS the B
// operand of the step that contracts over the rows 16 t + 4 reg + {0 .. 3}.  Its A operand, A[i = lane & 15][k = lane >> 4] =
// R[row 16 t + 4 reg + (lane >> 4)][factor row 16 u + (lane & 15)] for the output block u, is read from the slab of R that the
// first contraction has already staged.  So a tile costs 4 NQ matrix instructions for the product and 16 NU for the numerator per
// wave (NQ = KR / 4 steps, NU = max(KR, 16) / 16 blocks): the same number, twice the residual pass, from KR = 16 on.
// The numerator tile (KS x 64 per workgroup, KS x 16 per wave) stays in the result registers across the span; one partial per
// (span, factor row, column); kl_dense_finish_kernel adds the spans in span order and applies the update.
// Ranks above 64: both 64-row groups of both factors are staged (KR = 128: 150 KB of LDS, one workgroup per CU), so the dot
// product is complete before any quotient is formed and the numerator finds both groups of R where the product left them.
// Every sum has a fixed order: the same bits on every run, no floating-point atomics.  Columns >= n, rows >= m and factor rows
// >= k are read as zero here: neither the padding of the matrix nor pad rows of a factor are relied on.
#include <algorithm>

#include "common.h"
#include "devutil.h"
#include "kl_dev.h"

namespace smk {

static constexpr int KD_T = 64;               // rows and columns of a tile
static constexpr int KD_FP = 65;              // doubles per factor row of a slab in LDS (as RES_FP)
static constexpr int KD_AP = 68;              // floats per column of the matrix tile in LDS (as RES_AP)

// NQ: contraction steps of the product (KR = 4 NQ factor rows staged: 4, 8, 16, 32, 64, 128; those from k on as zeros), a template
// parameter so that both step loops unroll.  DIV = false: the step.  DIV = true: the same product, then per column
// sum a log(a / max(d, EPS)) and sum a over the entries with a > EPS instead of the quotient and the numerator; X is only read.
// part: !DIV [S][KS][ncols_pad] numerator partials; DIV [2][S][ncols_pad] (the log sums, then the sums of a).
template <int EBYTES, int NQ, bool DIV>
__global__ __launch_bounds__(256) void kl_dense_kernel(const unsigned char* __restrict__ A, i64 lda_bytes, i64 m, i64 n,
                                                       const double* __restrict__ R, const double* __restrict__ X, int ldf, int k,
                                                       i64 row_tiles, i64 tiles_per_span, int S, i64 ncols_pad, double* __restrict__ part)
{
    constexpr int KR = 4 * NQ;
    constexpr int KS = KR < 16 ? 16 : KR;                 // rows of R's slab: whole 16-row output blocks of the numerator
    constexpr int NU = KS / 16;
    constexpr int NG = (KR + KD_T - 1) / KD_T;            // 64-lane groups of factor rows
    extern __shared__ __attribute__((aligned(16))) unsigned char kd_lds[];
    double* Rs = (double*)kd_lds;                         // [KS][KD_FP]: R of the tile's rows
    double* Xs = Rs + KS * KD_FP;                         // [KR][KD_FP]: X of the tile's columns
    float* As = (float*)(Xs + KR * KD_FP);                // [64 columns][KD_AP]
    const i64 bid = blockIdx.x;                           // 1-D grid, 64-bit tile arithmetic
    const i64 ct = bid / S;
    const int sp = (int)(bid % S);
    const i64 rt0 = (i64)sp * tiles_per_span;
    i64 rt1 = rt0 + tiles_per_span;
    if (rt1 > row_tiles) rt1 = row_tiles;
    const i64 c0 = ct * KD_T;
    const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6), l15 = lane & 15, l4 = lane >> 4;
    typedef __attribute__((ext_vector_type(4))) double f64x4;
    f64x4 acc[4];
    f64x4 nacc[DIV ? 1 : NU];
    double tacc = 0.0, sacc = 0.0;
#pragma unroll
    for (int u = 0; u < (DIV ? 1 : NU); ++u) nacc[u] = f64x4{0.0, 0.0, 0.0, 0.0};
    // the matrix tile and R's rows of tile rt + 1 are loaded into registers while the matrix cores work on tile rt; every load is
    // unconditional at a clamped address and masked afterwards (residual.hip).  Trip i of a wave: column / row 4 i + wave, the lane
    // = the row of the matrix / the factor row (of group g: 64 g + lane).
    float bv[16];
    double rv[NG][16];
    int kc[NG];
#pragma unroll
    for (int g = 0; g < NG; ++g) kc[g] = 64 * g + lane < k ? 64 * g + lane : k - 1;
    auto fetch = [&](i64 rt) {
        const i64 r0 = rt * KD_T;
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
        for (int g = 0; g < NG; ++g)
#pragma unroll
            for (int i = 0; i < 16; ++i) {
                const i64 r = r0 + 4 * i + wave;
                const double* row = R + (r < m ? r : m - 1) * ldf;                   // scalar
                rv[g][i] = row[kc[g]];              // masked when it is stored to LDS (below)
            }
    };
    auto pin = [&](double (&t)[16]) {
#pragma unroll
        for (int i = 0; i < 16; ++i) asm volatile("" : "+v"(t[i]));
    };
    // the tile's columns of X: global (L2) -> registers -> LDS, once per span (every group stays)
#pragma unroll
    for (int g = 0; g < NG; ++g) {
        double t[16];
#pragma unroll
        for (int i = 0; i < 16; ++i) {
            const i64 c = c0 + 4 * i + wave;
            t[i] = X[(c < n ? c : n - 1) * ldf + kc[g]];
        }
        pin(t);
        if (64 * g + lane < KR) {
#pragma unroll
            for (int i = 0; i < 16; ++i) Xs[(64 * g + lane) * KD_FP + 4 * i + wave] = (c0 + 4 * i + wave < n && 64 * g + lane < k) ? t[i] : 0.0;
        }
    }
    if (rt0 < rt1) fetch(rt0);
    for (i64 rt = rt0; rt < rt1; ++rt) {
#pragma unroll
        for (int t = 0; t < 4; ++t) acc[t] = f64x4{0.0, 0.0, 0.0, 0.0};
#pragma unroll
        for (int i = 0; i < 16; ++i) {
            As[(4 * i + wave) * KD_AP + lane] = bv[i];
#pragma unroll
            for (int g = 0; g < NG; ++g)
                if (64 * g + lane < KS) Rs[(64 * g + lane) * KD_FP + 4 * i + wave] = (rt * KD_T + 4 * i + wave < m && 64 * g + lane < k) ? rv[g][i] : 0.0;
        }
        __syncthreads();
        if (rt + 1 < rt1) fetch(rt + 1);
#pragma unroll
        for (int q = 0; q < NQ; ++q) {
            const double b = Xs[(4 * q + l4) * KD_FP + 16 * wave + l15];
#pragma unroll
            for (int t = 0; t < 4; ++t) acc[t] = __builtin_amdgcn_mfma_f64_16x16x4f64(Rs[(4 * q + l4) * KD_FP + 16 * t + l15], b, acc[t], 0, 0, 0);
        }
#pragma unroll
        for (int t = 0; t < 4; ++t)
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const double av = (double)As[(16 * wave + l15) * KD_AP + 16 * t + l4 + 4 * r];
                const double d = acc[t][r] < KL_EPS ? KL_EPS : acc[t][r];
                if constexpr (DIV) {
                    if (av > KL_EPS) { tacc = __builtin_fma(av, log(av / d), tacc); sacc += av; }
                } else {
                    // (the one place another beta-divergence would enter: Itakura-Saito's quotient is a / d^2 against 1 / d)
                    acc[t][r] = av / d;
                }
            }
        if constexpr (!DIV) {
#pragma unroll
            for (int t = 0; t < 4; ++t)
#pragma unroll
                for (int r = 0; r < 4; ++r)
#pragma unroll
                    for (int u = 0; u < NU; ++u)
                        nacc[u] = __builtin_amdgcn_mfma_f64_16x16x4f64(Rs[(16 * u + l15) * KD_FP + 16 * t + 4 * r + l4], acc[t][r], nacc[u], 0, 0, 0);
        }
        __syncthreads();
    }
    const i64 col = c0 + 16 * wave + l15;                 // < ncols_pad
    if constexpr (DIV) {
        // the four lanes of a column, fixed order; one pair per (span, column)
        tacc += __shfl_xor(tacc, 16, 64);
        tacc += __shfl_xor(tacc, 32, 64);
        sacc += __shfl_xor(sacc, 16, 64);
        sacc += __shfl_xor(sacc, 32, 64);
        if (l4 == 0) {
            part[(i64)sp * ncols_pad + col] = tacc;
            part[((i64)S + sp) * ncols_pad + col] = sacc;
        }
    } else {
#pragma unroll
        for (int u = 0; u < NU; ++u)
#pragma unroll
            for (int r = 0; r < 4; ++r) part[((i64)sp * KS + 16 * u + 4 * r + l4) * ncols_pad + col] = nacc[u][r];
    }
}

// the spans of a (factor row, column) in span order, then the update of X in place.  A workgroup takes 64 columns; thread (c, g)
// the factor rows g, g + 4, ... of column c: the partials are read along the columns.
__global__ __launch_bounds__(256) void kl_dense_finish_kernel(const double* __restrict__ part, int S, int KS, i64 ncols_pad, i64 n,
                                                              double* __restrict__ X, int KP, int k, const double* __restrict__ base, int unit,
                                                              double l1, double l2, int flush)
{
    const i64 j = (i64)blockIdx.x * 64 + (threadIdx.x & 63);
    if (j >= n) return;
    for (int t = threadIdx.x >> 6; t < KP; t += 4) {
        double xn = 0.0;
        if (t < k) {
            double num = 0.0;
            for (int s = 0; s < S; ++s) num += part[((i64)s * KS + t) * ncols_pad + j];
            xn = kl_update(X[j * KP + t], num, base[t], unit, l1, l2, flush);
        }
        X[j * KP + t] = xn;
    }
}

// the spans of a column in span order; 256 columns per workgroup, whose two sums go to blockpart in column order (as
// residual_colsum_kernel: 16 sums of 16, then their sum)
__global__ __launch_bounds__(256) void kl_dense_colsum_kernel(const double* __restrict__ part, int S, i64 ncols_pad, i64 n,
                                                              double* __restrict__ blockpart)
{
    __shared__ double sh[256][2];
    const i64 j = (i64)blockIdx.x * 256 + threadIdx.x;
    double t = 0.0, s = 0.0;
    if (j < n)
        for (int q = 0; q < S; ++q) { t += part[(i64)q * ncols_pad + j]; s += part[((i64)S + q) * ncols_pad + j]; }
    sh[threadIdx.x][0] = t;
    sh[threadIdx.x][1] = s;
    __syncthreads();
    double t2 = 0.0, s2 = 0.0;
    if (threadIdx.x < 16)
        for (int i = 0; i < 16; ++i) { t2 += sh[16 * threadIdx.x + i][0]; s2 += sh[16 * threadIdx.x + i][1]; }
    __syncthreads();
    if (threadIdx.x < 16) { sh[threadIdx.x][0] = t2; sh[threadIdx.x][1] = s2; }
    __syncthreads();
    if (threadIdx.x == 0) {
        double tt = 0.0, ss = 0.0;
        for (int i = 0; i < 16; ++i) { tt += sh[i][0]; ss += sh[i][1]; }
        blockpart[2 * (i64)blockIdx.x] = tt;
        blockpart[2 * (i64)blockIdx.x + 1] = ss;
    }
}

// the workgroups' sums in index order (thread t takes t, t + 1024, ..., then a tree over the 1024 threads), sum WH from the row
// sums: out[0] = D = sum a log(a / d) + (sum WH - sum a), out[1] = sum a log(a / d), out[2] = sum WH, out[3] = sum a; host_out: pinned or null
__global__ __launch_bounds__(1024) void kl_dense_total_kernel(const double* __restrict__ blockpart, i64 nblk, const double* __restrict__ sums_a,
                                                              const double* __restrict__ sums_b, int k, double* __restrict__ out, double* host_out)
{
    __shared__ double sh[1024][2];
    double t = 0.0, s = 0.0;
    for (i64 b = threadIdx.x; b < nblk; b += 1024) { t += blockpart[2 * b]; s += blockpart[2 * b + 1]; }
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

// is a stored value negative (bit 0 of *flag), is one zero or negative (bit 1: what beta <= 0 refuses, beta_dense.cpp)?  A workgroup walks columns, its threads the rows of a column; only rows < m and columns < n are read
template <int EBYTES>
__global__ __launch_bounds__(256) void kl_dense_negative_kernel(const unsigned char* __restrict__ A, i64 lda_bytes, i64 m, i64 n, int* flag)
{
    int found = 0;
    for (i64 c = blockIdx.x; c < n; c += gridDim.x) {
        const unsigned char* col = A + c * lda_bytes;
        for (i64 r = threadIdx.x; r < m; r += 256) {
            float v;
            if constexpr (EBYTES == 2) v = bf16_bits_to_f32(((const unsigned short*)col)[r]);
            else v = ((const float*)col)[r];
            if (v < 0.f) found |= 1;
            if (!(v > 0.f)) found |= 2;
        }
    }
    if (found) atomicOr(flag, found);
}

// ---- launchers ---------------------------------------------------------------------------------------------------------
static int kl_dense_nq(int k) { return k > 64 ? 32 : k > 32 ? 16 : k > 16 ? 8 : k > 8 ? 4 : k > 4 ? 2 : 1; }
static int kl_dense_ks(int k) { const int kr = 4 * kl_dense_nq(k); return kr < 16 ? 16 : kr; }

size_t kl_dense_scratch_elems(i64 rows, i64 cols, int k, int num_cus)
{
    i64 rt, ctl, per; int S;
    residual_dense_shape(rows, cols, num_cus, &rt, &ctl, &per, &S);
    const size_t step = (size_t)S * kl_dense_ks(k) * ctl * KD_T;
    const size_t div = (size_t)2 * S * ctl * KD_T + (size_t)2 * ((cols + 255) / 256);
    return step > div ? step : div;
}

template <int EBYTES, int NQ, bool DIV>
static int kl_dense_launch(unsigned grid, const unsigned char* A, i64 lda_bytes, i64 m, i64 n, const double* R, const double* X, int ldf, int k,
                           i64 rt, i64 per, int S, i64 ncols_pad, double* part, hipStream_t st)
{
    constexpr int KR = 4 * NQ, KS = KR < 16 ? 16 : KR;
    constexpr int lds = (KS + KR) * KD_FP * (int)sizeof(double) + KD_T * KD_AP * (int)sizeof(float);
    if constexpr (lds > 64 * 1024) {
        static std::atomic<unsigned long long> attr_set{0};       // per device (DeviceOnce)
        if (DeviceOnce once{attr_set}) {
            SMK_HIP(hipFuncSetAttribute((const void*)kl_dense_kernel<EBYTES, NQ, DIV>, hipFuncAttributeMaxDynamicSharedMemorySize, lds));
            once.done();
        }
    }
    kl_dense_kernel<EBYTES, NQ, DIV><<<grid, 256, lds, st>>>(A, lda_bytes, m, n, R, X, ldf, k, rt, per, S, ncols_pad, part);
    return 0;
}

template <bool DIV>
static int kl_dense_dispatch(const void* A, int storage, i64 ld, i64 m, i64 n, const double* R, const double* X, int k, double* part, int num_cus,
                             hipStream_t st, int* S_out, i64* ncols_pad_out)
{
    i64 rt, ctl, per; int S;
    residual_dense_shape(m, n, num_cus, &rt, &ctl, &per, &S);
    const i64 ncols_pad = ctl * KD_T;
    if (ctl * S > 0x7FFFFFFFll) { set_error("kl_dense: matrix too wide for one launch"); return -100; }
    const unsigned grid = (unsigned)(ctl * S);
    const int ldf = kp_of(k);
    int rc = 0;
#define SMK_KD(EB, NQ) rc = kl_dense_launch<EB, NQ, DIV>(grid, (const unsigned char*)A, ld * EB, m, n, R, X, ldf, k, rt, per, S, ncols_pad, part, st)
#define SMK_KD_NQ(EB)                                  \
    switch (kl_dense_nq(k)) {                          \
        case 1: SMK_KD(EB, 1); break;                  \
        case 2: SMK_KD(EB, 2); break;                  \
        case 4: SMK_KD(EB, 4); break;                  \
        case 8: SMK_KD(EB, 8); break;                  \
        case 16: SMK_KD(EB, 16); break;                \
        default: SMK_KD(EB, 32); break;                \
    }
    if (storage == STORE_BF16) { SMK_KD_NQ(2) } else { SMK_KD_NQ(4) }
#undef SMK_KD_NQ
#undef SMK_KD
    if (rc) return rc;
    SMK_HIP(hipGetLastError());
    *S_out = S;
    *ncols_pad_out = ncols_pad;
    return 0;
}

int launch_kl_dense_step(const void* A, int storage, i64 ld, i64 rows, i64 cols, const double* R, double* X, int k, const double* base, int unit,
                         double l1, double l2, int flush, double* scratch, int num_cus, hipStream_t st)
{
    if (k < 1 || k > 128 || rows < 1 || cols < 1) { set_error("launch_kl_dense_step: k in [1, 128] and a matrix with entries"); return -3; }
    int S = 0;
    i64 ncols_pad = 0;
    const int rc = kl_dense_dispatch<false>(A, storage, ld, rows, cols, R, X, k, scratch, num_cus, st, &S, &ncols_pad);
    if (rc) return rc;
    kl_dense_finish_kernel<<<(unsigned)((cols + 63) / 64), 256, 0, st>>>(scratch, S, kl_dense_ks(k), ncols_pad, cols, X, kp_of(k), k, base, unit, l1, l2,
                                                                        flush);
    SMK_HIP(hipGetLastError());
    return 0;
}

int launch_kl_dense_divergence(const void* A, int storage, i64 ld, i64 rows, i64 cols, const double* R, const double* X, int k, const double* sums_r,
                               const double* sums_x, double* scratch, double* out4, double* host_out, int num_cus, hipStream_t st)
{
    if (k < 1 || k > 128 || rows < 1 || cols < 1) { set_error("launch_kl_dense_divergence: k in [1, 128] and a matrix with entries"); return -3; }
    int S = 0;
    i64 ncols_pad = 0;
    const int rc = kl_dense_dispatch<true>(A, storage, ld, rows, cols, R, X, k, scratch, num_cus, st, &S, &ncols_pad);
    if (rc) return rc;
    double* blockpart = scratch + (size_t)2 * S * ncols_pad;
    const i64 nblk = (cols + 255) / 256;
    kl_dense_colsum_kernel<<<(unsigned)nblk, 256, 0, st>>>(scratch, S, ncols_pad, cols, blockpart);
    SMK_HIP(hipGetLastError());
    kl_dense_total_kernel<<<1, 1024, 0, st>>>(blockpart, nblk, sums_r, sums_x, k, out4, host_out);
    SMK_HIP(hipGetLastError());
    return 0;
}

int launch_kl_dense_negative(const void* A, int storage, i64 ld, i64 rows, i64 cols, int* flag, hipStream_t st)
{
    const unsigned grid = (unsigned)std::min<i64>(cols, 4096);
    if (storage == STORE_BF16) kl_dense_negative_kernel<2><<<grid, 256, 0, st>>>((const unsigned char*)A, ld * 2, rows, cols, flag);
    else kl_dense_negative_kernel<4><<<grid, 256, 0, st>>>((const unsigned char*)A, ld * 4, rows, cols, flag);
    SMK_HIP(hipGetLastError());
    return 0;
}

}  // namespace smk
