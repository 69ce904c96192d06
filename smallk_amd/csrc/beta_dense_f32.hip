// smallk_amd/csrc/beta_dense_f32.hip -- the fp32 form of the dense KL (beta = 1) and Itakura-Saito (beta = 0) half-iterations
// (beta_dense_f32.cpp).  What is computed is kl_dense.hip's and beta_dense.hip's -- below the matrix is again `m` x
// `n` as stored, R the factor of its rows and X the factor of its columns, the one being updated; per entry (i, j, a)
//     d = r_i . x_j,  dc = max(d, EPS);    beta = 1: q = a / dc, num_j += q r_i;    beta = 0: r = 1 / dc, num_j += (r r a) r_i, den_j += r r_i
// -- but the factors live as fp32 (pitch KF = max(kp_of(k), 16) floats per row of R / column of X, rows >= k zero), the tile of
// the matrix is widened to fp32 and every per-entry operation is fp32 on v_mfma_f32_16x16x4_f32.  One value per factor entry is
// fp64: the finish kernel adds the spans' fp32 partials in span order in fp64, applies kl_update / beta_update (kl_dev.h) in fp64
// and rounds once, to the fp32 factor and to its exact fp64 widening (what the fp64 divergence and row-sum kernels read).
//
// This is not kl_dense_kernel with another type: that kernel is bound by staging 64 x 64 entries and a slab through registers
// into LDS between two barriers per tile.  Here
//   * LDS holds fp32, so two tile buffers fit (k <= 128: 136 KB against 150.5 KB for one fp64 buffer).  A tile is stored into the
//     buffer that is NOT being multiplied, the loads of the tile after it are issued, then the matrix cores run: ONE barrier per
//     tile, the global loads a whole tile ahead of their use.
//   * global loads and LDS accesses are 16 bytes wide: a lane loads 4 (fp32) or 8 (bf16, widened by a shift) consecutive rows
//     of a column and 4 consecutive factor rows of a slab row, and reads the matrix tile and the chained contraction's A operand
//     with one ds_read_b128 per four matrix instructions.
//   * with the slab pitch 68 every LDS access of the tile loop is free of bank conflicts: the product's contraction index is
//     permuted (lane group g takes factor row 16 Q + 4 g + s in step q = 4 Q + s, for both operands alike), so the four lane
//     groups read 16 banks each.
// The chained contraction carries over with ANOTHER row map.  v_mfma_f32_16x16x4_f32 leaves D[row 4 (lane >> 4) + reg][col
// lane & 15] in result register `reg` (the fp64 instruction: 4 reg + (lane >> 4)) and takes B[k = lane >> 4][j = lane & 15].  For
// a fixed reg of the 16-row block t the four lane groups hold the rows 16 t + {reg, 4 + reg, 8 + reg, 12 + reg} of one column
// each: a B operand over those four rows, whose A operand is R[row 16 t + 4 (lane >> 4) + reg][factor row 16 u + (lane & 15)] --
// four consecutive floats of a slab row for reg = 0 .. 3.  beta = 0 runs two chained contractions from the same d; they share
// those reads.  Every load is unconditional at a clamped address and masked afterwards, the step loops unroll through the template
// parameter, bases are scalar with one per-lane offset (residual.hip's three traps).  Fixed summation orders, no floating-point
// atomics: the same bits on every run.  Columns >= n, rows >= m and factor rows >= k are read as zero.
#include <algorithm>
#include <string>

#include "common.h"
#include "devutil.h"
#include "kl_dev.h"

namespace smk {

static constexpr int BF_T = 64;               // rows and columns of a tile
static constexpr int BF_P = 68;               // floats per factor row of a slab and per column of the matrix tile in LDS
static constexpr float BF_EPS = 1.1920928955078125e-07f;      // KL_EPS, exact in fp32

typedef __attribute__((ext_vector_type(4))) float f32x4;
typedef __attribute__((ext_vector_type(4))) unsigned u32x4;

static constexpr int bdf_lds_bytes(int KR) { return (3 * KR + 2 * BF_T) * BF_P * (int)sizeof(float); }

// KR: factor rows staged (16, 32, 64, 128; those from k on as zeros).  IS = false: beta = 1, part [S][KR][ncols_pad]; IS = true:
// beta = 0, part [S][2][KR][ncols_pad], numerator then denominator partials.  A's columns are 16-byte aligned and lda is a
// multiple of 16 bytes (the launcher checks), so a row group that starts below m ends inside its column.
template <int EBYTES, int KR, bool IS>
__global__ __launch_bounds__(256) void beta_dense_f32_kernel(const unsigned char* __restrict__ A, i64 lda_bytes, i64 m, i64 n,
                                                             const float* __restrict__ R, const float* __restrict__ X, int k, i64 row_tiles,
                                                             i64 tiles_per_span, int S, i64 ncols_pad, float* __restrict__ part)
{
    constexpr int NQ = KR / 4, NU = KR / 16;
    constexpr int V = 16 / EBYTES;                        // rows of the matrix per 16-byte load: 4 / 8
    constexpr int G = BF_T / V;                           // row groups per column: 16 / 8
    constexpr int NP = BF_T * G / 256;                    // loads per lane and tile: 4 / 2
    constexpr int CPP = 256 / G;                          // columns per pass: 16 / 32
    extern __shared__ __attribute__((aligned(16))) unsigned char bf_lds[];
    float* Xs = (float*)bf_lds;                           // [KR][BF_P]: X of the tile's columns, staged once per span
    float* Rs = Xs + KR * BF_P;                           // [2][KR][BF_P]: R of the tile's rows
    float* As = Rs + 2 * KR * BF_P;                       // [2][64 columns][BF_P]
    const i64 bid = blockIdx.x;
    const i64 ct = bid / S;
    const int sp = (int)(bid % S);
    const i64 rt0 = (i64)sp * tiles_per_span;
    i64 rt1 = rt0 + tiles_per_span;
    if (rt1 > row_tiles) rt1 = row_tiles;
    const i64 c0 = ct * BF_T;
    const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6), l15 = lane & 15, l4 = lane >> 4;
    f32x4 nacc[NU], dacc[IS ? NU : 1];
#pragma unroll
    for (int u = 0; u < NU; ++u) nacc[u] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int u = 0; u < (IS ? NU : 1); ++u) dacc[u] = f32x4{0.f, 0.f, 0.f, 0.f};
    // the matrix tile: pass p, column (tid / G) + CPP p, rows V (tid % G) .. + V - 1.  The column part of the address is fixed for
    // the span; the row part moves with the tile.
    const int ag = tid % G, ac = tid / G;
    i64 acol[NP];
#pragma unroll
    for (int p = 0; p < NP; ++p) {
        const i64 c = c0 + ac + CPP * p;
        acol[p] = (c < n ? c : n - 1) * lda_bytes;
    }
    const i64 last_group = (m - 1) / V * V;
    // a slab: a wave takes 16 rows (columns, for X), lane (r = lane >> 2, f = lane & 3) the factor rows 16 j + 4 f .. + 3 of row r
    const int sr = 16 * wave + (lane >> 2), sf = 4 * (lane & 3);
    u32x4 av[NP];
    f32x4 rv[NU];
    auto fetch = [&](i64 rt) {
        const i64 r0 = rt * BF_T;
        const i64 g0 = r0 + V * ag;
        const unsigned char* a0 = A + (g0 < last_group ? g0 : last_group) * EBYTES;
#pragma unroll
        for (int p = 0; p < NP; ++p) av[p] = __builtin_nontemporal_load((const u32x4*)(a0 + acol[p]));
        const i64 r = r0 + sr;
        const float* row = R + (r < m ? r : m - 1) * KR + sf;
#pragma unroll
        for (int j = 0; j < NU; ++j) rv[j] = *(const f32x4*)(row + 16 * j);
    };
    // registers -> the tile buffer b, masked: rows >= m, columns >= n and factor rows >= k become zeros
    auto stage = [&](i64 rt, int b) {
        const i64 r0 = rt * BF_T;
        float* Ab = As + b * BF_T * BF_P;
        float* Rb = Rs + b * KR * BF_P;
#pragma unroll
        for (int p = 0; p < NP; ++p) {
            const bool col_in = c0 + ac + CPP * p < n;
            float w[V];
            if constexpr (EBYTES == 4) {
#pragma unroll
                for (int e = 0; e < 4; ++e) {
                    const unsigned x = av[p][e];          // (a copy: a bit cast straight from the vector's element read element 0)
                    w[e] = __uint_as_float(x);
                }
            } else {
#pragma unroll
                for (int e = 0; e < 4; ++e) {
                    const unsigned x = av[p][e];
                    w[2 * e] = __uint_as_float(x << 16);
                    w[2 * e + 1] = __uint_as_float(x & 0xFFFF0000u);
                }
            }
#pragma unroll
            for (int e = 0; e < V; ++e) w[e] = (col_in && r0 + V * ag + e < m) ? w[e] : 0.f;
#pragma unroll
            for (int h = 0; h < V / 4; ++h)
                *(f32x4*)(Ab + (ac + CPP * p) * BF_P + V * ag + 4 * h) = f32x4{w[4 * h], w[4 * h + 1], w[4 * h + 2], w[4 * h + 3]};
        }
        const bool row_in = r0 + sr < m;
#pragma unroll
        for (int j = 0; j < NU; ++j)
#pragma unroll
            for (int e = 0; e < 4; ++e) Rb[(16 * j + sf + e) * BF_P + sr] = (row_in && 16 * j + sf + e < k) ? rv[j][e] : 0.f;
    };
    if (rt0 < rt1) {
        {   // the tile's columns of X, once per span
            const i64 c = c0 + sr;
            const float* colp = X + (c < n ? c : n - 1) * KR + sf;
            f32x4 xv[NU];
#pragma unroll
            for (int j = 0; j < NU; ++j) xv[j] = *(const f32x4*)(colp + 16 * j);
#pragma unroll
            for (int j = 0; j < NU; ++j)
#pragma unroll
                for (int e = 0; e < 4; ++e) Xs[(16 * j + sf + e) * BF_P + sr] = (c < n && 16 * j + sf + e < k) ? xv[j][e] : 0.f;
        }
        fetch(rt0);
        stage(rt0, 0);
        fetch(rt0 + 1 < rt1 ? rt0 + 1 : rt1 - 1);
        __syncthreads();
        int cur = 0;
        for (i64 rt = rt0; rt < rt1; ++rt, cur ^= 1) {
            // the next tile into the other buffer (its readers finished before the last barrier), the loads of the one after it,
            // then the matrix cores on this one.  Past the span's end the last tile is staged again and nobody reads it.
            const i64 nx = rt + 1 < rt1 ? rt + 1 : rt1 - 1;
            stage(nx, cur ^ 1);
            fetch(rt + 2 < rt1 ? rt + 2 : rt1 - 1);
            const float* Ab = As + cur * BF_T * BF_P;
            const float* Rb = Rs + cur * KR * BF_P;
            f32x4 acc[4];
#pragma unroll
            for (int t = 0; t < 4; ++t) acc[t] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
            for (int q = 0; q < NQ; ++q) {
                const int kk = 16 * (q >> 2) + 4 * l4 + (q & 3);          // the permuted contraction index, the same for both operands
                const float b = Xs[kk * BF_P + 16 * wave + l15];
#pragma unroll
                for (int t = 0; t < 4; ++t) acc[t] = __builtin_amdgcn_mfma_f32_16x16x4f32(Rb[kk * BF_P + 16 * t + l15], b, acc[t], 0, 0, 0);
            }
#pragma unroll
            for (int t = 0; t < 4; ++t) {
                // rows 16 t + 4 l4 + {0 .. 3} of column 16 wave + l15: the rows of this lane's four result registers
                const f32x4 a4 = *(const f32x4*)(Ab + (16 * wave + l15) * BF_P + 16 * t + 4 * l4);
                f32x4 qn, qd;
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    const float d = acc[t][r] < BF_EPS ? BF_EPS : acc[t][r];
                    if constexpr (IS) {
                        const float rc = 1.f / d;
                        qn[r] = __fmul_rn(__fmul_rn(rc, rc), a4[r]);
                        qd[r] = rc;
                    } else {
                        qn[r] = a4[r] / d;
                    }
                }
#pragma unroll
                for (int u = 0; u < NU; ++u) {
                    const f32x4 r4 = *(const f32x4*)(Rb + (16 * u + l15) * BF_P + 16 * t + 4 * l4);
#pragma unroll
                    for (int r = 0; r < 4; ++r) {
                        nacc[u] = __builtin_amdgcn_mfma_f32_16x16x4f32(r4[r], qn[r], nacc[u], 0, 0, 0);
                        if constexpr (IS) dacc[u] = __builtin_amdgcn_mfma_f32_16x16x4f32(r4[r], qd[r], dacc[u], 0, 0, 0);
                    }
                }
            }
            __syncthreads();
        }
    }
    // result register r of block u: factor row 16 u + 4 l4 + r of column 16 wave + l15
    const i64 col = c0 + 16 * wave + l15;                 // < ncols_pad
#pragma unroll
    for (int u = 0; u < NU; ++u)
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const int t = 16 * u + 4 * l4 + r;
            if constexpr (IS) {
                part[(((i64)sp * 2) * KR + t) * ncols_pad + col] = nacc[u][r];
                part[(((i64)sp * 2 + 1) * KR + t) * ncols_pad + col] = dacc[u][r];
            } else {
                part[((i64)sp * KR + t) * ncols_pad + col] = nacc[u][r];
            }
        }
}

// the spans of a (factor row, column) in span order in fp64, the update in fp64 (kl_dev.h), one rounding: to the fp32 factor X
// (pitch KR) and to its exact widening X64 (pitch KP).  Rows >= k are written as zeros.  base / unit: beta = 1's row sums.
template <bool IS>
__global__ __launch_bounds__(256) void beta_dense_f32_finish_kernel(const float* __restrict__ part, int S, int KR, i64 ncols_pad, i64 n,
                                                                    float* __restrict__ X, double* __restrict__ X64, int KP, int k,
                                                                    const double* __restrict__ base, int unit, double l1, double l2, int flush)
{
    const i64 j = (i64)blockIdx.x * 64 + (threadIdx.x & 63);
    if (j >= n) return;
    for (int t = threadIdx.x >> 6; t < KR; t += 4) {
        float xn = 0.f;
        if (t < k) {
            double num = 0.0, den = 0.0;
            for (int s = 0; s < S; ++s) {
                if constexpr (IS) {
                    num += (double)part[(((i64)s * 2) * KR + t) * ncols_pad + j];
                    den += (double)part[(((i64)s * 2 + 1) * KR + t) * ncols_pad + j];
                } else {
                    num += (double)part[((i64)s * KR + t) * ncols_pad + j];
                }
            }
            const double x = (double)X[j * KR + t];
            if constexpr (IS) xn = (float)beta_update(x, num, den, l1, l2, 1, 0.5, flush);
            else xn = (float)kl_update(x, num, base[t], unit, l1, l2, flush);
        }
        X[j * KR + t] = xn;
        if (t < KP) X64[j * KP + t] = (double)xn;
    }
}

// X64 (pitch KP) rounded once to X (pitch KR), and X64 replaced by the exact widening of what X holds; rows >= k become zeros
__global__ __launch_bounds__(256) void beta_dense_f32_narrow_kernel(double* __restrict__ X64, int KP, float* __restrict__ X, int KR, int k, i64 n)
{
    const i64 j = (i64)blockIdx.x * 64 + (threadIdx.x & 63);
    if (j >= n) return;
    for (int t = threadIdx.x >> 6; t < KR; t += 4) {
        const float v = t < k ? (float)X64[j * KP + t] : 0.f;
        X[j * KR + t] = v;
        if (t < KP) X64[j * KP + t] = (double)v;
    }
}

// ---- launchers ---------------------------------------------------------------------------------------------------------
int beta_dense_f32_pitch(int k) { return k > 64 ? 128 : k > 32 ? 64 : k > 16 ? 32 : 16; }

size_t beta_dense_f32_scratch_bytes(i64 rows, i64 cols, int k, double beta, int num_cus)
{
    i64 rt, ctl, per; int S;
    residual_dense_shape(rows, cols, num_cus, &rt, &ctl, &per, &S);
    return (size_t)(beta == 0.0 ? 2 : 1) * S * beta_dense_f32_pitch(k) * ctl * BF_T * sizeof(float);
}

template <int EBYTES, int KR, bool IS>
static int bdf_launch(unsigned grid, const unsigned char* A, i64 lda_bytes, i64 m, i64 n, const float* R, const float* X, int k, i64 rt, i64 per,
                      int S, i64 ncols_pad, float* part, hipStream_t st)
{
    constexpr int lds = bdf_lds_bytes(KR);
    if constexpr (lds > 64 * 1024) {
        static std::atomic<unsigned long long> attr_set{0};       // per device (DeviceOnce)
        if (DeviceOnce once{attr_set}) {
            SMK_HIP(hipFuncSetAttribute((const void*)beta_dense_f32_kernel<EBYTES, KR, IS>, hipFuncAttributeMaxDynamicSharedMemorySize, lds));
            once.done();
        }
    }
    beta_dense_f32_kernel<EBYTES, KR, IS><<<grid, 256, lds, st>>>(A, lda_bytes, m, n, R, X, k, rt, per, S, ncols_pad, part);
    return 0;
}

template <bool IS>
static int bdf_step(const void* A, int storage, i64 ld, i64 rows, i64 cols, const float* R, float* X, double* X64, int k, const double* base, int unit,
                    double l1, double l2, int flush, float* part, int num_cus, hipStream_t st)
{
    i64 rt, ctl, per; int S;
    residual_dense_shape(rows, cols, num_cus, &rt, &ctl, &per, &S);
    const i64 ncols_pad = ctl * BF_T;
    if (ctl * S > 0x7FFFFFFFll) { set_error("beta_dense_f32: matrix too wide for one launch"); return -100; }
    const int eb = storage == STORE_BF16 ? 2 : 4;
    // the 16-byte loads: whole row groups inside every column
    if (((uintptr_t)A & 15) || (ld * eb) % 16 || ld < rows) { set_error("beta_dense_f32: the stored matrix is not 16-byte aligned column by column"); return -3; }
    const unsigned grid = (unsigned)(ctl * S);
    const int KR = beta_dense_f32_pitch(k);
    int rc = 0;
#define SMK_BF(EB, KRV) rc = bdf_launch<EB, KRV, IS>(grid, (const unsigned char*)A, ld * EB, rows, cols, R, X, k, rt, per, S, ncols_pad, part, st)
#define SMK_BF_KR(EB)                                  \
    switch (KR) {                                      \
        case 16: SMK_BF(EB, 16); break;                \
        case 32: SMK_BF(EB, 32); break;                \
        case 64: SMK_BF(EB, 64); break;                \
        default: SMK_BF(EB, 128); break;               \
    }
    if (eb == 2) { SMK_BF_KR(2) } else { SMK_BF_KR(4) }
#undef SMK_BF_KR
#undef SMK_BF
    if (rc) return rc;
    SMK_HIP(hipGetLastError());
    beta_dense_f32_finish_kernel<IS><<<(unsigned)((cols + 63) / 64), 256, 0, st>>>(part, S, KR, ncols_pad, cols, X, X64, kp_of(k), k, base, unit, l1, l2,
                                                                                  flush);
    SMK_HIP(hipGetLastError());
    return 0;
}

int launch_beta_dense_f32_step(const void* A, int storage, i64 ld, i64 rows, i64 cols, const float* R, float* X, double* X64, int k, double beta,
                               const double* base, int unit, double l1, double l2, int flush, float* scratch, int num_cus, hipStream_t st)
{
    if (k < 1 || k > 128 || rows < 1 || cols < 1 || (beta != 0.0 && beta != 1.0) || (beta == 1.0 && !base)) {
        set_error("launch_beta_dense_f32_step: k in [1, 128], a matrix with entries, beta 0 or 1 (with the row sums)");
        return -3;
    }
    if (beta == 0.0) return bdf_step<true>(A, storage, ld, rows, cols, R, X, X64, k, nullptr, 0, l1, l2, flush, scratch, num_cus, st);
    return bdf_step<false>(A, storage, ld, rows, cols, R, X, X64, k, base, unit, l1, l2, flush, scratch, num_cus, st);
}

int launch_beta_dense_f32_narrow(double* X64, float* X, int k, i64 N, hipStream_t st)
{
    beta_dense_f32_narrow_kernel<<<(unsigned)((N + 63) / 64), 256, 0, st>>>(X64, kp_of(k), X, beta_dense_f32_pitch(k), k, N);
    SMK_HIP(hipGetLastError());
    return 0;
}

}  // namespace smk
