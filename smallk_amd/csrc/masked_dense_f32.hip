// smallk_amd/csrc/masked_dense_f32.hip -- the fp32 form of the masked dense half-iterations for beta = 2 (Frobenius), 1
// (Kullback-Leibler) and 0 (Itakura-Saito) (masked_dense_f32.cpp).  What is computed is masked_dense.hip's -- a stored
// NaN is "not measured", the matrix is `m` x `n` as stored, R the factor of its rows and X the factor of its columns, the one being
// updated; per MEASURED entry (i, j, a), d = r_i . x_j:
//     MF_FRO (beta = 2):  qn = a,                 qd = d          no clamp, no division
//     MF_KL  (beta = 1):  qn = a / max(d, EPS),   qd = 1          a second contraction with the 0 / 1 mask, not a vector of row sums
//     MF_IS  (beta = 0):  r = 1 / max(d, EPS),    qn = (r r) a,   qd = r
// num_j += qn r_i, den_j += qd r_i -- but every per-entry operation is fp32 on v_mfma_f32_16x16x4_f32 and the factors live as fp32
// (pitch KR = max(kp_of(k), 16) floats per row of R / column of X, rows >= k zero).  One value per factor entry is fp64: the finish
// kernel adds the spans' fp32 partials in span order in fp64, applies beta_update (kl_dev.h) in fp64 and rounds once, to the fp32
// factor and to its exact fp64 widening (what the fp64 divergence of masked_dense.hip reads).
//
// The frame is beta_dense_f32_kernel's -- read its comments for the register map: two tile buffers and two slabs of R in LDS at
// pitch 68, the next tile stored into the buffer that is not being multiplied, the loads of the one after it in flight, ONE barrier
// per tile; 16-byte global loads of 4 (fp32) or 8 (bf16) consecutive rows of a column; the permuted contraction index; one
// ds_read_b128 of R's slab per four rows of a lane's result registers.  What differs:
//   * numerator AND denominator are chained contractions in all three modes; one read of R's slab feeds eight matrix instructions
//     (four of each sum), so beta = 2 and beta = 1 cost the matrix instructions of beta = 0 and only the per-entry work differs;
//   * the tile of A is read from LDS as BITS.  "Measured" is (bits & 0x7FFFFFFF) <= 0x7F800000 on the scalar copy of an element
//     (a bit cast straight from a vector's element read element 0: DESIGN.md 23), a is SELECTED to 0.f before any arithmetic and qn,
//     qd of an unmeasured entry are selected to 0.f -- never multiplied by a mask: no NaN reaches a matrix-instruction operand;
//   * padding is the missing marker: rows >= m and columns >= n of a tile are staged as the canonical NaN (beta_dense_f32_kernel
//     stages 0.f, which here would be a measured zero with qd = 1 or 1 / EPS).  The widening shift of bf16 storage turns 0x7FC0 into
//     0x7FC00000 by itself.  Factor rows >= k and slab rows >= m are staged as zeros.
// Every load is unconditional at a clamped address and masked afterwards, the step loops unroll through the template parameter,
// bases are scalar with one per-lane offset.  Fixed summation orders, no atomics: the same bits on every run.
#include <algorithm>
#include <string>

#include "common.h"
#include "devutil.h"
#include "kl_dev.h"

namespace smk {

static constexpr int MF_T = 64;               // rows and columns of a tile
static constexpr int MF_P = 68;               // floats per factor row of a slab and per column of the matrix tile in LDS
static constexpr int MF_IS = 0, MF_KL = 1, MF_FRO = 2;        // the mode is beta itself
static constexpr unsigned MF_NAN = 0x7FC00000u;               // the canonical quiet NaN: what padding is staged as
static constexpr float MF_EPS = 1.1920928955078125e-07f;      // KL_EPS, exact in fp32

typedef __attribute__((ext_vector_type(4))) float f32x4;
typedef __attribute__((ext_vector_type(4))) unsigned u32x4;

static constexpr int mdf_lds_bytes(int KR) { return (3 * KR + 2 * MF_T) * MF_P * (int)sizeof(float); }

// KR: factor rows staged (16, 32, 64, 128; those from k on as zeros).  part [S][2][KR][ncols_pad], numerator then denominator
// partials.  A's columns are 16-byte aligned and lda is a multiple of 16 bytes (the launcher checks), so a row group that starts
// below m ends inside its column.
template <int EBYTES, int KR, int MODE>
__global__ __launch_bounds__(256) void masked_dense_f32_kernel(const unsigned char* __restrict__ A, i64 lda_bytes, i64 m, i64 n,
                                                               const float* __restrict__ R, const float* __restrict__ X, int k, i64 row_tiles,
                                                               i64 tiles_per_span, int S, i64 ncols_pad, float* __restrict__ part)
{
    constexpr int NQ = KR / 4, NU = KR / 16;
    constexpr int V = 16 / EBYTES;                        // rows of the matrix per 16-byte load: 4 / 8
    constexpr int G = MF_T / V;                           // row groups per column: 16 / 8
    constexpr int NP = MF_T * G / 256;                    // loads per lane and tile: 4 / 2
    constexpr int CPP = 256 / G;                          // columns per pass: 16 / 32
    extern __shared__ __attribute__((aligned(16))) unsigned char mf_lds[];
    float* Xs = (float*)mf_lds;                           // [KR][MF_P]: X of the tile's columns, staged once per span
    float* Rs = Xs + KR * MF_P;                           // [2][KR][MF_P]: R of the tile's rows
    unsigned* As = (unsigned*)(Rs + 2 * KR * MF_P);       // [2][64 columns][MF_P]: the tile as fp32 bits
    const i64 bid = blockIdx.x;
    const i64 ct = bid / S;
    const int sp = (int)(bid % S);
    const i64 rt0 = (i64)sp * tiles_per_span;
    i64 rt1 = rt0 + tiles_per_span;
    if (rt1 > row_tiles) rt1 = row_tiles;
    const i64 c0 = ct * MF_T;
    const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6), l15 = lane & 15, l4 = lane >> 4;
    f32x4 nacc[NU], dacc[NU];
#pragma unroll
    for (int u = 0; u < NU; ++u) nacc[u] = dacc[u] = f32x4{0.f, 0.f, 0.f, 0.f};
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
        const i64 r0 = rt * MF_T;
        const i64 g0 = r0 + V * ag;
        const unsigned char* a0 = A + (g0 < last_group ? g0 : last_group) * EBYTES;
#pragma unroll
        for (int p = 0; p < NP; ++p) av[p] = __builtin_nontemporal_load((const u32x4*)(a0 + acol[p]));
        const i64 r = r0 + sr;
        const float* row = R + (r < m ? r : m - 1) * KR + sf;
#pragma unroll
        for (int j = 0; j < NU; ++j) rv[j] = *(const f32x4*)(row + 16 * j);
    };
    // registers -> the tile buffer b: rows >= m and columns >= n become NaN (a clamped row group lies wholly past m), factor rows
    // >= k and slab rows >= m zeros
    auto stage = [&](i64 rt, int b) {
        const i64 r0 = rt * MF_T;
        unsigned* Ab = As + b * MF_T * MF_P;
        float* Rb = Rs + b * KR * MF_P;
#pragma unroll
        for (int p = 0; p < NP; ++p) {
            const bool col_in = c0 + ac + CPP * p < n;
            unsigned w[V];
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                const unsigned x = av[p][e];
                if constexpr (EBYTES == 4) {
                    w[e] = x;
                } else {
                    w[2 * e] = x << 16;                   // 0x7FC0 -> 0x7FC00000
                    w[2 * e + 1] = x & 0xFFFF0000u;
                }
            }
#pragma unroll
            for (int e = 0; e < V; ++e) w[e] = (col_in && r0 + V * ag + e < m) ? w[e] : MF_NAN;
#pragma unroll
            for (int h = 0; h < V / 4; ++h)
                *(u32x4*)(Ab + (ac + CPP * p) * MF_P + V * ag + 4 * h) = u32x4{w[4 * h], w[4 * h + 1], w[4 * h + 2], w[4 * h + 3]};
        }
        // R's rows >= k are zeros in memory (every kernel that writes a factor writes them so) and meet zeros of Xs: one mask, the
        // row's, instead of KR / 4 per lane held across the loop
        const bool row_in = r0 + sr < m;
#pragma unroll
        for (int j = 0; j < NU; ++j)
#pragma unroll
            for (int e = 0; e < 4; ++e) Rb[(16 * j + sf + e) * MF_P + sr] = row_in ? rv[j][e] : 0.f;
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
                for (int e = 0; e < 4; ++e) Xs[(16 * j + sf + e) * MF_P + sr] = (c < n && 16 * j + sf + e < k) ? xv[j][e] : 0.f;
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
            const unsigned* Ab = As + cur * MF_T * MF_P;
            const float* Rb = Rs + cur * KR * MF_P;
            f32x4 acc[4];
#pragma unroll
            for (int t = 0; t < 4; ++t) acc[t] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
            for (int q = 0; q < NQ; ++q) {
                const int kk = 16 * (q >> 2) + 4 * l4 + (q & 3);          // the permuted contraction index, the same for both operands
                const float b = Xs[kk * MF_P + 16 * wave + l15];
#pragma unroll
                for (int t = 0; t < 4; ++t) acc[t] = __builtin_amdgcn_mfma_f32_16x16x4f32(Rb[kk * MF_P + 16 * t + l15], b, acc[t], 0, 0, 0);
            }
#pragma unroll
            for (int t = 0; t < 4; ++t) {
                // rows 16 t + 4 l4 + {0 .. 3} of column 16 wave + l15: the rows of this lane's four result registers
                const u32x4 a4 = *(const u32x4*)(Ab + (16 * wave + l15) * MF_P + 16 * t + 4 * l4);
                f32x4 qn, qd;
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    const unsigned bits = a4[r];          // (a copy: the bits of the scalar, not of the vector's element)
                    const bool meas = (bits & 0x7FFFFFFFu) <= 0x7F800000u;
                    const float a = meas ? __uint_as_float(bits) : 0.f;       // from here on no NaN is in any arithmetic
                    const float d = acc[t][r];
                    float vn, vd;
                    if constexpr (MODE == MF_FRO) {
                        vn = a;
                        vd = d;
                    } else {
                        const float dc = d < MF_EPS ? MF_EPS : d;
                        if constexpr (MODE == MF_KL) {
                            vn = a / dc;
                            vd = 1.f;
                        } else {
                            const float rc = 1.f / dc;
                            vn = __fmul_rn(__fmul_rn(rc, rc), a);
                            vd = rc;
                        }
                    }
                    qn[r] = meas ? vn : 0.f;
                    qd[r] = meas ? vd : 0.f;
                }
#pragma unroll
                for (int u = 0; u < NU; ++u) {
                    const f32x4 r4 = *(const f32x4*)(Rb + (16 * u + l15) * MF_P + 16 * t + 4 * l4);
#pragma unroll
                    for (int r = 0; r < 4; ++r) {
                        nacc[u] = __builtin_amdgcn_mfma_f32_16x16x4f32(r4[r], qn[r], nacc[u], 0, 0, 0);
                        dacc[u] = __builtin_amdgcn_mfma_f32_16x16x4f32(r4[r], qd[r], dacc[u], 0, 0, 0);
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
            part[(((i64)sp * 2) * KR + t) * ncols_pad + col] = nacc[u][r];
            part[(((i64)sp * 2 + 1) * KR + t) * ncols_pad + col] = dacc[u][r];
        }
}

// the spans of a (factor row, column) in span order in fp64, the update in fp64 (kl_dev.h), one rounding: to the fp32 factor X
// (pitch KR) and to its exact widening X64 (pitch KP).  Rows >= k are written as zeros.  A column without a measured entry has
// num = den = 0: den becomes EPS in beta_update and the column goes to 0.  gmode 1: the square root of beta = 0
__global__ __launch_bounds__(256) void masked_dense_f32_finish_kernel(const float* __restrict__ part, int S, int KR, i64 ncols_pad, i64 n,
                                                                      float* __restrict__ X, double* __restrict__ X64, int KP, int k, double l1,
                                                                      double l2, int gmode, int flush)
{
    const i64 j = (i64)blockIdx.x * 64 + (threadIdx.x & 63);
    if (j >= n) return;
    for (int t = threadIdx.x >> 6; t < KR; t += 4) {
        float xn = 0.f;
        if (t < k) {
            double num = 0.0, den = 0.0;
            for (int s = 0; s < S; ++s) {
                num += (double)part[(((i64)s * 2) * KR + t) * ncols_pad + j];
                den += (double)part[(((i64)s * 2 + 1) * KR + t) * ncols_pad + j];
            }
            xn = (float)beta_update((double)X[j * KR + t], num, den, l1, l2, gmode, 0.5, flush);
        }
        X[j * KR + t] = xn;
        if (t < KP) X64[j * KP + t] = (double)xn;
    }
}

// ---- launchers ---------------------------------------------------------------------------------------------------------
size_t masked_dense_f32_scratch_bytes(i64 rows, i64 cols, int k, int num_cus)
{
    i64 rt, ctl, per; int S;
    residual_dense_shape(rows, cols, num_cus, &rt, &ctl, &per, &S);
    return (size_t)2 * S * beta_dense_f32_pitch(k) * ctl * MF_T * sizeof(float);
}

template <int EBYTES, int KR, int MODE>
static int mdf_launch(unsigned grid, const unsigned char* A, i64 lda_bytes, i64 m, i64 n, const float* R, const float* X, int k, i64 rt, i64 per,
                      int S, i64 ncols_pad, float* part, hipStream_t st)
{
    constexpr int lds = mdf_lds_bytes(KR);
    if constexpr (lds > 64 * 1024) {
        static std::atomic<unsigned long long> attr_set{0};       // per device (DeviceOnce)
        if (DeviceOnce once{attr_set}) {
            SMK_HIP(hipFuncSetAttribute((const void*)masked_dense_f32_kernel<EBYTES, KR, MODE>, hipFuncAttributeMaxDynamicSharedMemorySize, lds));
            once.done();
        }
    }
    masked_dense_f32_kernel<EBYTES, KR, MODE><<<grid, 256, lds, st>>>(A, lda_bytes, m, n, R, X, k, rt, per, S, ncols_pad, part);
    return 0;
}

template <int MODE>
static int mdf_step(const void* A, int storage, i64 ld, i64 rows, i64 cols, const float* R, float* X, double* X64, int k, double l1, double l2, int flush,
                    float* part, int num_cus, hipStream_t st)
{
    i64 rt, ctl, per; int S;
    residual_dense_shape(rows, cols, num_cus, &rt, &ctl, &per, &S);
    const i64 ncols_pad = ctl * MF_T;
    if (ctl * S > 0x7FFFFFFFll) { set_error("masked_dense_f32: matrix too wide for one launch"); return -100; }
    const int eb = storage == STORE_BF16 ? 2 : 4;
    // the 16-byte loads: whole row groups inside every column
    if (((uintptr_t)A & 15) || (ld * eb) % 16 || ld < rows) { set_error("masked_dense_f32: the stored matrix is not 16-byte aligned column by column"); return -3; }
    const unsigned grid = (unsigned)(ctl * S);
    const int KR = beta_dense_f32_pitch(k);
    int rc = 0;
#define SMK_MF(EB, KRV) rc = mdf_launch<EB, KRV, MODE>(grid, (const unsigned char*)A, ld * EB, rows, cols, R, X, k, rt, per, S, ncols_pad, part, st)
#define SMK_MF_KR(EB)                                  \
    switch (KR) {                                      \
        case 16: SMK_MF(EB, 16); break;                \
        case 32: SMK_MF(EB, 32); break;                \
        case 64: SMK_MF(EB, 64); break;                \
        default: SMK_MF(EB, 128); break;               \
    }
    if (eb == 2) { SMK_MF_KR(2) } else { SMK_MF_KR(4) }
#undef SMK_MF_KR
#undef SMK_MF
    if (rc) return rc;
    SMK_HIP(hipGetLastError());
    masked_dense_f32_finish_kernel<<<(unsigned)((cols + 63) / 64), 256, 0, st>>>(part, S, KR, ncols_pad, cols, X, X64, kp_of(k), k, l1, l2,
                                                                                MODE == MF_IS ? 1 : 0, flush);
    SMK_HIP(hipGetLastError());
    return 0;
}

int launch_masked_dense_f32_step(const void* A, int storage, i64 ld, i64 rows, i64 cols, const float* R, float* X, double* X64, int k, int beta,
                                 double l1, double l2, int flush, float* scratch, int num_cus, hipStream_t st)
{
    if (k < 1 || k > 128 || rows < 1 || cols < 1 || beta < 0 || beta > 2) {
        set_error("launch_masked_dense_f32_step: k in [1, 128], a matrix with entries and beta 0, 1 or 2");
        return -3;
    }
    if (beta == MF_FRO) return mdf_step<MF_FRO>(A, storage, ld, rows, cols, R, X, X64, k, l1, l2, flush, scratch, num_cus, st);
    if (beta == MF_KL) return mdf_step<MF_KL>(A, storage, ld, rows, cols, R, X, X64, k, l1, l2, flush, scratch, num_cus, st);
    return mdf_step<MF_IS>(A, storage, ld, rows, cols, R, X, X64, k, l1, l2, flush, scratch, num_cus, st);
}

}  // namespace smk
