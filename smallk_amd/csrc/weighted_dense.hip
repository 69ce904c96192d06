// smallk_amd/csrc/weighted_dense.hip -- the kernels of WEIGHTED masked beta-divergence NMF on a dense stored matrix (weighted_dense.cpp,
// DESIGN.md 26): masked_dense_f32.hip's fp32 half-iteration and masked_dense.hip's fp64 divergence with a per-entry weight w >= 0 from
// a second stored matrix V of A's shape, leading dimension and storage.  Per MEASURED entry (i, j, a), d = r_i . x_j, qn and qd as in
// masked_dense_f32.hip (a, d; a / max(d, EPS), 1; (r r) a, r with r = 1 / max(d, EPS)):
//     num_j += (w qn) r_i,   den_j += (w qd) r_i
// qn and qd are formed exactly as there -- the NaN of A selected away on the bits before any arithmetic -- and only then each is
// multiplied by w in fp32, one rounding; an entry with w = 0 is SELECTED to +0 like an unmeasured one (0 times an overflowed
// quotient would be a NaN).  With every weight 1 the products are exact and the step is masked_dense_f32_kernel's bit for bit;
// a weight matrix scaled by a power of two scales both sums exactly.
//
// The step keeps masked_dense_f32_kernel's frame -- read its comments and beta_dense_f32_kernel's: 64 x 64 tiles over spans, 256
// lanes, X's slab once per span, R's slab and the tile of A twice in LDS at pitch 68, the next tile stored while the loads of the one
// after it are in flight, ONE barrier per tile, 16-byte unconditional clamped loads, the permuted contraction index, one ds_read_b128
// of R's slab per eight matrix instructions, partials [S][2][KR][ncols_pad].  What is new is the second stream, and it takes no LDS
// of its own at any KR, so LDS (and with it the workgroups per CU) stays masked_dense_f32_kernel's -- a second double-buffered fp32
// tile (34 816 B) would cost a workgroup per CU at KR = 16 and 32 and overflow the 160 KiB at KR = 128.  One arrangement per STORAGE,
// the same at every KR:
//   * bf16 storage: the tile of A in LDS is fp32 BITS whose low halves are zero after the widening shift.  The weight's 16 bits go
//     there: word = (a << 16) | w.  The weight tile is loaded at the same offsets as the data tile by the same lanes (one offset
//     computation, two base pointers), packed while staging, and comes out of the one ds_read_b128 that brings the data: a's bits
//     are word & 0xFFFF0000, w's are word << 16.  Padding is staged as 0x7FC00000: a missing a with weight 0;
//   * fp32 storage: the four rows 16 t + 4 (lane >> 4) .. + 3 of column 16 wave + (lane & 15) that a lane's four result registers
//     of row block t stand for are 16 contiguous bytes of a column of V.  The lane loads them straight from global memory into
//     registers (four 16-byte loads per tile, the count of the data tile's) one tile ahead -- issued before the matrix
//     instructions of the current tile, consumed after the next barrier -- so the weight tile reaches the accumulator's layout
//     element for element without LDS.  Rows >= m and columns >= n are clamped addresses and become 0.f.
// Fixed summation orders, no atomics: the same bits on every run.
#include <algorithm>
#include <string>

#include "common.h"
#include "devutil.h"
#include "kl_dev.h"

namespace smk {

static constexpr int WD_T = 64;               // rows and columns of a tile
static constexpr int WD_P = 68;               // floats per factor row of a slab and per column of the matrix tile in LDS
static constexpr int WD_FP = 65;              // doubles per factor row of a slab in LDS (the divergence)
static constexpr int WD_IS = 0, WD_KL = 1, WD_FRO = 2;        // the mode is beta itself
static constexpr unsigned WD_NAN = 0x7FC00000u;               // the canonical quiet NaN: what padding of A is staged as
static constexpr float WD_EPS = 1.1920928955078125e-07f;      // KL_EPS, exact in fp32
static constexpr int WD_NS = 5;               // sums of the divergence: s1, s2, s3, the count, the sum of the weights

typedef __attribute__((ext_vector_type(4))) float f32x4;
typedef __attribute__((ext_vector_type(4))) unsigned u32x4;

static constexpr int wd_lds_bytes(int KR) { return (3 * KR + 2 * WD_T) * WD_P * (int)sizeof(float); }

__device__ __forceinline__ bool wd_measured(unsigned bits) { return (bits & 0x7FFFFFFFu) <= 0x7F800000u; }

// KR: factor rows staged (16, 32, 64, 128; those from k on as zeros).  part [S][2][KR][ncols_pad], numerator then denominator
// partials.  The columns of A and of V are 16-byte aligned and lda is a multiple of 16 bytes (the launcher checks), so a row group
// that starts below m ends inside its column.
template <int EBYTES, int KR, int MODE>
__global__ __launch_bounds__(256) void weighted_dense_kernel(const unsigned char* __restrict__ A, const unsigned char* __restrict__ Vw,
                                                             i64 lda_bytes, i64 m, i64 n, const float* __restrict__ R,
                                                             const float* __restrict__ X, int k, i64 row_tiles, i64 tiles_per_span, int S,
                                                             i64 ncols_pad, float* __restrict__ part)
{
    constexpr int NQ = KR / 4, NU = KR / 16;
    constexpr int V = 16 / EBYTES;                        // rows of the matrix per 16-byte load: 4 / 8
    constexpr int G = WD_T / V;                           // row groups per column: 16 / 8
    constexpr int NP = WD_T * G / 256;                    // loads per lane and tile: 4 / 2
    constexpr int CPP = 256 / G;                          // columns per pass: 16 / 32
    constexpr bool PACKED = EBYTES == 2;                  // the weight rides in the low halves of the tile's words
    extern __shared__ __attribute__((aligned(16))) unsigned char wd_lds[];
    float* Xs = (float*)wd_lds;                           // [KR][WD_P]: X of the tile's columns, staged once per span
    float* Rs = Xs + KR * WD_P;                           // [2][KR][WD_P]: R of the tile's rows
    unsigned* As = (unsigned*)(Rs + 2 * KR * WD_P);       // [2][64 columns][WD_P]: the tile as fp32 bits (bf16: data and weight halves)
    const i64 bid = blockIdx.x;
    const i64 ct = bid / S;
    const int sp = (int)(bid % S);
    const i64 rt0 = (i64)sp * tiles_per_span;
    i64 rt1 = rt0 + tiles_per_span;
    if (rt1 > row_tiles) rt1 = row_tiles;
    const i64 c0 = ct * WD_T;
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
    // fp32 storage: the lane's own column of V and whether it exists; its row groups are 4 rows each
    const i64 wc = c0 + 16 * wave + l15;
    const bool wcol_in = wc < n;
    const unsigned char* wcolp = Vw + (wcol_in ? wc : n - 1) * lda_bytes;
    const i64 wlast = (m - 1) / 4 * 4;
    // a slab: a wave takes 16 rows (columns, for X), lane (r = lane >> 2, f = lane & 3) the factor rows 16 j + 4 f .. + 3 of row r
    const int sr = 16 * wave + (lane >> 2), sf = 4 * (lane & 3);
    u32x4 av[NP], wv[PACKED ? NP : 1];
    f32x4 rv[NU];
    f32x4 wnext[PACKED ? 1 : 4];                          // fp32 storage: the weights of the tile that is multiplied next
    auto fetch = [&](i64 rt) {
        const i64 r0 = rt * WD_T;
        const i64 g0 = r0 + V * ag;
        const i64 off = (g0 < last_group ? g0 : last_group) * EBYTES;          // one offset, two base pointers
#pragma unroll
        for (int p = 0; p < NP; ++p) {
            av[p] = __builtin_nontemporal_load((const u32x4*)(A + off + acol[p]));
            if constexpr (PACKED) wv[p] = __builtin_nontemporal_load((const u32x4*)(Vw + off + acol[p]));
        }
        const i64 r = r0 + sr;
        const float* row = R + (r < m ? r : m - 1) * KR + sf;
#pragma unroll
        for (int j = 0; j < NU; ++j) rv[j] = *(const f32x4*)(row + 16 * j);
    };
    // fp32 storage: rows 16 t + 4 l4 .. + 3 of the lane's column of tile rt, outside the matrix 0.f
    auto wfetch = [&](i64 rt) {
        if constexpr (!PACKED) {
            const i64 r0 = rt * WD_T;
#pragma unroll
            for (int t = 0; t < 4; ++t) {
                const i64 g = r0 + 16 * t + 4 * l4;
                const f32x4 w4 = __builtin_nontemporal_load((const f32x4*)(wcolp + (g < wlast ? g : wlast) * 4));
#pragma unroll
                for (int r = 0; r < 4; ++r) wnext[t][r] = (wcol_in && g + r < m) ? w4[r] : 0.f;
            }
        }
    };
    // registers -> the tile buffer b: rows >= m and columns >= n become NaN with weight 0 (a clamped row group lies wholly past m),
    // factor rows >= k and slab rows >= m zeros
    auto stage = [&](i64 rt, int b) {
        const i64 r0 = rt * WD_T;
        unsigned* Ab = As + b * WD_T * WD_P;
        float* Rb = Rs + b * KR * WD_P;
#pragma unroll
        for (int p = 0; p < NP; ++p) {
            const bool col_in = c0 + ac + CPP * p < n;
            unsigned w[V];
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                const unsigned x = av[p][e];
                if constexpr (!PACKED) {
                    w[e] = x;
                } else {
                    const unsigned y = wv[p][e];
                    w[2 * e] = (x << 16) | (y & 0xFFFFu);                 // 0x7FC0 -> 0x7FC0 in the high half
                    w[2 * e + 1] = (x & 0xFFFF0000u) | (y >> 16);
                }
            }
#pragma unroll
            for (int e = 0; e < V; ++e) w[e] = (col_in && r0 + V * ag + e < m) ? w[e] : WD_NAN;
#pragma unroll
            for (int h = 0; h < V / 4; ++h)
                *(u32x4*)(Ab + (ac + CPP * p) * WD_P + V * ag + 4 * h) = u32x4{w[4 * h], w[4 * h + 1], w[4 * h + 2], w[4 * h + 3]};
        }
        // R's rows >= k are zeros in memory and meet zeros of Xs: one mask, the row's (masked_dense_f32_kernel)
        const bool row_in = r0 + sr < m;
#pragma unroll
        for (int j = 0; j < NU; ++j)
#pragma unroll
            for (int e = 0; e < 4; ++e) Rb[(16 * j + sf + e) * WD_P + sr] = row_in ? rv[j][e] : 0.f;
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
                for (int e = 0; e < 4; ++e) Xs[(16 * j + sf + e) * WD_P + sr] = (c < n && 16 * j + sf + e < k) ? xv[j][e] : 0.f;
        }
        fetch(rt0);
        stage(rt0, 0);
        wfetch(rt0);
        fetch(rt0 + 1 < rt1 ? rt0 + 1 : rt1 - 1);
        __syncthreads();
        int cur = 0;
        for (i64 rt = rt0; rt < rt1; ++rt, cur ^= 1) {
            // the next tile into the other buffer (its readers finished before the last barrier), the loads of the one after it,
            // then the matrix cores on this one.  Past the span's end the last tile is staged again and nobody reads it.
            const i64 nx = rt + 1 < rt1 ? rt + 1 : rt1 - 1;
            stage(nx, cur ^ 1);
            fetch(rt + 2 < rt1 ? rt + 2 : rt1 - 1);
            f32x4 wcur[PACKED ? 1 : 4];                   // this tile's weights leave wnext before the next tile's loads are issued
            if constexpr (!PACKED) {
#pragma unroll
                for (int t = 0; t < 4; ++t) wcur[t] = wnext[t];
            }
            wfetch(nx);
            const unsigned* Ab = As + cur * WD_T * WD_P;
            const float* Rb = Rs + cur * KR * WD_P;
            f32x4 acc[4];
#pragma unroll
            for (int t = 0; t < 4; ++t) acc[t] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
            for (int q = 0; q < NQ; ++q) {
                const int kk = 16 * (q >> 2) + 4 * l4 + (q & 3);          // the permuted contraction index, the same for both operands
                const float b = Xs[kk * WD_P + 16 * wave + l15];
#pragma unroll
                for (int t = 0; t < 4; ++t) acc[t] = __builtin_amdgcn_mfma_f32_16x16x4f32(Rb[kk * WD_P + 16 * t + l15], b, acc[t], 0, 0, 0);
            }
#pragma unroll
            for (int t = 0; t < 4; ++t) {
                // rows 16 t + 4 l4 + {0 .. 3} of column 16 wave + l15: the rows of this lane's four result registers
                const u32x4 a4 = *(const u32x4*)(Ab + (16 * wave + l15) * WD_P + 16 * t + 4 * l4);
                f32x4 qn, qd;
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    const unsigned word = a4[r];          // (a copy: the bits of the scalar, not of the vector's element)
                    const unsigned bits = PACKED ? word & 0xFFFF0000u : word;
                    float w;
                    if constexpr (PACKED) w = __uint_as_float(word << 16);
                    else w = wcur[t][r];
                    const bool meas = wd_measured(bits);
                    const float a = meas ? __uint_as_float(bits) : 0.f;       // from here on no NaN is in any arithmetic
                    const float d = acc[t][r];
                    float vn, vd;
                    if constexpr (MODE == WD_FRO) {
                        vn = a;
                        vd = d;
                    } else {
                        const float dc = d < WD_EPS ? WD_EPS : d;
                        if constexpr (MODE == WD_KL) {
                            vn = a / dc;
                            vd = 1.f;
                        } else {
                            const float rc = 1.f / dc;
                            vn = __fmul_rn(__fmul_rn(rc, rc), a);
                            vd = rc;
                        }
                    }
                    const bool use = meas && w > 0.f;     // weight 0 removes the entry as a NaN does: both terms +0
                    qn[r] = use ? __fmul_rn(vn, w) : 0.f;
                    qd[r] = use ? __fmul_rn(vd, w) : 0.f;
                }
#pragma unroll
                for (int u = 0; u < NU; ++u) {
                    const f32x4 r4 = *(const f32x4*)(Rb + (16 * u + l15) * WD_P + 16 * t + 4 * l4);
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

// masked_dense_f32_finish_kernel's arithmetic: the spans of a (factor row, column) in span order in fp64, beta_update in fp64
// (kl_dev.h), one rounding: to the fp32 factor X (pitch KR) and to its exact widening X64 (pitch KP).  Rows >= k are written as
// zeros.  A column whose entries are all unmeasured or of weight 0 has num = den = 0 and goes to 0 through the 0 -> EPS rule
__global__ __launch_bounds__(256) void weighted_dense_finish_kernel(const float* __restrict__ part, int S, int KR, i64 ncols_pad, i64 n,
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

// ---- the weighted divergence: masked_dense_kernel's DIV pass (fp64 matrix cores, one tile buffer, its row map D[row = 4 reg +
// (lane >> 4)]) with the weight in every term and the sum of the weights beside the count.  part [WD_NS][S][ncols_pad]:
//   WD_FRO: sum w (a - d)^2, sum w a^2, nothing;
//   WD_KL:  sum w a log(a / d) over a > EPS (d clamped), sum w a, sum w d (d as it is);
//   WD_IS:  sum w a / d, sum w log(a / d) over a > EPS (d clamped), nothing;
// then the number of measured entries and the sum of their weights.  The tile of A goes through LDS as there.  The weight does not:
// LDS is (KS + KR) 65 8 + 17 408 bytes = 150 528 at k > 64, and a second tile would pass 160 KiB.  A lane loads the sixteen weights of
// its own result registers (row 16 t + 4 r + (lane >> 4) of column 16 wave + (lane & 15)) from global memory one tile ahead.  With
// every weight 1 each term and the sum of the weights are the masked pass's bit for bit.
template <int EBYTES, int NQ, int MODE>
__global__ __launch_bounds__(256) void weighted_dense_div_kernel(const unsigned char* __restrict__ A, const unsigned char* __restrict__ Vw,
                                                                 i64 lda_bytes, i64 m, i64 n, const double* __restrict__ R,
                                                                 const double* __restrict__ X, int ldf, int k, i64 row_tiles,
                                                                 i64 tiles_per_span, int S, i64 ncols_pad, double* __restrict__ part)
{
    constexpr int KR = 4 * NQ;
    constexpr int KS = KR < 16 ? 16 : KR;
    constexpr int NG = (KR + WD_T - 1) / WD_T;
    extern __shared__ __attribute__((aligned(16))) unsigned char wd_lds[];
    double* Rs = (double*)wd_lds;                         // [KS][WD_FP]: R of the tile's rows
    double* Xs = Rs + KS * WD_FP;                         // [KR][WD_FP]: X of the tile's columns
    float* As = (float*)(Xs + KR * WD_FP);                // [64 columns][WD_P]
    const i64 bid = blockIdx.x;
    const i64 ct = bid / S;
    const int sp = (int)(bid % S);
    const i64 rt0 = (i64)sp * tiles_per_span;
    i64 rt1 = rt0 + tiles_per_span;
    if (rt1 > row_tiles) rt1 = row_tiles;
    const i64 c0 = ct * WD_T;
    const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6), l15 = lane & 15, l4 = lane >> 4;
    typedef __attribute__((ext_vector_type(4))) double f64x4;
    f64x4 acc[4];
    double s1 = 0.0, s2 = 0.0, s3 = 0.0, cnt = 0.0, sw = 0.0;
    float bv[16], wn[16];
    double rv[NG][16];
    int kc[NG];
#pragma unroll
    for (int g = 0; g < NG; ++g) kc[g] = 64 * g + lane < k ? 64 * g + lane : k - 1;
    const i64 wc = c0 + 16 * wave + l15;
    const bool wcol_in = wc < n;
    const unsigned char* wcolp = Vw + (wcol_in ? wc : n - 1) * lda_bytes;
    auto fetch = [&](i64 rt) {
        const i64 r0 = rt * WD_T;
        const bool row_in = r0 + lane < m;
        const i64 rl = row_in ? r0 + lane : m - 1;
#pragma unroll
        for (int i = 0; i < 16; ++i) {
            const i64 c = c0 + 4 * i + wave;
            const unsigned char* col = A + (c < n ? c : n - 1) * lda_bytes;      // scalar
            float v;
            if constexpr (EBYTES == 2) v = bf16_bits_to_f32(__builtin_nontemporal_load((const unsigned short*)col + rl));
            else v = __builtin_nontemporal_load((const float*)col + rl);
            bv[i] = (row_in && c < n) ? v : __builtin_bit_cast(float, WD_NAN);   // outside the matrix: not measured
        }
#pragma unroll
        for (int i = 0; i < 16; ++i) {                    // i = 4 t + r: the weight of acc[t][r]
            const i64 row = r0 + 16 * (i >> 2) + 4 * (i & 3) + l4;
            const i64 rc = row < m ? row : m - 1;
            float v;
            if constexpr (EBYTES == 2) v = bf16_bits_to_f32(__builtin_nontemporal_load((const unsigned short*)wcolp + rc));
            else v = __builtin_nontemporal_load((const float*)wcolp + rc);
            wn[i] = (wcol_in && row < m) ? v : 0.f;
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
            for (int i = 0; i < 16; ++i) Xs[(64 * g + lane) * WD_FP + 4 * i + wave] = (c0 + 4 * i + wave < n && 64 * g + lane < k) ? t[i] : 0.0;
        }
    }
    if (rt0 < rt1) fetch(rt0);
    for (i64 rt = rt0; rt < rt1; ++rt) {
        float wcur[16];
#pragma unroll
        for (int t = 0; t < 4; ++t) acc[t] = f64x4{0.0, 0.0, 0.0, 0.0};
#pragma unroll
        for (int i = 0; i < 16; ++i) {
            wcur[i] = wn[i];
            As[(4 * i + wave) * WD_P + lane] = bv[i];
#pragma unroll
            for (int g = 0; g < NG; ++g)
                if (64 * g + lane < KS) Rs[(64 * g + lane) * WD_FP + 4 * i + wave] = (rt * WD_T + 4 * i + wave < m && 64 * g + lane < k) ? rv[g][i] : 0.0;
        }
        __syncthreads();
        if (rt + 1 < rt1) fetch(rt + 1);
#pragma unroll
        for (int q = 0; q < NQ; ++q) {
            const double b = Xs[(4 * q + l4) * WD_FP + 16 * wave + l15];
#pragma unroll
            for (int t = 0; t < 4; ++t) acc[t] = __builtin_amdgcn_mfma_f64_16x16x4f64(Rs[(4 * q + l4) * WD_FP + 16 * t + l15], b, acc[t], 0, 0, 0);
        }
#pragma unroll
        for (int t = 0; t < 4; ++t)
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const float af = As[(16 * wave + l15) * WD_P + 16 * t + l4 + 4 * r];
                const bool meas = wd_measured(__builtin_bit_cast(unsigned, af));
                const double av = meas ? (double)af : 0.0;            // from here on no NaN is in any arithmetic
                const double w = (double)wcur[4 * t + r];
                const double d = acc[t][r];
                cnt += meas ? 1.0 : 0.0;
                sw += meas ? w : 0.0;
                if constexpr (MODE == WD_FRO) {
                    const double e = meas ? av - d : 0.0;
                    s1 = __builtin_fma(__dmul_rn(w, e), e, s1);
                    s2 = __builtin_fma(__dmul_rn(w, av), av, s2);
                } else {
                    const double dc = d < KL_EPS ? KL_EPS : d;
                    if constexpr (MODE == WD_KL) {
                        const double wa = __dmul_rn(w, av);
                        if (av > KL_EPS) s1 = __builtin_fma(wa, log(av / dc), s1);
                        s2 += wa;
                        s3 += meas ? __dmul_rn(w, d) : 0.0;
                    } else {
                        if (av > KL_EPS) { const double q = av / dc; s1 += __dmul_rn(w, q); s2 += __dmul_rn(w, log(q)); }
                    }
                }
            }
        __syncthreads();
    }
    const i64 col = c0 + 16 * wave + l15;                 // < ncols_pad
    double s[WD_NS] = {s1, s2, s3, cnt, sw};
#pragma unroll
    for (int i = 0; i < WD_NS; ++i) {
        s[i] += __shfl_xor(s[i], 16, 64);
        s[i] += __shfl_xor(s[i], 32, 64);
        if (l4 == 0) part[((i64)i * S + sp) * ncols_pad + col] = s[i];
    }
}

// masked_dense_colsum_kernel with one more sum: the spans of a column in span order; 256 columns per workgroup, whose sums go to
// blockpart in column order (16 sums of 16, then their sum)
__global__ __launch_bounds__(256) void weighted_dense_colsum_kernel(const double* __restrict__ part, int S, i64 ncols_pad, i64 n,
                                                                    double* __restrict__ blockpart)
{
    __shared__ double sh[256][WD_NS];
    const i64 j = (i64)blockIdx.x * 256 + threadIdx.x;
    double v[WD_NS] = {0.0, 0.0, 0.0, 0.0, 0.0};
    if (j < n)
        for (int q = 0; q < S; ++q)
            for (int i = 0; i < WD_NS; ++i) v[i] += part[((i64)i * S + q) * ncols_pad + j];
    for (int i = 0; i < WD_NS; ++i) sh[threadIdx.x][i] = v[i];
    __syncthreads();
    double w[WD_NS] = {0.0, 0.0, 0.0, 0.0, 0.0};
    if (threadIdx.x < 16)
        for (int e = 0; e < 16; ++e)
            for (int i = 0; i < WD_NS; ++i) w[i] += sh[16 * threadIdx.x + e][i];
    __syncthreads();
    if (threadIdx.x < 16)
        for (int i = 0; i < WD_NS; ++i) sh[threadIdx.x][i] = w[i];
    __syncthreads();
    if (threadIdx.x == 0)
        for (int i = 0; i < WD_NS; ++i) {
            double t = 0.0;
            for (int e = 0; e < 16; ++e) t += sh[e][i];
            blockpart[WD_NS * (i64)blockIdx.x + i] = t;
        }
}

// masked_dense_total_kernel with one more sum: the workgroups' sums in its order, then D over the measured entries:
// out = {D, s1, s2, s3, count, sum w} with D = s1 / 2 (WD_FRO), (s1 - s2) + s3 (WD_KL), (s1 - sum w) - s2 (WD_IS).  host_out: pinned or null
__global__ __launch_bounds__(1024) void weighted_dense_total_kernel(const double* __restrict__ blockpart, i64 nblk, int mode,
                                                                    double* __restrict__ out, double* host_out)
{
    __shared__ double sh[1024][WD_NS];
    double v[WD_NS] = {0.0, 0.0, 0.0, 0.0, 0.0};
    for (i64 b = threadIdx.x; b < nblk; b += 1024)
        for (int i = 0; i < WD_NS; ++i) v[i] += blockpart[WD_NS * b + i];
    for (int i = 0; i < WD_NS; ++i) sh[threadIdx.x][i] = v[i];
    __syncthreads();
    for (int w = 512; w > 0; w >>= 1) {
        if ((int)threadIdx.x < w)
            for (int i = 0; i < WD_NS; ++i) sh[threadIdx.x][i] += sh[threadIdx.x + w][i];
        __syncthreads();
    }
    if (threadIdx.x == 0) {
        const double a = sh[0][0], b = sh[0][1], c = sh[0][2], cnt = sh[0][3], sw = sh[0][4];
        const double D = mode == WD_FRO ? 0.5 * a : mode == WD_KL ? (a - b) + c : (a - sw) - b;
        const double r6[6] = {D, a, b, c, cnt, sw};
        for (int i = 0; i < 6; ++i) {
            out[i] = r6[i];
            if (host_out) host_out[i] = r6[i];
        }
    }
}

// what V is: bit 0 of *flag a weight that is negative, NaN or infinite (measured or not), bit 1 a measured entry of A with a
// positive weight.  masked_dense_look_kernel's walk; only rows < m and columns < n are read
template <int EBYTES>
__global__ __launch_bounds__(256) void weighted_dense_look_kernel(const unsigned char* __restrict__ A, const unsigned char* __restrict__ Vw,
                                                                  i64 lda_bytes, i64 m, i64 n, int* flag)
{
    int found = 0;
    for (i64 c = blockIdx.x; c < n; c += gridDim.x) {
        const unsigned char *col = A + c * lda_bytes, *wcol = Vw + c * lda_bytes;
        for (i64 r = threadIdx.x; r < m; r += 256) {
            float a, w;
            if constexpr (EBYTES == 2) {
                a = bf16_bits_to_f32(((const unsigned short*)col)[r]);
                w = bf16_bits_to_f32(((const unsigned short*)wcol)[r]);
            } else {
                a = ((const float*)col)[r];
                w = ((const float*)wcol)[r];
            }
            if (!(w >= 0.f) || (__builtin_bit_cast(unsigned, w) & 0x7FFFFFFFu) >= 0x7F800000u) found |= 1;
            else if (w > 0.f && wd_measured(__builtin_bit_cast(unsigned, a))) found |= 2;
        }
    }
    if (found) atomicOr(flag, found);
}

// ---- launchers ---------------------------------------------------------------------------------------------------------
static int wd_div_nq(int k) { return k > 64 ? 32 : k > 32 ? 16 : k > 16 ? 8 : k > 8 ? 4 : k > 4 ? 2 : 1; }

size_t weighted_dense_scratch_bytes(i64 rows, i64 cols, int k, int num_cus)
{
    i64 rt, ctl, per; int S;
    residual_dense_shape(rows, cols, num_cus, &rt, &ctl, &per, &S);
    const size_t step = (size_t)2 * S * beta_dense_f32_pitch(k) * ctl * WD_T * sizeof(float);
    const size_t div = ((size_t)WD_NS * S * ctl * WD_T + (size_t)WD_NS * ((cols + 255) / 256)) * sizeof(double);
    return std::max(step, div);
}

// the two matrices as the kernels read them: whole 16-byte row groups inside every column, at the same offsets in both
static int wd_layout(const char* who, const void* A, const void* V, int eb, i64 ld, i64 rows)
{
    if (!(((uintptr_t)A | (uintptr_t)V) & 15) && (ld * eb) % 16 == 0 && ld >= rows) return 0;
    set_error(std::string(who) + ": the stored matrices are not 16-byte aligned column by column");
    return -3;
}

template <int EBYTES, int KR, int MODE>
static int wd_launch(unsigned grid, const unsigned char* A, const unsigned char* V, i64 lda_bytes, i64 m, i64 n, const float* R, const float* X,
                     int k, i64 rt, i64 per, int S, i64 ncols_pad, float* part, hipStream_t st)
{
    constexpr int lds = wd_lds_bytes(KR);
    if constexpr (lds > 64 * 1024) {
        static std::atomic<unsigned long long> attr_set{0};       // per device (DeviceOnce)
        if (DeviceOnce once{attr_set}) {
            SMK_HIP(hipFuncSetAttribute((const void*)weighted_dense_kernel<EBYTES, KR, MODE>, hipFuncAttributeMaxDynamicSharedMemorySize, lds));
            once.done();
        }
    }
    weighted_dense_kernel<EBYTES, KR, MODE><<<grid, 256, lds, st>>>(A, V, lda_bytes, m, n, R, X, k, rt, per, S, ncols_pad, part);
    return 0;
}

template <int MODE>
static int wd_step(const void* A, const void* V, int storage, i64 ld, i64 rows, i64 cols, const float* R, float* X, double* X64, int k, double l1,
                   double l2, int flush, float* part, int num_cus, hipStream_t st)
{
    i64 rt, ctl, per; int S;
    residual_dense_shape(rows, cols, num_cus, &rt, &ctl, &per, &S);
    const i64 ncols_pad = ctl * WD_T;
    if (ctl * S > 0x7FFFFFFFll) { set_error("weighted_dense: matrix too wide for one launch"); return -100; }
    const int eb = storage == STORE_BF16 ? 2 : 4;
    if (int rc = wd_layout("weighted_dense", A, V, eb, ld, rows)) return rc;
    const unsigned grid = (unsigned)(ctl * S);
    const int KR = beta_dense_f32_pitch(k);
    int rc = 0;
#define SMK_WD(EB, KRV) \
    rc = wd_launch<EB, KRV, MODE>(grid, (const unsigned char*)A, (const unsigned char*)V, ld * EB, rows, cols, R, X, k, rt, per, S, ncols_pad, part, st)
#define SMK_WD_KR(EB)                                  \
    switch (KR) {                                      \
        case 16: SMK_WD(EB, 16); break;                \
        case 32: SMK_WD(EB, 32); break;                \
        case 64: SMK_WD(EB, 64); break;                \
        default: SMK_WD(EB, 128); break;               \
    }
    if (eb == 2) { SMK_WD_KR(2) } else { SMK_WD_KR(4) }
#undef SMK_WD_KR
#undef SMK_WD
    if (rc) return rc;
    SMK_HIP(hipGetLastError());
    weighted_dense_finish_kernel<<<(unsigned)((cols + 63) / 64), 256, 0, st>>>(part, S, KR, ncols_pad, cols, X, X64, kp_of(k), k, l1, l2,
                                                                              MODE == WD_IS ? 1 : 0, flush);
    SMK_HIP(hipGetLastError());
    return 0;
}

static bool wd_args(const char* who, int k, i64 rows, i64 cols, int beta)
{
    if (k >= 1 && k <= 128 && rows >= 1 && cols >= 1 && beta >= 0 && beta <= 2) return true;
    set_error(std::string(who) + ": k in [1, 128], a matrix with entries and beta 0, 1 or 2");
    return false;
}

int launch_weighted_dense_step(const void* A, const void* V, int storage, i64 ld, i64 rows, i64 cols, const float* R, float* X, double* X64, int k,
                               int beta, double l1, double l2, int flush, float* scratch, int num_cus, hipStream_t st)
{
    if (!wd_args("launch_weighted_dense_step", k, rows, cols, beta)) return -3;
    if (beta == WD_FRO) return wd_step<WD_FRO>(A, V, storage, ld, rows, cols, R, X, X64, k, l1, l2, flush, scratch, num_cus, st);
    if (beta == WD_KL) return wd_step<WD_KL>(A, V, storage, ld, rows, cols, R, X, X64, k, l1, l2, flush, scratch, num_cus, st);
    return wd_step<WD_IS>(A, V, storage, ld, rows, cols, R, X, X64, k, l1, l2, flush, scratch, num_cus, st);
}

template <int EBYTES, int NQ, int MODE>
static int wd_div_launch(unsigned grid, const unsigned char* A, const unsigned char* V, i64 lda_bytes, i64 m, i64 n, const double* R, const double* X,
                         int ldf, int k, i64 rt, i64 per, int S, i64 ncols_pad, double* part, hipStream_t st)
{
    constexpr int KR = 4 * NQ, KS = KR < 16 ? 16 : KR;
    constexpr int lds = (KS + KR) * WD_FP * (int)sizeof(double) + WD_T * WD_P * (int)sizeof(float);
    if constexpr (lds > 64 * 1024) {
        static std::atomic<unsigned long long> attr_set{0};       // per device (DeviceOnce)
        if (DeviceOnce once{attr_set}) {
            SMK_HIP(hipFuncSetAttribute((const void*)weighted_dense_div_kernel<EBYTES, NQ, MODE>, hipFuncAttributeMaxDynamicSharedMemorySize, lds));
            once.done();
        }
    }
    weighted_dense_div_kernel<EBYTES, NQ, MODE><<<grid, 256, lds, st>>>(A, V, lda_bytes, m, n, R, X, ldf, k, rt, per, S, ncols_pad, part);
    return 0;
}

template <int MODE>
static int wd_div(const void* A, const void* V, int storage, i64 ld, i64 m, i64 n, const double* R, const double* X, int k, double* part, int num_cus,
                  hipStream_t st, int* S_out, i64* ncols_pad_out)
{
    i64 rt, ctl, per; int S;
    residual_dense_shape(m, n, num_cus, &rt, &ctl, &per, &S);
    const i64 ncols_pad = ctl * WD_T;
    if (ctl * S > 0x7FFFFFFFll) { set_error("weighted_dense: matrix too wide for one launch"); return -100; }
    const unsigned grid = (unsigned)(ctl * S);
    const int ldf = kp_of(k);
    int rc = 0;
#define SMK_WD(EB, NQ) \
    rc = wd_div_launch<EB, NQ, MODE>(grid, (const unsigned char*)A, (const unsigned char*)V, ld * EB, m, n, R, X, ldf, k, rt, per, S, ncols_pad, part, st)
#define SMK_WD_NQ(EB)                                  \
    switch (wd_div_nq(k)) {                            \
        case 1: SMK_WD(EB, 1); break;                  \
        case 2: SMK_WD(EB, 2); break;                  \
        case 4: SMK_WD(EB, 4); break;                  \
        case 8: SMK_WD(EB, 8); break;                  \
        case 16: SMK_WD(EB, 16); break;                \
        default: SMK_WD(EB, 32); break;                \
    }
    if (storage == STORE_BF16) { SMK_WD_NQ(2) } else { SMK_WD_NQ(4) }
#undef SMK_WD_NQ
#undef SMK_WD
    if (rc) return rc;
    SMK_HIP(hipGetLastError());
    *S_out = S;
    *ncols_pad_out = ncols_pad;
    return 0;
}

int launch_weighted_dense_divergence(const void* A, const void* V, int storage, i64 ld, i64 rows, i64 cols, const double* R, const double* X, int k,
                                     int beta, double* scratch, double* out6, double* host_out, int num_cus, hipStream_t st)
{
    if (!wd_args("launch_weighted_dense_divergence", k, rows, cols, beta)) return -3;
    int S = 0;
    i64 ncols_pad = 0;
    int rc;
    if (beta == WD_FRO) rc = wd_div<WD_FRO>(A, V, storage, ld, rows, cols, R, X, k, scratch, num_cus, st, &S, &ncols_pad);
    else if (beta == WD_KL) rc = wd_div<WD_KL>(A, V, storage, ld, rows, cols, R, X, k, scratch, num_cus, st, &S, &ncols_pad);
    else rc = wd_div<WD_IS>(A, V, storage, ld, rows, cols, R, X, k, scratch, num_cus, st, &S, &ncols_pad);
    if (rc) return rc;
    double* blockpart = scratch + (size_t)WD_NS * S * ncols_pad;
    const i64 nblk = (cols + 255) / 256;
    weighted_dense_colsum_kernel<<<(unsigned)nblk, 256, 0, st>>>(scratch, S, ncols_pad, cols, blockpart);
    SMK_HIP(hipGetLastError());
    weighted_dense_total_kernel<<<1, 1024, 0, st>>>(blockpart, nblk, beta, out6, host_out);
    SMK_HIP(hipGetLastError());
    return 0;
}

int launch_weighted_dense_look(const void* A, const void* V, int storage, i64 ld, i64 rows, i64 cols, int* flag, hipStream_t st)
{
    const unsigned grid = (unsigned)std::min<i64>(cols, 4096);
    if (storage == STORE_BF16) weighted_dense_look_kernel<2><<<grid, 256, 0, st>>>((const unsigned char*)A, (const unsigned char*)V, ld * 2, rows, cols, flag);
    else weighted_dense_look_kernel<4><<<grid, 256, 0, st>>>((const unsigned char*)A, (const unsigned char*)V, ld * 4, rows, cols, flag);
    SMK_HIP(hipGetLastError());
    return 0;
}

}  // namespace smk
