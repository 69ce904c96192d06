// smallk_amd/csrc/beta_dense.hip -- the kernels of beta-divergence NMF on a dense stored matrix (beta_dense.cpp):
// scikit-learn's multiplicative update for any beta >= 0 but 1 (kl_dense.hip) and 2 (the Frobenius solvers), Itakura-Saito
// (beta = 0) first.  The frame is kl_dense_kernel's -- read its comments: 64 x 64 tiles, spans, unconditional clamped loads masked
// afterwards, unrolled step loops, its row map D[row = 4 reg + (lane >> 4)] -- and below the matrix is again `m` x `n` as stored,
// R (KP x m) the factor of its rows and X (KP x n) the factor of its columns, the one being updated.  Per entry (i, j, a):
//     d = r_i . x_j,   qn = a dn^(beta - 2),   qd = dd^(beta - 1),   num_j += qn r_i,   den_j += qd r_i
// (dn = max(d, EPS) when beta < 2, dd = max(d, EPS) when beta < 1, else d itself) and per column
//     x_j[t] *= (num_j[t] / den_j[t])^gamma                       (kl_dev.h: beta_update).
// What beta != 1 changes against the KL step: the denominator is no longer a vector of factor row sums but a SECOND chained
// contraction over the same (WH) tile.  After the product, one 16-row block of the tile (4 result registers) at a time becomes the
// pair (qn, qd) and feeds both contractions from the same staged slab of R, whose LDS read is shared: 4 NQ + 2 * 16 NU matrix
// instructions per wave and tile, the matrix read once, no m x n temporary, no shuffle, no LDS round trip for the quotients.
// Rows >= m of the tile carry qd != 0 (beta < 1: EPS^(beta - 1)) but meet zero rows of R's slab; columns >= n are never summed.
// MODE selects how the powers are formed.  BETA_IS (beta = 0): r = 1 / dn, qn = (r r) a, qd = r -- divisions only.  BETA_POW: one
// double-precision pow per entry, p = d^(beta - 2), qn = a p, qd = p d; where d < EPS the clamped side is a constant formed on the
// host (EPS^(beta - 2), EPS^(beta - 1)) and for 1 < beta < 2, where only dn is clamped, the same call forms d^(beta - 1) instead.
// Every sum has a fixed order: the same bits on every run, no floating-point atomics.
#include <algorithm>
#include <cmath>
#include <string>

#include "common.h"
#include "devutil.h"
#include "kl_dev.h"

namespace smk {

static constexpr int BD_T = 64;               // rows and columns of a tile
static constexpr int BD_FP = 65;              // doubles per factor row of a slab in LDS (as KD_FP)
static constexpr int BD_AP = 68;              // floats per column of the matrix tile in LDS (as KD_AP)
static constexpr int BETA_IS = 0, BETA_POW = 1;

// what a launch knows about beta (BETA_IS reads none of it)
struct BetaParams {
    double beta, e1, e2;                      // beta, beta - 1, beta - 2
    double cn, cd;                            // EPS^(beta - 2), EPS^(beta - 1): the clamped powers
    int clamp_n, clamp_d;                     // beta < 2, beta < 1
};

// DIV = false: the step; part [S][2][KS][ncols_pad], numerator then denominator partials.  DIV = true: the same product, then per
// column the sums the divergence is formed from; part [3][S][ncols_pad]:
//   BETA_IS:  sum a / d, sum log(a / d) over the entries with a > EPS (d clamped), nothing;
//   BETA_POW: sum a^beta, sum a d^(beta - 1) over the entries with a > EPS (d clamped), sum d^beta over every entry (d as it is).
template <int EBYTES, int NQ, int MODE, bool DIV>
__global__ __launch_bounds__(256) void beta_dense_kernel(const unsigned char* __restrict__ A, i64 lda_bytes, i64 m, i64 n,
                                                         const double* __restrict__ R, const double* __restrict__ X, int ldf, int k,
                                                         i64 row_tiles, i64 tiles_per_span, int S, i64 ncols_pad, BetaParams bp,
                                                         double* __restrict__ part)
{
    constexpr int KR = 4 * NQ;
    constexpr int KS = KR < 16 ? 16 : KR;
    constexpr int NU = KS / 16;
    constexpr int NG = (KR + BD_T - 1) / BD_T;
    extern __shared__ __attribute__((aligned(16))) unsigned char bd_lds[];
    double* Rs = (double*)bd_lds;                         // [KS][BD_FP]: R of the tile's rows
    double* Xs = Rs + KS * BD_FP;                         // [KR][BD_FP]: X of the tile's columns
    float* As = (float*)(Xs + KR * BD_FP);                // [64 columns][BD_AP]
    const i64 bid = blockIdx.x;
    const i64 ct = bid / S;
    const int sp = (int)(bid % S);
    const i64 rt0 = (i64)sp * tiles_per_span;
    i64 rt1 = rt0 + tiles_per_span;
    if (rt1 > row_tiles) rt1 = row_tiles;
    const i64 c0 = ct * BD_T;
    const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6), l15 = lane & 15, l4 = lane >> 4;
    typedef __attribute__((ext_vector_type(4))) double f64x4;
    f64x4 acc[4];
    f64x4 nacc[DIV ? 1 : NU], dacc[DIV ? 1 : NU];
    double s1 = 0.0, s2 = 0.0, s3 = 0.0;
#pragma unroll
    for (int u = 0; u < (DIV ? 1 : NU); ++u) nacc[u] = dacc[u] = f64x4{0.0, 0.0, 0.0, 0.0};
    float bv[16];
    double rv[NG][16];
    int kc[NG];
#pragma unroll
    for (int g = 0; g < NG; ++g) kc[g] = 64 * g + lane < k ? 64 * g + lane : k - 1;
    auto fetch = [&](i64 rt) {
        const i64 r0 = rt * BD_T;
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
            for (int i = 0; i < 16; ++i) Xs[(64 * g + lane) * BD_FP + 4 * i + wave] = (c0 + 4 * i + wave < n && 64 * g + lane < k) ? t[i] : 0.0;
        }
    }
    if (rt0 < rt1) fetch(rt0);
    for (i64 rt = rt0; rt < rt1; ++rt) {
#pragma unroll
        for (int t = 0; t < 4; ++t) acc[t] = f64x4{0.0, 0.0, 0.0, 0.0};
#pragma unroll
        for (int i = 0; i < 16; ++i) {
            As[(4 * i + wave) * BD_AP + lane] = bv[i];
#pragma unroll
            for (int g = 0; g < NG; ++g)
                if (64 * g + lane < KS) Rs[(64 * g + lane) * BD_FP + 4 * i + wave] = (rt * BD_T + 4 * i + wave < m && 64 * g + lane < k) ? rv[g][i] : 0.0;
        }
        __syncthreads();
        if (rt + 1 < rt1) fetch(rt + 1);
#pragma unroll
        for (int q = 0; q < NQ; ++q) {
            const double b = Xs[(4 * q + l4) * BD_FP + 16 * wave + l15];
#pragma unroll
            for (int t = 0; t < 4; ++t) acc[t] = __builtin_amdgcn_mfma_f64_16x16x4f64(Rs[(4 * q + l4) * BD_FP + 16 * t + l15], b, acc[t], 0, 0, 0);
        }
        if constexpr (DIV && MODE == BETA_POW) {
            // sum a^beta by itself (a loop that stays a loop: one more copy of the power routine, not sixteen)
#pragma unroll 1
            for (int e = 0; e < 16; ++e) {
                const double av = (double)As[(16 * wave + l15) * BD_AP + 4 * e + l4];
                if (av > KL_EPS) s1 += pow(av, bp.beta);
            }
        }
#pragma unroll
        for (int t = 0; t < 4; ++t) {
            f64x4 qn, qd;
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const double av = (double)As[(16 * wave + l15) * BD_AP + 16 * t + l4 + 4 * r];
                const double d = acc[t][r];
                const bool low = d < KL_EPS;
                if constexpr (MODE == BETA_IS) {
                    const double dc = low ? KL_EPS : d;
                    if constexpr (DIV) {
                        if (av > KL_EPS) { const double q = av / dc; s1 += q; s2 += log(q); }
                    } else {
                        const double rc = 1.0 / dc;
                        qn[r] = __dmul_rn(__dmul_rn(rc, rc), av);
                        qd[r] = rc;
                    }
                } else if constexpr (DIV) {
                    // low: the clamped d^(beta - 1) is the constant and the one call forms d^beta; else d^beta = d^(beta - 1) d
                    const double p = pow(d, low ? bp.beta : bp.e1);
                    if (av > KL_EPS) s2 = __builtin_fma(av, low ? bp.cd : p, s2);
                    s3 += low ? p : __dmul_rn(p, d);
                } else {
                    const bool mid = low && bp.clamp_n && !bp.clamp_d;          // 1 < beta < 2 and d < EPS: only dn is clamped
                    const double p = pow(d, mid ? bp.e1 : bp.e2);
                    qn[r] = __dmul_rn(av, (low && bp.clamp_n) ? bp.cn : p);
                    qd[r] = (low && bp.clamp_d) ? bp.cd : mid ? p : __dmul_rn(p, d);
                }
            }
            if constexpr (!DIV) {
#pragma unroll
                for (int r = 0; r < 4; ++r)
#pragma unroll
                    for (int u = 0; u < NU; ++u) {
                        const double a = Rs[(16 * u + l15) * BD_FP + 16 * t + 4 * r + l4];
                        nacc[u] = __builtin_amdgcn_mfma_f64_16x16x4f64(a, qn[r], nacc[u], 0, 0, 0);
                        dacc[u] = __builtin_amdgcn_mfma_f64_16x16x4f64(a, qd[r], dacc[u], 0, 0, 0);
                    }
            }
        }
        __syncthreads();
    }
    const i64 col = c0 + 16 * wave + l15;                 // < ncols_pad
    if constexpr (DIV) {
        s1 += __shfl_xor(s1, 16, 64);
        s1 += __shfl_xor(s1, 32, 64);
        s2 += __shfl_xor(s2, 16, 64);
        s2 += __shfl_xor(s2, 32, 64);
        s3 += __shfl_xor(s3, 16, 64);
        s3 += __shfl_xor(s3, 32, 64);
        if (l4 == 0) {
            part[(i64)sp * ncols_pad + col] = s1;
            part[((i64)S + sp) * ncols_pad + col] = s2;
            part[((i64)2 * S + sp) * ncols_pad + col] = s3;
        }
    } else {
#pragma unroll
        for (int u = 0; u < NU; ++u)
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                part[(((i64)sp * 2) * KS + 16 * u + 4 * r + l4) * ncols_pad + col] = nacc[u][r];
                part[(((i64)sp * 2 + 1) * KS + 16 * u + 4 * r + l4) * ncols_pad + col] = dacc[u][r];
            }
    }
}

// the spans of both partial sets in span order, then the update of X in place (thread map: kl_dense_finish_kernel's)
__global__ __launch_bounds__(256) void beta_dense_finish_kernel(const double* __restrict__ part, int S, int KS, i64 ncols_pad, i64 n,
                                                                double* __restrict__ X, int KP, int k, double l1, double l2, int gmode,
                                                                double gamma, int flush)
{
    const i64 j = (i64)blockIdx.x * 64 + (threadIdx.x & 63);
    if (j >= n) return;
    for (int t = threadIdx.x >> 6; t < KP; t += 4) {
        double xn = 0.0;
        if (t < k) {
            double num = 0.0, den = 0.0;
            for (int s = 0; s < S; ++s) {
                num += part[(((i64)s * 2) * KS + t) * ncols_pad + j];
                den += part[(((i64)s * 2 + 1) * KS + t) * ncols_pad + j];
            }
            xn = beta_update(X[j * KP + t], num, den, l1, l2, gmode, gamma, flush);
        }
        X[j * KP + t] = xn;
    }
}

// the spans of a column in span order; 256 columns per workgroup, whose three sums go to blockpart in column order (the shape of
// kl_dense_colsum_kernel: 16 sums of 16, then their sum)
__global__ __launch_bounds__(256) void beta_dense_colsum_kernel(const double* __restrict__ part, int S, i64 ncols_pad, i64 n,
                                                                double* __restrict__ blockpart)
{
    __shared__ double sh[256][3];
    const i64 j = (i64)blockIdx.x * 256 + threadIdx.x;
    double v[3] = {0.0, 0.0, 0.0};
    if (j < n)
        for (int q = 0; q < S; ++q)
            for (int i = 0; i < 3; ++i) v[i] += part[((i64)i * S + q) * ncols_pad + j];
    for (int i = 0; i < 3; ++i) sh[threadIdx.x][i] = v[i];
    __syncthreads();
    double w[3] = {0.0, 0.0, 0.0};
    if (threadIdx.x < 16)
        for (int e = 0; e < 16; ++e)
            for (int i = 0; i < 3; ++i) w[i] += sh[16 * threadIdx.x + e][i];
    __syncthreads();
    if (threadIdx.x < 16)
        for (int i = 0; i < 3; ++i) sh[threadIdx.x][i] = w[i];
    __syncthreads();
    if (threadIdx.x == 0)
        for (int i = 0; i < 3; ++i) {
            double t = 0.0;
            for (int e = 0; e < 16; ++e) t += sh[e][i];
            blockpart[3 * (i64)blockIdx.x + i] = t;
        }
}

// the workgroups' sums in index order (kl_dense_total_kernel's shape), then D.  is != 0: out = {s1 - count - s2, s1, s2, count};
// else out = {(s1 - beta s2 + (beta - 1) s3) / (beta (beta - 1)), s1, s2, s3}.  host_out: pinned or null
__global__ __launch_bounds__(1024) void beta_dense_total_kernel(const double* __restrict__ blockpart, i64 nblk, int is, double beta, double count,
                                                                double* __restrict__ out, double* host_out)
{
    __shared__ double sh[1024][3];
    double v[3] = {0.0, 0.0, 0.0};
    for (i64 b = threadIdx.x; b < nblk; b += 1024)
        for (int i = 0; i < 3; ++i) v[i] += blockpart[3 * b + i];
    for (int i = 0; i < 3; ++i) sh[threadIdx.x][i] = v[i];
    __syncthreads();
    for (int w = 512; w > 0; w >>= 1) {
        if ((int)threadIdx.x < w)
            for (int i = 0; i < 3; ++i) sh[threadIdx.x][i] += sh[threadIdx.x + w][i];
        __syncthreads();
    }
    if (threadIdx.x == 0) {
        const double a = sh[0][0], b = sh[0][1], c = is ? count : sh[0][2];
        double D;
        if (is) D = (a - c) - b;
        else D = ((a - __dmul_rn(beta, b)) + __dmul_rn(c, beta - 1.0)) / __dmul_rn(beta, beta - 1.0);
        const double r4[4] = {D, a, b, c};
        for (int i = 0; i < 4; ++i) {
            out[i] = r4[i];
            if (host_out) host_out[i] = r4[i];
        }
    }
}

// ---- launchers ---------------------------------------------------------------------------------------------------------
static int beta_dense_nq(int k) { return k > 64 ? 32 : k > 32 ? 16 : k > 16 ? 8 : k > 8 ? 4 : k > 4 ? 2 : 1; }
static int beta_dense_ks(int k) { const int kr = 4 * beta_dense_nq(k); return kr < 16 ? 16 : kr; }

size_t beta_dense_scratch_elems(i64 rows, i64 cols, int k, int num_cus)
{
    i64 rt, ctl, per; int S;
    residual_dense_shape(rows, cols, num_cus, &rt, &ctl, &per, &S);
    const size_t step = (size_t)2 * S * beta_dense_ks(k) * ctl * BD_T;
    const size_t div = (size_t)3 * S * ctl * BD_T + (size_t)3 * ((cols + 255) / 256);
    return step > div ? step : div;
}

static BetaParams beta_params(double beta)
{
    BetaParams bp;
    bp.beta = beta;
    bp.e1 = beta - 1.0;
    bp.e2 = beta - 2.0;
    bp.cn = std::pow(KL_EPS, beta - 2.0);
    bp.cd = std::pow(KL_EPS, beta - 1.0);
    bp.clamp_n = beta < 2.0;
    bp.clamp_d = beta < 1.0;
    return bp;
}

template <int EBYTES, int NQ, int MODE, bool DIV>
static int beta_dense_launch(unsigned grid, const unsigned char* A, i64 lda_bytes, i64 m, i64 n, const double* R, const double* X, int ldf, int k,
                             i64 rt, i64 per, int S, i64 ncols_pad, const BetaParams& bp, double* part, hipStream_t st)
{
    constexpr int KR = 4 * NQ, KS = KR < 16 ? 16 : KR;
    constexpr int lds = (KS + KR) * BD_FP * (int)sizeof(double) + BD_T * BD_AP * (int)sizeof(float);
    if constexpr (lds > 64 * 1024) {
        static std::atomic<unsigned long long> attr_set{0};       // per device (DeviceOnce)
        if (DeviceOnce once{attr_set}) {
            SMK_HIP(hipFuncSetAttribute((const void*)beta_dense_kernel<EBYTES, NQ, MODE, DIV>, hipFuncAttributeMaxDynamicSharedMemorySize, lds));
            once.done();
        }
    }
    beta_dense_kernel<EBYTES, NQ, MODE, DIV><<<grid, 256, lds, st>>>(A, lda_bytes, m, n, R, X, ldf, k, rt, per, S, ncols_pad, bp, part);
    return 0;
}

template <int MODE, bool DIV>
static int beta_dense_dispatch(const void* A, int storage, i64 ld, i64 m, i64 n, const double* R, const double* X, int k, double beta, double* part,
                               int num_cus, hipStream_t st, int* S_out, i64* ncols_pad_out)
{
    i64 rt, ctl, per; int S;
    residual_dense_shape(m, n, num_cus, &rt, &ctl, &per, &S);
    const i64 ncols_pad = ctl * BD_T;
    if (ctl * S > 0x7FFFFFFFll) { set_error("beta_dense: matrix too wide for one launch"); return -100; }
    const unsigned grid = (unsigned)(ctl * S);
    const int ldf = kp_of(k);
    const BetaParams bp = beta_params(beta);
    int rc = 0;
#define SMK_BD(EB, NQ) rc = beta_dense_launch<EB, NQ, MODE, DIV>(grid, (const unsigned char*)A, ld * EB, m, n, R, X, ldf, k, rt, per, S, ncols_pad, bp, part, st)
#define SMK_BD_NQ(EB)                                  \
    switch (beta_dense_nq(k)) {                        \
        case 1: SMK_BD(EB, 1); break;                  \
        case 2: SMK_BD(EB, 2); break;                  \
        case 4: SMK_BD(EB, 4); break;                  \
        case 8: SMK_BD(EB, 8); break;                  \
        case 16: SMK_BD(EB, 16); break;                \
        default: SMK_BD(EB, 32); break;                \
    }
    if (storage == STORE_BF16) { SMK_BD_NQ(2) } else { SMK_BD_NQ(4) }
#undef SMK_BD_NQ
#undef SMK_BD
    if (rc) return rc;
    SMK_HIP(hipGetLastError());
    *S_out = S;
    *ncols_pad_out = ncols_pad;
    return 0;
}

static bool beta_dense_args(const char* who, int k, i64 rows, i64 cols, double beta)
{
    if (k >= 1 && k <= 128 && rows >= 1 && cols >= 1 && beta >= 0.0 && beta != 1.0 && beta != 2.0) return true;
    set_error(std::string(who) + ": k in [1, 128], a matrix with entries and beta >= 0 other than 1 and 2");
    return false;
}

int launch_beta_dense_step(const void* A, int storage, i64 ld, i64 rows, i64 cols, const double* R, double* X, int k, double beta, double l1,
                           double l2, int flush, double* scratch, int num_cus, hipStream_t st)
{
    if (!beta_dense_args("launch_beta_dense_step", k, rows, cols, beta)) return -3;
    int S = 0;
    i64 ncols_pad = 0;
    const int rc = beta == 0.0 ? beta_dense_dispatch<BETA_IS, false>(A, storage, ld, rows, cols, R, X, k, beta, scratch, num_cus, st, &S, &ncols_pad)
                               : beta_dense_dispatch<BETA_POW, false>(A, storage, ld, rows, cols, R, X, k, beta, scratch, num_cus, st, &S, &ncols_pad);
    if (rc) return rc;
    // gamma: 1 / (2 - beta) below 1, 1 / (beta - 1) above 2, else 1; a half is a square root, not a power
    const double gamma = beta < 1.0 ? 1.0 / (2.0 - beta) : beta > 2.0 ? 1.0 / (beta - 1.0) : 1.0;
    const int gmode = gamma == 1.0 ? 0 : gamma == 0.5 ? 1 : 2;
    beta_dense_finish_kernel<<<(unsigned)((cols + 63) / 64), 256, 0, st>>>(scratch, S, beta_dense_ks(k), ncols_pad, cols, X, kp_of(k), k, l1, l2, gmode,
                                                                          gamma, flush);
    SMK_HIP(hipGetLastError());
    return 0;
}

int launch_beta_dense_divergence(const void* A, int storage, i64 ld, i64 rows, i64 cols, const double* R, const double* X, int k, double beta,
                                 double* scratch, double* out4, double* host_out, int num_cus, hipStream_t st)
{
    if (!beta_dense_args("launch_beta_dense_divergence", k, rows, cols, beta)) return -3;
    int S = 0;
    i64 ncols_pad = 0;
    const int rc = beta == 0.0 ? beta_dense_dispatch<BETA_IS, true>(A, storage, ld, rows, cols, R, X, k, beta, scratch, num_cus, st, &S, &ncols_pad)
                               : beta_dense_dispatch<BETA_POW, true>(A, storage, ld, rows, cols, R, X, k, beta, scratch, num_cus, st, &S, &ncols_pad);
    if (rc) return rc;
    double* blockpart = scratch + (size_t)3 * S * ncols_pad;
    const i64 nblk = (cols + 255) / 256;
    beta_dense_colsum_kernel<<<(unsigned)nblk, 256, 0, st>>>(scratch, S, ncols_pad, cols, blockpart);
    SMK_HIP(hipGetLastError());
    beta_dense_total_kernel<<<1, 1024, 0, st>>>(blockpart, nblk, beta == 0.0, beta, (double)rows * (double)cols, out4, host_out);
    SMK_HIP(hipGetLastError());
    return 0;
}

}  // namespace smk
