// smallk_amd/csrc/masked_dense.hip -- the kernels of masked beta-divergence NMF on a dense stored matrix (masked_dense.cpp,
// DESIGN.md 24): scikit-learn's multiplicative update for beta = 2 (Frobenius), 1 (Kullback-Leibler) and 0 (Itakura-Saito) with
// every sum over entries restricted to the MEASURED ones.  An entry whose stored value is NaN is not measured; every other stored
// value is a measurement, 0 included.  The mask is carried by the stored copies themselves: a half-step is still one streaming
// read of one copy, no second matrix and no bit mask.  The frame is beta_dense_kernel's -- read its comments and kl_dense_kernel's:
// 64 x 64 tiles, spans, unconditional clamped loads masked afterwards, unrolled step loops, the row map D[row = 4 reg + (lane >> 4)]
// -- and below the matrix is again `m` x `n` as stored, R (KP x m) the factor of its rows and X (KP x n) the factor of its columns,
// the one being updated.  Per measured entry (i, j, a), d = r_i . x_j:
//     MD_FRO (beta = 2):  qn = a,                 qd = d          no clamp, no division
//     MD_KL  (beta = 1):  qn = a / max(d, EPS),   qd = 1          the denominator is a contraction too: the mask differs per column
//     MD_IS  (beta = 0):  r = 1 / max(d, EPS),    qn = (r r) a,   qd = r        (beta_dense.hip's BETA_IS, the same order)
// num_j += qn r_i, den_j += qd r_i on the fp64 matrix cores, then x_j[t] *= (num_j[t] / den_j[t])^gamma (kl_dev.h: beta_update).
// What the mask asks of the kernel:
//   * a NaN never reaches a matrix-instruction operand (NaN * 0 = NaN would poison a whole accumulator): qn and qd of an
//     unmeasured entry are SELECTED to 0.0, never multiplied by a mask, and a itself is selected to 0.0 before any arithmetic;
//   * "measured" is a test on the bits of the fp32 value read from LDS, (bits & 0x7FFFFFFF) <= 0x7F800000;
//   * padding is the missing marker: rows >= m and columns >= n of a tile are staged as NaN, so the same select removes them (a
//     padded 0 would be a measured zero, and at beta = 0 its qd is 1 / EPS).
// Every sum has a fixed order and there are no atomics in the passes over the matrix: the same bits on every run.
#include <algorithm>
#include <string>

#include "common.h"
#include "devutil.h"
#include "kl_dev.h"

namespace smk {

static constexpr int MD_T = 64;               // rows and columns of a tile
static constexpr int MD_FP = 65;              // doubles per factor row of a slab in LDS (as BD_FP)
static constexpr int MD_AP = 68;              // floats per column of the matrix tile in LDS (as BD_AP)
static constexpr int MD_IS = 0, MD_KL = 1, MD_FRO = 2;        // the mode is beta itself
static constexpr unsigned MD_NAN = 0x7FC00000u;               // the canonical quiet NaN: what padding is staged as

__device__ __forceinline__ bool md_measured(float v) { return (__builtin_bit_cast(unsigned, v) & 0x7FFFFFFFu) <= 0x7F800000u; }

// DIV = false: the step; part [S][2][KS][ncols_pad], numerator then denominator partials.  DIV = true: the same product, then per
// column the sums D over the measured entries is formed from and their number; part [4][S][ncols_pad]:
//   MD_FRO: sum (a - d)^2, sum a^2, nothing, count;
//   MD_KL:  sum a log(a / d) over a > EPS (d clamped), sum a, sum d (d as it is), count;
//   MD_IS:  sum a / d, sum log(a / d) over a > EPS (d clamped), nothing, count.
// a > EPS is false for a NaN by itself; sum d and the count take the select.
template <int EBYTES, int NQ, int MODE, bool DIV>
__global__ __launch_bounds__(256) void masked_dense_kernel(const unsigned char* __restrict__ A, i64 lda_bytes, i64 m, i64 n,
                                                           const double* __restrict__ R, const double* __restrict__ X, int ldf, int k,
                                                           i64 row_tiles, i64 tiles_per_span, int S, i64 ncols_pad, double* __restrict__ part)
{
    constexpr int KR = 4 * NQ;
    constexpr int KS = KR < 16 ? 16 : KR;
    constexpr int NU = KS / 16;
    constexpr int NG = (KR + MD_T - 1) / MD_T;
    extern __shared__ __attribute__((aligned(16))) unsigned char md_lds[];
    double* Rs = (double*)md_lds;                         // [KS][MD_FP]: R of the tile's rows
    double* Xs = Rs + KS * MD_FP;                         // [KR][MD_FP]: X of the tile's columns
    float* As = (float*)(Xs + KR * MD_FP);                // [64 columns][MD_AP]
    const i64 bid = blockIdx.x;
    const i64 ct = bid / S;
    const int sp = (int)(bid % S);
    const i64 rt0 = (i64)sp * tiles_per_span;
    i64 rt1 = rt0 + tiles_per_span;
    if (rt1 > row_tiles) rt1 = row_tiles;
    const i64 c0 = ct * MD_T;
    const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6), l15 = lane & 15, l4 = lane >> 4;
    typedef __attribute__((ext_vector_type(4))) double f64x4;
    f64x4 acc[4];
    f64x4 nacc[DIV ? 1 : NU], dacc[DIV ? 1 : NU];
    double s1 = 0.0, s2 = 0.0, s3 = 0.0, cnt = 0.0;
#pragma unroll
    for (int u = 0; u < (DIV ? 1 : NU); ++u) nacc[u] = dacc[u] = f64x4{0.0, 0.0, 0.0, 0.0};
    float bv[16];
    double rv[NG][16];
    int kc[NG];
#pragma unroll
    for (int g = 0; g < NG; ++g) kc[g] = 64 * g + lane < k ? 64 * g + lane : k - 1;
    auto fetch = [&](i64 rt) {
        const i64 r0 = rt * MD_T;
        const bool row_in = r0 + lane < m;
        const i64 rl = row_in ? r0 + lane : m - 1;
#pragma unroll
        for (int i = 0; i < 16; ++i) {
            const i64 c = c0 + 4 * i + wave;
            const unsigned char* col = A + (c < n ? c : n - 1) * lda_bytes;      // scalar
            float v;
            if constexpr (EBYTES == 2) v = bf16_bits_to_f32(__builtin_nontemporal_load((const unsigned short*)col + rl));
            else v = __builtin_nontemporal_load((const float*)col + rl);
            bv[i] = (row_in && c < n) ? v : __builtin_bit_cast(float, MD_NAN);   // outside the matrix: not measured
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
            for (int i = 0; i < 16; ++i) Xs[(64 * g + lane) * MD_FP + 4 * i + wave] = (c0 + 4 * i + wave < n && 64 * g + lane < k) ? t[i] : 0.0;
        }
    }
    if (rt0 < rt1) fetch(rt0);
    for (i64 rt = rt0; rt < rt1; ++rt) {
#pragma unroll
        for (int t = 0; t < 4; ++t) acc[t] = f64x4{0.0, 0.0, 0.0, 0.0};
#pragma unroll
        for (int i = 0; i < 16; ++i) {
            As[(4 * i + wave) * MD_AP + lane] = bv[i];
#pragma unroll
            for (int g = 0; g < NG; ++g)
                if (64 * g + lane < KS) Rs[(64 * g + lane) * MD_FP + 4 * i + wave] = (rt * MD_T + 4 * i + wave < m && 64 * g + lane < k) ? rv[g][i] : 0.0;
        }
        __syncthreads();
        if (rt + 1 < rt1) fetch(rt + 1);
#pragma unroll
        for (int q = 0; q < NQ; ++q) {
            const double b = Xs[(4 * q + l4) * MD_FP + 16 * wave + l15];
#pragma unroll
            for (int t = 0; t < 4; ++t) acc[t] = __builtin_amdgcn_mfma_f64_16x16x4f64(Rs[(4 * q + l4) * MD_FP + 16 * t + l15], b, acc[t], 0, 0, 0);
        }
#pragma unroll
        for (int t = 0; t < 4; ++t) {
            f64x4 qn, qd;
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const float af = As[(16 * wave + l15) * MD_AP + 16 * t + l4 + 4 * r];
                const bool meas = md_measured(af);
                const double av = meas ? (double)af : 0.0;            // from here on no NaN is in any arithmetic
                const double d = acc[t][r];
                if constexpr (DIV) cnt += meas ? 1.0 : 0.0;
                if constexpr (MODE == MD_FRO) {
                    if constexpr (DIV) {
                        const double e = meas ? av - d : 0.0;
                        s1 = __builtin_fma(e, e, s1);
                        s2 = __builtin_fma(av, av, s2);
                    } else {
                        qn[r] = av;
                        qd[r] = meas ? d : 0.0;
                    }
                } else {
                    const double dc = d < KL_EPS ? KL_EPS : d;
                    if constexpr (MODE == MD_KL) {
                        if constexpr (DIV) {
                            if (av > KL_EPS) s1 = __builtin_fma(av, log(av / dc), s1);
                            s2 += av;
                            s3 += meas ? d : 0.0;
                        } else {
                            qn[r] = av / dc;
                            qd[r] = meas ? 1.0 : 0.0;
                        }
                    } else if constexpr (DIV) {
                        if (av > KL_EPS) { const double q = av / dc; s1 += q; s2 += log(q); }
                    } else {
                        const double rc = 1.0 / dc;
                        qn[r] = __dmul_rn(__dmul_rn(rc, rc), av);
                        qd[r] = meas ? rc : 0.0;
                    }
                }
            }
            if constexpr (!DIV) {
#pragma unroll
                for (int r = 0; r < 4; ++r)
#pragma unroll
                    for (int u = 0; u < NU; ++u) {
                        const double a = Rs[(16 * u + l15) * MD_FP + 16 * t + 4 * r + l4];
                        nacc[u] = __builtin_amdgcn_mfma_f64_16x16x4f64(a, qn[r], nacc[u], 0, 0, 0);
                        dacc[u] = __builtin_amdgcn_mfma_f64_16x16x4f64(a, qd[r], dacc[u], 0, 0, 0);
                    }
            }
        }
        __syncthreads();
    }
    const i64 col = c0 + 16 * wave + l15;                 // < ncols_pad
    if constexpr (DIV) {
        double s[4] = {s1, s2, s3, cnt};
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            s[i] += __shfl_xor(s[i], 16, 64);
            s[i] += __shfl_xor(s[i], 32, 64);
            if (l4 == 0) part[((i64)i * S + sp) * ncols_pad + col] = s[i];
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

// the spans of both partial sets in span order, then the update of X in place (beta_dense_finish_kernel's thread map).  A column
// without a measured entry has num = den = 0: den becomes EPS in beta_update and the column goes to 0
__global__ __launch_bounds__(256) void masked_dense_finish_kernel(const double* __restrict__ part, int S, int KS, i64 ncols_pad, i64 n,
                                                                  double* __restrict__ X, int KP, int k, double l1, double l2, int gmode, int flush)
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
            xn = beta_update(X[j * KP + t], num, den, l1, l2, gmode, 0.5, flush);
        }
        X[j * KP + t] = xn;
    }
}

// the spans of a column in span order; 256 columns per workgroup, whose four sums go to blockpart in column order
// (beta_dense_colsum_kernel's shape with one more sum: 16 sums of 16, then their sum)
__global__ __launch_bounds__(256) void masked_dense_colsum_kernel(const double* __restrict__ part, int S, i64 ncols_pad, i64 n,
                                                                  double* __restrict__ blockpart)
{
    __shared__ double sh[256][4];
    const i64 j = (i64)blockIdx.x * 256 + threadIdx.x;
    double v[4] = {0.0, 0.0, 0.0, 0.0};
    if (j < n)
        for (int q = 0; q < S; ++q)
            for (int i = 0; i < 4; ++i) v[i] += part[((i64)i * S + q) * ncols_pad + j];
    for (int i = 0; i < 4; ++i) sh[threadIdx.x][i] = v[i];
    __syncthreads();
    double w[4] = {0.0, 0.0, 0.0, 0.0};
    if (threadIdx.x < 16)
        for (int e = 0; e < 16; ++e)
            for (int i = 0; i < 4; ++i) w[i] += sh[16 * threadIdx.x + e][i];
    __syncthreads();
    if (threadIdx.x < 16)
        for (int i = 0; i < 4; ++i) sh[threadIdx.x][i] = w[i];
    __syncthreads();
    if (threadIdx.x == 0)
        for (int i = 0; i < 4; ++i) {
            double t = 0.0;
            for (int e = 0; e < 16; ++e) t += sh[e][i];
            blockpart[4 * (i64)blockIdx.x + i] = t;
        }
}

// the workgroups' sums in index order (beta_dense_total_kernel's shape), then D over the measured entries:
// out = {D, s1, s2, s3, count} with D = s1 / 2 (MD_FRO), (s1 - s2) + s3 (MD_KL), (s1 - count) - s2 (MD_IS).  host_out: pinned or null
__global__ __launch_bounds__(1024) void masked_dense_total_kernel(const double* __restrict__ blockpart, i64 nblk, int mode, double* __restrict__ out,
                                                                  double* host_out)
{
    __shared__ double sh[1024][4];
    double v[4] = {0.0, 0.0, 0.0, 0.0};
    for (i64 b = threadIdx.x; b < nblk; b += 1024)
        for (int i = 0; i < 4; ++i) v[i] += blockpart[4 * b + i];
    for (int i = 0; i < 4; ++i) sh[threadIdx.x][i] = v[i];
    __syncthreads();
    for (int w = 512; w > 0; w >>= 1) {
        if ((int)threadIdx.x < w)
            for (int i = 0; i < 4; ++i) sh[threadIdx.x][i] += sh[threadIdx.x + w][i];
        __syncthreads();
    }
    if (threadIdx.x == 0) {
        const double a = sh[0][0], b = sh[0][1], c = sh[0][2], cnt = sh[0][3];
        const double D = mode == MD_FRO ? 0.5 * a : mode == MD_KL ? (a - b) + c : (a - cnt) - b;
        const double r5[5] = {D, a, b, c, cnt};
        for (int i = 0; i < 5; ++i) {
            out[i] = r5[i];
            if (host_out) host_out[i] = r5[i];
        }
    }
}

// what the stored values are, NaN aside: bit 0 of *flag a measured negative value, bit 1 a measured zero, bit 2 any measured entry.
// A workgroup walks columns, its threads the rows of a column; only rows < m and columns < n are read
template <int EBYTES>
__global__ __launch_bounds__(256) void masked_dense_look_kernel(const unsigned char* __restrict__ A, i64 lda_bytes, i64 m, i64 n, int* flag)
{
    int found = 0;
    for (i64 c = blockIdx.x; c < n; c += gridDim.x) {
        const unsigned char* col = A + c * lda_bytes;
        for (i64 r = threadIdx.x; r < m; r += 256) {
            float v;
            if constexpr (EBYTES == 2) v = bf16_bits_to_f32(((const unsigned short*)col)[r]);
            else v = ((const float*)col)[r];
            if (!md_measured(v)) continue;
            found |= 4;
            if (v < 0.f) found |= 1;
            else if (!(v > 0.f)) found |= 2;
        }
    }
    if (found) atomicOr(flag, found);
}

// ---- launchers ---------------------------------------------------------------------------------------------------------
static int masked_dense_nq(int k) { return k > 64 ? 32 : k > 32 ? 16 : k > 16 ? 8 : k > 8 ? 4 : k > 4 ? 2 : 1; }
static int masked_dense_ks(int k) { const int kr = 4 * masked_dense_nq(k); return kr < 16 ? 16 : kr; }

size_t masked_dense_scratch_elems(i64 rows, i64 cols, int k, int num_cus)
{
    i64 rt, ctl, per; int S;
    residual_dense_shape(rows, cols, num_cus, &rt, &ctl, &per, &S);
    const size_t step = (size_t)2 * S * masked_dense_ks(k) * ctl * MD_T;
    const size_t div = (size_t)4 * S * ctl * MD_T + (size_t)4 * ((cols + 255) / 256);
    return step > div ? step : div;
}

template <int EBYTES, int NQ, int MODE, bool DIV>
static int masked_dense_launch(unsigned grid, const unsigned char* A, i64 lda_bytes, i64 m, i64 n, const double* R, const double* X, int ldf, int k,
                               i64 rt, i64 per, int S, i64 ncols_pad, double* part, hipStream_t st)
{
    constexpr int KR = 4 * NQ, KS = KR < 16 ? 16 : KR;
    constexpr int lds = (KS + KR) * MD_FP * (int)sizeof(double) + MD_T * MD_AP * (int)sizeof(float);
    if constexpr (lds > 64 * 1024) {
        static std::atomic<unsigned long long> attr_set{0};       // per device (DeviceOnce)
        if (DeviceOnce once{attr_set}) {
            SMK_HIP(hipFuncSetAttribute((const void*)masked_dense_kernel<EBYTES, NQ, MODE, DIV>, hipFuncAttributeMaxDynamicSharedMemorySize, lds));
            once.done();
        }
    }
    masked_dense_kernel<EBYTES, NQ, MODE, DIV><<<grid, 256, lds, st>>>(A, lda_bytes, m, n, R, X, ldf, k, rt, per, S, ncols_pad, part);
    return 0;
}

template <int MODE, bool DIV>
static int masked_dense_dispatch(const void* A, int storage, i64 ld, i64 m, i64 n, const double* R, const double* X, int k, double* part, int num_cus,
                                 hipStream_t st, int* S_out, i64* ncols_pad_out)
{
    i64 rt, ctl, per; int S;
    residual_dense_shape(m, n, num_cus, &rt, &ctl, &per, &S);
    const i64 ncols_pad = ctl * MD_T;
    if (ctl * S > 0x7FFFFFFFll) { set_error("masked_dense: matrix too wide for one launch"); return -100; }
    const unsigned grid = (unsigned)(ctl * S);
    const int ldf = kp_of(k);
    int rc = 0;
#define SMK_MD(EB, NQ) rc = masked_dense_launch<EB, NQ, MODE, DIV>(grid, (const unsigned char*)A, ld * EB, m, n, R, X, ldf, k, rt, per, S, ncols_pad, part, st)
#define SMK_MD_NQ(EB)                                  \
    switch (masked_dense_nq(k)) {                      \
        case 1: SMK_MD(EB, 1); break;                  \
        case 2: SMK_MD(EB, 2); break;                  \
        case 4: SMK_MD(EB, 4); break;                  \
        case 8: SMK_MD(EB, 8); break;                  \
        case 16: SMK_MD(EB, 16); break;                \
        default: SMK_MD(EB, 32); break;                \
    }
    if (storage == STORE_BF16) { SMK_MD_NQ(2) } else { SMK_MD_NQ(4) }
#undef SMK_MD_NQ
#undef SMK_MD
    if (rc) return rc;
    SMK_HIP(hipGetLastError());
    *S_out = S;
    *ncols_pad_out = ncols_pad;
    return 0;
}

template <bool DIV>
static int masked_dense_mode(int mode, const void* A, int storage, i64 ld, i64 m, i64 n, const double* R, const double* X, int k, double* part,
                             int num_cus, hipStream_t st, int* S, i64* ncols_pad)
{
    if (mode == MD_FRO) return masked_dense_dispatch<MD_FRO, DIV>(A, storage, ld, m, n, R, X, k, part, num_cus, st, S, ncols_pad);
    if (mode == MD_KL) return masked_dense_dispatch<MD_KL, DIV>(A, storage, ld, m, n, R, X, k, part, num_cus, st, S, ncols_pad);
    return masked_dense_dispatch<MD_IS, DIV>(A, storage, ld, m, n, R, X, k, part, num_cus, st, S, ncols_pad);
}

static bool masked_dense_args(const char* who, int k, i64 rows, i64 cols, int beta)
{
    if (k >= 1 && k <= 128 && rows >= 1 && cols >= 1 && beta >= 0 && beta <= 2) return true;
    set_error(std::string(who) + ": k in [1, 128], a matrix with entries and beta 0, 1 or 2");
    return false;
}

int launch_masked_dense_step(const void* A, int storage, i64 ld, i64 rows, i64 cols, const double* R, double* X, int k, int beta, double l1, double l2,
                             int flush, double* scratch, int num_cus, hipStream_t st)
{
    if (!masked_dense_args("launch_masked_dense_step", k, rows, cols, beta)) return -3;
    int S = 0;
    i64 ncols_pad = 0;
    const int rc = masked_dense_mode<false>(beta, A, storage, ld, rows, cols, R, X, k, scratch, num_cus, st, &S, &ncols_pad);
    if (rc) return rc;
    // gamma: a half at beta = 0 (a square root, not a power), else 1
    masked_dense_finish_kernel<<<(unsigned)((cols + 63) / 64), 256, 0, st>>>(scratch, S, masked_dense_ks(k), ncols_pad, cols, X, kp_of(k), k, l1, l2,
                                                                            beta == MD_IS ? 1 : 0, flush);
    SMK_HIP(hipGetLastError());
    return 0;
}

int launch_masked_dense_divergence(const void* A, int storage, i64 ld, i64 rows, i64 cols, const double* R, const double* X, int k, int beta,
                                   double* scratch, double* out5, double* host_out, int num_cus, hipStream_t st)
{
    if (!masked_dense_args("launch_masked_dense_divergence", k, rows, cols, beta)) return -3;
    int S = 0;
    i64 ncols_pad = 0;
    const int rc = masked_dense_mode<true>(beta, A, storage, ld, rows, cols, R, X, k, scratch, num_cus, st, &S, &ncols_pad);
    if (rc) return rc;
    double* blockpart = scratch + (size_t)4 * S * ncols_pad;
    const i64 nblk = (cols + 255) / 256;
    masked_dense_colsum_kernel<<<(unsigned)nblk, 256, 0, st>>>(scratch, S, ncols_pad, cols, blockpart);
    SMK_HIP(hipGetLastError());
    masked_dense_total_kernel<<<1, 1024, 0, st>>>(blockpart, nblk, beta, out5, host_out);
    SMK_HIP(hipGetLastError());
    return 0;
}

int launch_masked_dense_look(const void* A, int storage, i64 ld, i64 rows, i64 cols, int* flag, hipStream_t st)
{
    const unsigned grid = (unsigned)std::min<i64>(cols, 4096);
    if (storage == STORE_BF16) masked_dense_look_kernel<2><<<grid, 256, 0, st>>>((const unsigned char*)A, ld * 2, rows, cols, flag);
    else masked_dense_look_kernel<4><<<grid, 256, 0, st>>>((const unsigned char*)A, ld * 4, rows, cols, flag);
    SMK_HIP(hipGetLastError());
    return 0;
}

}  // namespace smk
