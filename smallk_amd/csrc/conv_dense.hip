// smallk_amd/csrc/conv_dense.hip -- the kernels of convolutive NMF on a dense stored matrix (conv_dense.cpp, conv_dense.h, DESIGN.md
// 27): a component is a pattern of T consecutive columns,
//     Lambda[i, j] = sum_{t < T} sum_{r < k} W_t[i, r] H[r, j - t]                       (terms with j - t < 0 are absent),
// fitted under the Kullback-Leibler (beta = 1) or the Itakura-Saito (beta = 0) divergence by the multiplicative update.  With the
// slices side by side, Wc = [W_0 ... W_{T-1}] (m x T KP4, KP4 = k rounded up to a multiple of 4), and H~[(t, r), j] = H[r, j - t] the
// Toeplitz expansion of H, Lambda = Wc H~ is a product of inner dimension KR = T KP4 <= 128, and the frame of beta_dense.hip
// carries over -- read its comments and kl_dense_kernel's: 64 x 64 tiles, spans of row tiles, unconditional clamped loads masked
// afterwards, the product on v_mfma_f64_16x16x4_f64 with the row map D[row = 4 reg + (lane >> 4)], the quotients (qn, qd) formed in the
// accumulator registers one 16-row block at a time, two chained contractions, fixed summation orders, no atomics.
//
// What differs: H~ exists nowhere.  The columns of H a tile can meet are staged once as the slab Hs[KP4][64 + T - 1] -- slab column
// cc is column base - (T - 1) + cc of H, zero before column 0 and from column n on -- and the operand of lag t is that slab read
// T - 1 - t columns to the right.  The four inner indices of one matrix instruction lie in one lag (KP4 is a multiple of 4), so in
// the product the shift is one scalar term of the LDS address.  In global memory the slab is one contiguous range of Hc (pitch
// KP4), so staging it is a copy with a range check.
//   SIDE_H (over A, H updated): the slab is the factor of the tile's columns, staged once per workgroup; Wc's rows are streamed with
//     the matrix as beta_dense's R.  The second contractions give G[(t, r), j] = sum_i W_t[i, r] q[i, j] per span; the update of
//     H[r, j] needs sum_t G[(t, r), j + t], a sum along a diagonal that crosses into the next tile's partials: the finishing kernel.
//   SIDE_W (over the stored transpose, Wc updated): the slab is the factor of the streamed rows, staged per row tile through
//     registers like the matrix; Wc of the tile's columns is staged once.  The second contractions' left operand is H~ itself,
//     row q = (t, r) per lane: a per-lane slab offset formed once.  The partials are the numerators and denominators of Wc's
//     entries as they stand.  The T - 1 streamed rows past the last one are not rows of zeros of H~ -- lag t of row n + s is
//     column n + s - t of H -- so their quotients are set to zero before the contractions.
//   SIDE_DIV: SIDE_H's product, then per column the sums the divergence is formed from.
// MODE: CONV_IS  r = 1 / max(d, EPS), qn = (r r) a, qd = r;     CONV_KL  qn = a / max(d, EPS), qd = 1 (the uniform second
// contraction then forms the lag-dependent truncated sums of the other factor; DESIGN.md 27 says why no kernel of their own).
// NU: 16-row blocks of the second contractions, KS = 16 NU >= KR; the product's length KR / 4 is a run-time count.
#include <algorithm>
#include <string>

#include "conv_dense.h"
#include "devutil.h"
#include "kl_dev.h"

namespace smk {

static constexpr int CV_T = 64;               // rows and columns of a tile
static constexpr int CV_FP = 65;              // doubles per row of the plain factor's slab in LDS (as BD_FP)
static constexpr int CV_AP = 68;              // floats per column of the matrix tile in LDS (as BD_AP)
static constexpr int CONV_IS = 0, CONV_KL = 1;
static constexpr int SIDE_H = 0, SIDE_W = 1, SIDE_DIV = 2;

// doubles per row of the shifted slab: 64 + T - 1 columns, made odd
__host__ __device__ inline int conv_hp(int T) { return (CV_T + T - 1) | 1; }

// rows x cols: the matrix as stored (A for SIDE_H / SIDE_DIV, the transpose for SIDE_W).  P: Wc (pitch KR).  Hc: pitch KP4, hlen =
// KP4 times its columns.  part: step [S][2][KS][ncols_pad] numerator then denominator partials; SIDE_DIV [3][S][ncols_pad]:
//   CONV_IS: sum a / d, sum log(a / d) over the entries with a > EPS (d clamped), nothing;
//   CONV_KL: sum a log(a / d), sum a over the entries with a > EPS (d clamped), sum d over every entry.
template <int EBYTES, int NU, int MODE, int SIDE>
__global__ __launch_bounds__(256) void conv_dense_kernel(const unsigned char* __restrict__ A, i64 lda_bytes, i64 rows, i64 cols,
                                                         const double* __restrict__ P, const double* __restrict__ Hc, i64 hlen, int KP4, int T,
                                                         i64 row_tiles, i64 tiles_per_span, int S, i64 ncols_pad, double* __restrict__ part)
{
    constexpr int KS = 16 * NU;
    constexpr int NG = (KS + CV_T - 1) / CV_T;
    constexpr int SLN = 4 * NU;                           // slab elements per thread: KP4 (63 + T) <= 64 KR <= 256 SLN
    constexpr bool DIV = SIDE == SIDE_DIV, WS = SIDE == SIDE_W;
    const int KR = T * KP4, nq = KR >> 2, HP = conv_hp(T), slab_total = KP4 * (CV_T + T - 1);
    extern __shared__ __attribute__((aligned(16))) unsigned char cv_lds[];
    double* Ps = (double*)cv_lds;                         // [KS][CV_FP]: Wc of the tile's rows (SIDE_W: columns), rows >= KR zero
    double* Hs = Ps + KS * CV_FP;                         // [KP4][HP]: the slab of H
    float* As = (float*)(Hs + KP4 * HP);                  // [64 columns][CV_AP]
    const i64 bid = blockIdx.x;
    const i64 ct = bid / S;
    const int sp = (int)(bid % S);
    const i64 rt0 = (i64)sp * tiles_per_span;
    i64 rt1 = rt0 + tiles_per_span;
    if (rt1 > row_tiles) rt1 = row_tiles;
    const i64 c0 = ct * CV_T;
    const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6), l15 = lane & 15, l4 = lane >> 4;
    typedef __attribute__((ext_vector_type(4))) double f64x4;
    f64x4 acc[4];
    f64x4 nacc[DIV ? 1 : NU], dacc[DIV ? 1 : NU];
    double s1 = 0.0, s2 = 0.0, s3 = 0.0;
#pragma unroll
    for (int u = 0; u < (DIV ? 1 : NU); ++u) nacc[u] = dacc[u] = f64x4{0.0, 0.0, 0.0, 0.0};
    float bv[16];
    double rv[WS ? 1 : NG][16];                           // SIDE_H: Wc of the next row tile
    double sv[WS ? SLN : 1];                              // SIDE_W: the slab of the next row tile
    int kc[NG];
#pragma unroll
    for (int g = 0; g < NG; ++g) kc[g] = 64 * g + lane < KR ? 64 * g + lane : KR - 1;
    // the slab whose column T - 1 is column `base` of H: element idx = cc KP4 + r of it is Hc[(base - (T - 1)) KP4 + idx]
    const int sa = 256 / KP4, sb = 256 % KP4, sr0 = tid % KP4, sc0 = tid / KP4;
    auto slab_load = [&](i64 base, double (&v)[SLN]) {
        const i64 g0 = (base - (T - 1)) * KP4 + tid;
#pragma unroll
        for (int e = 0; e < SLN; ++e) {
            const i64 g = g0 + 256 * e;
            v[e] = (tid + 256 * e < slab_total && g >= 0 && g < hlen) ? Hc[g] : 0.0;
        }
    };
    auto slab_store = [&](const double (&v)[SLN]) {
        int r = sr0, c = sc0;
#pragma unroll
        for (int e = 0; e < SLN; ++e) {
            if (tid + 256 * e < slab_total) Hs[r * HP + c] = v[e];
            r += sb;
            c += sa;
            if (r >= KP4) { r -= KP4; ++c; }
        }
    };
    auto fetch = [&](i64 rt) {
        const i64 r0 = rt * CV_T;
        const bool row_in = r0 + lane < rows;
        const i64 rl = row_in ? r0 + lane : rows - 1;
#pragma unroll
        for (int i = 0; i < 16; ++i) {
            const i64 c = c0 + 4 * i + wave;
            const unsigned char* col = A + (c < cols ? c : cols - 1) * lda_bytes;      // scalar
            float v;
            if constexpr (EBYTES == 2) v = bf16_bits_to_f32(__builtin_nontemporal_load((const unsigned short*)col + rl));
            else v = __builtin_nontemporal_load((const float*)col + rl);
            bv[i] = (row_in && c < cols) ? v : 0.f;
        }
        if constexpr (WS) {
            slab_load(r0, sv);
        } else {
#pragma unroll
            for (int g = 0; g < NG; ++g)
#pragma unroll
                for (int i = 0; i < 16; ++i) {
                    const i64 r = r0 + 4 * i + wave;
                    const double* row = P + (r < rows ? r : rows - 1) * KR;               // scalar
                    rv[g][i] = row[kc[g]];              // masked when it is stored to LDS (below)
                }
        }
    };
    // what belongs to the tile's columns, staged once
    if constexpr (WS) {
#pragma unroll
        for (int g = 0; g < NG; ++g) {
            double t[16];
#pragma unroll
            for (int i = 0; i < 16; ++i) {
                const i64 c = c0 + 4 * i + wave;
                t[i] = P[(c < cols ? c : cols - 1) * KR + kc[g]];
            }
            if (64 * g + lane < KS) {
#pragma unroll
                for (int i = 0; i < 16; ++i) Ps[(64 * g + lane) * CV_FP + 4 * i + wave] = (c0 + 4 * i + wave < cols && 64 * g + lane < KR) ? t[i] : 0.0;
            }
        }
    } else {
        double t[SLN];
        slab_load(c0, t);
        slab_store(t);
    }
    // SIDE_W: where row q = (t, r) of H~ starts in the slab, per lane and 16-row block (rows >= KR: any valid place, never read back)
    int hb[WS ? NU : 1];
    if constexpr (WS) {
#pragma unroll
        for (int u = 0; u < NU; ++u) {
            const int q = 16 * u + l15 < KR ? 16 * u + l15 : 0;
            const int tq = q / KP4;
            hb[u] = (q - tq * KP4) * HP + (T - 1 - tq);
        }
    }
    if (rt0 < rt1) fetch(rt0);
    for (i64 rt = rt0; rt < rt1; ++rt) {
#pragma unroll
        for (int t = 0; t < 4; ++t) acc[t] = f64x4{0.0, 0.0, 0.0, 0.0};
#pragma unroll
        for (int i = 0; i < 16; ++i) {
            As[(4 * i + wave) * CV_AP + lane] = bv[i];
            if constexpr (!WS) {
#pragma unroll
                for (int g = 0; g < NG; ++g)
                    if (64 * g + lane < KS) Ps[(64 * g + lane) * CV_FP + 4 * i + wave] = (rt * CV_T + 4 * i + wave < rows && 64 * g + lane < KR) ? rv[g][i] : 0.0;
            }
        }
        if constexpr (WS) slab_store(sv);
        __syncthreads();
        if (rt + 1 < rt1) fetch(rt + 1);
        [[maybe_unused]] const int live_rows = rows - rt * CV_T < CV_T ? (int)(rows - rt * CV_T) : CV_T;
        // the product: step q covers inner indices 4 q .. 4 q + 3 = (lag, rows r0 .. r0 + 3); sh = T - 1 - lag
        {
            int r0 = 0, sh = T - 1;
            for (int q = 0; q < nq; ++q) {
                const double* prow = Ps + (4 * q + l4) * CV_FP;
                const double* hrow = Hs + (r0 + l4) * HP + sh;
                if constexpr (WS) {
                    const double b = prow[16 * wave + l15];
#pragma unroll
                    for (int t = 0; t < 4; ++t) acc[t] = __builtin_amdgcn_mfma_f64_16x16x4f64(hrow[16 * t + l15], b, acc[t], 0, 0, 0);
                } else {
                    const double b = hrow[16 * wave + l15];
#pragma unroll
                    for (int t = 0; t < 4; ++t) acc[t] = __builtin_amdgcn_mfma_f64_16x16x4f64(prow[16 * t + l15], b, acc[t], 0, 0, 0);
                }
                r0 += 4;
                if (r0 == KP4) { r0 = 0; --sh; }
            }
        }
#pragma unroll
        for (int t = 0; t < 4; ++t) {
            f64x4 qn, qd;
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const double av = (double)As[(16 * wave + l15) * CV_AP + 16 * t + l4 + 4 * r];
                const double d = acc[t][r];
                const double dc = d < KL_EPS ? KL_EPS : d;
                if constexpr (MODE == CONV_IS) {
                    if constexpr (DIV) {
                        if (av > KL_EPS) { const double q = av / dc; s1 += q; s2 += log(q); }
                    } else {
                        const double rc = 1.0 / dc;
                        qn[r] = __dmul_rn(__dmul_rn(rc, rc), av);
                        qd[r] = rc;
                    }
                } else {
                    if constexpr (DIV) {
                        if (av > KL_EPS) { s1 = __builtin_fma(av, log(av / dc), s1); s2 += av; }
                        s3 += d;
                    } else {
                        qn[r] = av / dc;
                        qd[r] = 1.0;
                    }
                }
            }
            if constexpr (WS) {
                // a streamed row past the last one still meets columns of H through its lags: its quotients must not count
#pragma unroll
                for (int r = 0; r < 4; ++r)
                    if (16 * t + 4 * r + l4 >= live_rows) qn[r] = qd[r] = 0.0;
            }
            if constexpr (!DIV) {
#pragma unroll
                for (int r = 0; r < 4; ++r)
#pragma unroll
                    for (int u = 0; u < NU; ++u) {
                        double a;
                        if constexpr (WS) a = Hs[hb[u] + 16 * t + 4 * r + l4];
                        else a = Ps[(16 * u + l15) * CV_FP + 16 * t + 4 * r + l4];
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

// The finish of both sides, a column per lane.  X has `nout` entries per column (pitch ldx); entry q takes, for lag t = 0 .. TL - 1
// in order and within a lag the spans in order, the partials of row q + t KP4 at column j + t while j + t < ncols -- SIDE_H: nout =
// KP4, TL = T, the shift-add along the diagonal, which reads the next column tile's partials; SIDE_W: nout = T KP4, TL = 1, the
// plain sum over spans.  Then beta_update in place.  Pad entries (q mod KP4 >= k) are zero and stay zero.
__global__ __launch_bounds__(256) void conv_dense_finish_kernel(const double* __restrict__ part, int S, int KS, i64 ncols_pad, i64 ncols,
                                                                double* __restrict__ X, int ldx, int KP4, int k, int nout, int TL, double l1, double l2,
                                                                int gmode, int flush)
{
    const i64 j = (i64)blockIdx.x * 64 + (threadIdx.x & 63);
    if (j >= ncols) return;
    for (int q = threadIdx.x >> 6; q < nout; q += 4) {
        if (q % KP4 >= k) continue;
        double num = 0.0, den = 0.0;
        for (int t = 0; t < TL && j + t < ncols; ++t)
            for (int s = 0; s < S; ++s) {
                num += part[(((i64)s * 2) * KS + q + t * KP4) * ncols_pad + j + t];
                den += part[(((i64)s * 2 + 1) * KS + q + t * KP4) * ncols_pad + j + t];
            }
        X[j * ldx + q] = beta_update(X[j * ldx + q], num, den, l1, l2, gmode, 0.5, flush);
    }
}

// the spans of a column in span order; 256 columns per workgroup, whose three sums go to blockpart in column order (the shape of
// beta_dense_colsum_kernel: 16 sums of 16, then their sum)
__global__ __launch_bounds__(256) void conv_dense_colsum_kernel(const double* __restrict__ part, int S, i64 ncols_pad, i64 n,
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

// the workgroups' sums in index order (beta_dense_total_kernel's shape), then D.  is != 0: out = {(s1 - count) - s2, s1, s2, count};
// else out = {s1 + (s3 - s2), s1, s3, 0}.  host_out: pinned or null
__global__ __launch_bounds__(1024) void conv_dense_total_kernel(const double* __restrict__ blockpart, i64 nblk, int is, double count,
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
        const double a = sh[0][0], b = sh[0][1], c = sh[0][2];
        const double r4[4] = {is ? (a - count) - b : a + (c - b), a, is ? b : c, is ? count : 0.0};
        for (int i = 0; i < 4; ++i) {
            out[i] = r4[i];
            if (host_out) host_out[i] = r4[i];
        }
    }
}

// ---- launchers ---------------------------------------------------------------------------------------------------------
static int conv_dense_nu(int KR) { return KR > 64 ? 8 : KR > 32 ? 4 : KR > 16 ? 2 : 1; }

size_t conv_dense_scratch_elems(i64 m, i64 n, int k, int T, int num_cus)
{
    const int KS = 16 * conv_dense_nu(T * conv_kp4(k));
    size_t best = 0;
    for (int side = 0; side < 2; ++side) {
        const i64 rows = side ? n : m, cols = side ? m : n;
        i64 rt, ctl, per; int S;
        residual_dense_shape(rows, cols, num_cus, &rt, &ctl, &per, &S);
        best = std::max(best, (size_t)2 * S * KS * ctl * CV_T);
        best = std::max(best, (size_t)3 * S * ctl * CV_T + (size_t)3 * ((cols + 255) / 256));
    }
    return best;
}

struct ConvLaunch {
    const unsigned char* A; i64 lda_bytes, rows, cols;
    const double *P, *Hc; i64 hlen; int KP4, T;
    i64 rt, per; int S; i64 ncols_pad; double* part;
    unsigned grid; int lds; hipStream_t st;
};

template <int EBYTES, int NU, int MODE, int SIDE>
static int conv_dense_launch(const ConvLaunch& c)
{
    // the most a kernel of this NU can ask for: T = 1, KP4 = 16 NU (both slabs [16 NU][65])
    constexpr int lds_max = 2 * 16 * NU * CV_FP * (int)sizeof(double) + CV_T * CV_AP * (int)sizeof(float);
    if constexpr (lds_max > 64 * 1024) {
        static std::atomic<unsigned long long> attr_set{0};       // per device (DeviceOnce)
        if (DeviceOnce once{attr_set}) {
            SMK_HIP(hipFuncSetAttribute((const void*)conv_dense_kernel<EBYTES, NU, MODE, SIDE>, hipFuncAttributeMaxDynamicSharedMemorySize, lds_max));
            once.done();
        }
    }
    conv_dense_kernel<EBYTES, NU, MODE, SIDE><<<c.grid, 256, c.lds, c.st>>>(c.A, c.lda_bytes, c.rows, c.cols, c.P, c.Hc, c.hlen, c.KP4, c.T, c.rt, c.per, c.S,
                                                                             c.ncols_pad, c.part);
    return 0;
}

template <int MODE, int SIDE>
static int conv_dense_dispatch(const void* A, int storage, i64 ld, i64 rows, i64 cols, const double* P, const double* Hc, i64 hcols, int k, int T,
                               double* part, int num_cus, hipStream_t st, int* S_out, i64* ncols_pad_out)
{
    ConvLaunch c;
    i64 ctl;
    residual_dense_shape(rows, cols, num_cus, &c.rt, &ctl, &c.per, &c.S);
    if (ctl * c.S > 0x7FFFFFFFll) { set_error("conv_dense: matrix too wide for one launch"); return -100; }
    c.KP4 = conv_kp4(k);
    c.T = T;
    const int NU = conv_dense_nu(T * c.KP4), eb = storage == STORE_BF16 ? 2 : 4;
    c.A = (const unsigned char*)A;
    c.lda_bytes = ld * eb;
    c.rows = rows;
    c.cols = cols;
    c.P = P;
    c.Hc = Hc;
    c.hlen = hcols * c.KP4;
    c.ncols_pad = ctl * CV_T;
    c.part = part;
    c.grid = (unsigned)(ctl * c.S);
    c.lds = (16 * NU * CV_FP + c.KP4 * conv_hp(T)) * (int)sizeof(double) + CV_T * CV_AP * (int)sizeof(float);
    c.st = st;
    int rc = 0;
#define SMK_CV_NU(EB)                                                       \
    switch (NU) {                                                           \
        case 1: rc = conv_dense_launch<EB, 1, MODE, SIDE>(c); break;        \
        case 2: rc = conv_dense_launch<EB, 2, MODE, SIDE>(c); break;        \
        case 4: rc = conv_dense_launch<EB, 4, MODE, SIDE>(c); break;        \
        default: rc = conv_dense_launch<EB, 8, MODE, SIDE>(c); break;       \
    }
    if (eb == 2) { SMK_CV_NU(2) } else { SMK_CV_NU(4) }
#undef SMK_CV_NU
    if (rc) return rc;
    SMK_HIP(hipGetLastError());
    *S_out = c.S;
    *ncols_pad_out = c.ncols_pad;
    return 0;
}

static bool conv_dense_args(const char* who, i64 m, i64 n, int k, int T, int beta)
{
    if (k >= 1 && T >= 1 && T * conv_kp4(k) <= 128 && m >= 1 && n >= T && (beta == 0 || beta == 1)) return true;
    set_error(std::string(who) + ": k >= 1, 1 <= T <= n, T roundup(k, 4) <= 128 and beta 0 or 1");
    return false;
}

int launch_conv_dense_step(const void* A, int storage, i64 ld, i64 m, i64 n, int w_side, double* Wc, double* Hc, int k, int T, int beta, double l1,
                           double l2, int flush, double* scratch, int num_cus, hipStream_t st)
{
    if (!conv_dense_args("launch_conv_dense_step", m, n, k, T, beta)) return -3;
    const int KP4 = conv_kp4(k), KR = T * KP4, KS = 16 * conv_dense_nu(KR);
    // the stored copy read: A (m x n) for H, the transpose (n x m) for W; H has n columns either way
    const i64 rows = w_side ? n : m, cols = w_side ? m : n;
    int S = 0, rc;
    i64 ncols_pad = 0;
    if (w_side) rc = beta ? conv_dense_dispatch<CONV_KL, SIDE_W>(A, storage, ld, rows, cols, Wc, Hc, n, k, T, scratch, num_cus, st, &S, &ncols_pad)
                          : conv_dense_dispatch<CONV_IS, SIDE_W>(A, storage, ld, rows, cols, Wc, Hc, n, k, T, scratch, num_cus, st, &S, &ncols_pad);
    else rc = beta ? conv_dense_dispatch<CONV_KL, SIDE_H>(A, storage, ld, rows, cols, Wc, Hc, n, k, T, scratch, num_cus, st, &S, &ncols_pad)
                   : conv_dense_dispatch<CONV_IS, SIDE_H>(A, storage, ld, rows, cols, Wc, Hc, n, k, T, scratch, num_cus, st, &S, &ncols_pad);
    if (rc) return rc;
    // gamma: 1 at beta = 1, a half -- a square root -- at beta = 0
    conv_dense_finish_kernel<<<(unsigned)((cols + 63) / 64), 256, 0, st>>>(scratch, S, KS, ncols_pad, cols, w_side ? Wc : Hc, w_side ? KR : KP4, KP4, k,
                                                                          w_side ? KR : KP4, w_side ? 1 : T, l1, l2, beta ? 0 : 1, flush);
    SMK_HIP(hipGetLastError());
    return 0;
}

int launch_conv_dense_divergence(const void* A, int storage, i64 ld, i64 m, i64 n, const double* Wc, const double* Hc, int k, int T, int beta,
                                 double* scratch, double* out4, double* host_out, int num_cus, hipStream_t st)
{
    if (!conv_dense_args("launch_conv_dense_divergence", m, n, k, T, beta)) return -3;
    int S = 0;
    i64 ncols_pad = 0;
    const int rc = beta ? conv_dense_dispatch<CONV_KL, SIDE_DIV>(A, storage, ld, m, n, Wc, Hc, n, k, T, scratch, num_cus, st, &S, &ncols_pad)
                        : conv_dense_dispatch<CONV_IS, SIDE_DIV>(A, storage, ld, m, n, Wc, Hc, n, k, T, scratch, num_cus, st, &S, &ncols_pad);
    if (rc) return rc;
    double* blockpart = scratch + (size_t)3 * S * ncols_pad;
    const i64 nblk = (n + 255) / 256;
    conv_dense_colsum_kernel<<<(unsigned)nblk, 256, 0, st>>>(scratch, S, ncols_pad, n, blockpart);
    SMK_HIP(hipGetLastError());
    conv_dense_total_kernel<<<1, 1024, 0, st>>>(blockpart, nblk, beta == 0, (double)m * (double)n, out4, host_out);
    SMK_HIP(hipGetLastError());
    return 0;
}

}  // namespace smk
