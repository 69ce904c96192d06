// smallk_amd/csrc/svd.hip -- the tall-skinny kernels of the truncated SVD and of the NNDSVD start (svd.cpp).
// Every factor here is fp64, column-major KP x N with leading dimension KP = kp_of(l) (l <= 128 live rows): the layout of the
// solver's Wt / H, so that the streaming products, the gather products and launch_gram take them as they are.  The kernels
// mask rows >= l and columns >= N on the way in and write the pad rows as zeros on the way out.  No floating-point atomics:
// every sum is taken in a fixed order and has the same bits on every run.
#include "devutil.h"

namespace smk {

typedef __attribute__((ext_vector_type(4))) double f64x4_t;

// ---------------------------------------------------------------------------------------------------------------------------
// Tall-skinny apply: Xout[:, c] = M' Xin[:, c] for every column c (M: lin x lout, row-major with pitch ldm, staged in LDS).
// A wave takes 16 columns at a time on v_mfma_f64_16x16x4_f64: A = a 16 x 4 slice of M', B = 4 rows x 16 columns of X,
// D[row = (lane >> 4) + 4 reg][column = lane & 15].  Two free permutations make both global accesses 32-byte
// vectors per lane and 128 contiguous bytes per column and quarter wave:
//   * the contraction index is arbitrary as long as A and B agree: at step (Q, e) lane group l4 = lane >> 4 supplies row
//     16 Q + 4 l4 + e, so the four steps of a Q are ONE load of rows 16 Q + 4 l4 .. + 3;
//   * row rho of the A tile carries output row 16 t + 4 (rho & 3) + (rho >> 2), so register r of lane group l4 holds output
//     row 16 t + 4 l4 + r: one store of four consecutive rows.
// A wave reads its 16 columns completely before it writes them and no other wave touches them: Xout may be Xin.
// ---------------------------------------------------------------------------------------------------------------------------
template <int KP>
__global__ __launch_bounds__(256) void svd_apply_kernel(const double* Xin, double* Xout, i64 N, const double* __restrict__ M, int ldm,
                                                        int lin, int lout)
{
    constexpr int NQ = KP >= 16 ? KP / 16 : 1;      // 16-row chunks of the contraction = 16-row tiles of the output
    constexpr int LR = 16 * NQ, LDM = 16 * NQ + 2;
    extern __shared__ double svd_ms[];              // [LR][LDM]; rows >= lin and columns >= lout are zeros
    for (int idx = threadIdx.x; idx < LR * 16 * NQ; idx += 256) {
        const int r = idx / (16 * NQ), c = idx % (16 * NQ);
        svd_ms[r * LDM + c] = (r < lin && c < lout) ? M[(i64)r * ldm + c] : 0.0;
    }
    __syncthreads();
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, l15 = lane & 15, l4 = lane >> 4;
    const int perm = 4 * (l15 & 3) + (l15 >> 2);
    const i64 ntiles = (N + 15) / 16;
    const int row0 = 4 * l4;
    for (i64 tile = (i64)blockIdx.x * 4 + wave; tile < ntiles; tile += (i64)gridDim.x * 4) {
        const i64 col = tile * 16 + l15;
        const bool live = col < N;
        f64x4_t xb[NQ];
#pragma unroll
        for (int Q = 0; Q < NQ; ++Q) {
            xb[Q] = f64x4_t{0.0, 0.0, 0.0, 0.0};
            const int r = 16 * Q + row0;
            if (live && r + 3 < KP && r < lin) {
                const f64x4_t v = *(const f64x4_t*)(Xin + col * KP + r);
#pragma unroll
                for (int e = 0; e < 4; ++e) xb[Q][e] = (r + e < lin) ? v[e] : 0.0;     // a select: pad rows may hold anything
            }
        }
        f64x4_t acc[NQ];
#pragma unroll
        for (int t = 0; t < NQ; ++t) acc[t] = f64x4_t{0.0, 0.0, 0.0, 0.0};
#pragma unroll
        for (int Q = 0; Q < NQ; ++Q)
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                const double* mrow = svd_ms + (16 * Q + row0 + e) * LDM + perm;
#pragma unroll
                for (int t = 0; t < NQ; ++t) acc[t] = __builtin_amdgcn_mfma_f64_16x16x4f64(mrow[16 * t], xb[Q][e], acc[t], 0, 0, 0);
            }
#pragma unroll
        for (int t = 0; t < NQ; ++t) {
            const int r = 16 * t + row0;
            if (live && r + 3 < KP) *(f64x4_t*)(Xout + col * KP + r) = acc[t];
        }
    }
}

template <int KP>
static int launch_svd_apply_t(const double* Xin, double* Xout, i64 N, const double* M, int ldm, int lin, int lout, int num_cus, hipStream_t st)
{
    constexpr int NQ = KP >= 16 ? KP / 16 : 1;
    constexpr int lds = 16 * NQ * (16 * NQ + 2) * (int)sizeof(double);
    if constexpr (lds > 64 * 1024) {
        static std::atomic<unsigned long long> attr_set{0};       // per device (DeviceOnce)
        if (DeviceOnce once{attr_set}) {
            SMK_HIP(hipFuncSetAttribute((const void*)svd_apply_kernel<KP>, hipFuncAttributeMaxDynamicSharedMemorySize, lds));
            once.done();
        }
    }
    const i64 ntiles = (N + 15) / 16;
    i64 grid = (ntiles + 3) / 4;
    const i64 cap = (i64)num_cus * (lds > 64 * 1024 ? 1 : 4);
    if (grid > cap) grid = cap;
    if (grid < 1) return 0;
    svd_apply_kernel<KP><<<(unsigned)grid, 256, lds, st>>>(Xin, Xout, N, M, ldm, lin, lout);
    SMK_HIP(hipGetLastError());
    return 0;
}

// The same apply that also leaves the Gram matrix of its OUTPUT as one partial sum per workgroup (Gp: [gridDim.x][KP * KP], what
// launch_gram_reduce adds up in order), so that the second orthonormalisation round needs no pass over the factor for its Gram
// matrix.  A wave's 16 x KP output tile goes through LDS to become both MFMA operands (rows x 4 columns per step); the upper
// triangle of 16 x 16 tiles is accumulated in registers over all tiles of the wave, the four waves are joined in LDS in wave
// order, both triangles are written.  KP = 16 / 32 / 64 (at 128 the 36 accumulator tiles do not fit the registers).
template <int KP>
__global__ __launch_bounds__(256) void svd_apply_gram_kernel(const double* Xin, double* Xout, i64 N, const double* __restrict__ M, int ldm,
                                                             int lin, int lout, double* __restrict__ Gp)
{
    constexpr int NQ = KP / 16, LDM = KP + 2, NT = NQ * (NQ + 1) / 2;
    extern __shared__ double svd_ms[];              // [KP][LDM] M, then [4][16][LDM] the waves' output tiles
    double* ot = svd_ms + KP * LDM + (threadIdx.x >> 6) * 16 * LDM;
    for (int idx = threadIdx.x; idx < KP * KP; idx += 256) {
        const int r = idx / KP, c = idx % KP;
        svd_ms[r * LDM + c] = (r < lin && c < lout) ? M[(i64)r * ldm + c] : 0.0;
    }
    __syncthreads();
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, l15 = lane & 15, l4 = lane >> 4;
    const int perm = 4 * (l15 & 3) + (l15 >> 2);
    const i64 ntiles = (N + 15) / 16;
    const int row0 = 4 * l4;
    f64x4_t g[NT];
#pragma unroll
    for (int i = 0; i < NT; ++i) g[i] = f64x4_t{0.0, 0.0, 0.0, 0.0};
    for (i64 base = (i64)blockIdx.x * 4; base < ntiles; base += (i64)gridDim.x * 4) {       // the same trip count for every wave
        const i64 col = (base + wave) * 16 + l15;
        const bool live = col < N;
        f64x4_t xb[NQ];
#pragma unroll
        for (int Q = 0; Q < NQ; ++Q) {
            xb[Q] = f64x4_t{0.0, 0.0, 0.0, 0.0};
            const int r = 16 * Q + row0;
            if (live && r < lin) {
                const f64x4_t v = *(const f64x4_t*)(Xin + col * KP + r);
#pragma unroll
                for (int e = 0; e < 4; ++e) xb[Q][e] = (r + e < lin) ? v[e] : 0.0;
            }
        }
        f64x4_t acc[NQ];
#pragma unroll
        for (int t = 0; t < NQ; ++t) acc[t] = f64x4_t{0.0, 0.0, 0.0, 0.0};
#pragma unroll
        for (int Q = 0; Q < NQ; ++Q)
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                const double* mrow = svd_ms + (16 * Q + row0 + e) * LDM + perm;
#pragma unroll
                for (int t = 0; t < NQ; ++t) acc[t] = __builtin_amdgcn_mfma_f64_16x16x4f64(mrow[16 * t], xb[Q][e], acc[t], 0, 0, 0);
            }
#pragma unroll
        for (int t = 0; t < NQ; ++t) {
            if (live) *(f64x4_t*)(Xout + col * KP + 16 * t + row0) = acc[t];
#pragma unroll
            for (int e = 0; e < 4; ++e) ot[l15 * LDM + 16 * t + row0 + e] = acc[t][e];      // a dead column is a column of zeros
        }
        __syncthreads();
#pragma unroll
        for (int c = 0; c < 4; ++c) {
            double op[NQ];
#pragma unroll
            for (int t = 0; t < NQ; ++t) op[t] = ot[(4 * c + l4) * LDM + 16 * t + l15];
            int i = 0;
#pragma unroll
            for (int ta = 0; ta < NQ; ++ta)
#pragma unroll
                for (int tb = ta; tb < NQ; ++tb, ++i) g[i] = __builtin_amdgcn_mfma_f64_16x16x4f64(op[ta], op[tb], g[i], 0, 0, 0);
        }
        __syncthreads();
    }
    // join the waves in wave order in LDS (M is no longer needed), then one coalesced store of the workgroup's partial sum
    double* red = svd_ms;
    for (int w = 0; w < 4; ++w) {
        if (wave == w) {
            int i = 0;
#pragma unroll
            for (int ta = 0; ta < NQ; ++ta)
#pragma unroll
                for (int tb = ta; tb < NQ; ++tb, ++i)
#pragma unroll
                    for (int r = 0; r < 4; ++r) {
                        const int a = 16 * ta + l4 + 4 * r, b = 16 * tb + l15;
                        const double v = (w == 0 ? 0.0 : red[a * KP + b]) + g[i][r];
                        red[a * KP + b] = v;
                        if (ta != tb) red[b * KP + a] = v;
                    }
        }
        __syncthreads();
    }
    for (int idx = threadIdx.x; idx < KP * KP; idx += 256) Gp[(i64)blockIdx.x * KP * KP + idx] = red[idx];
}

int svd_apply_gram_blocks(int KPv, i64 N, int num_cus)
{
    if (KPv != 16 && KPv != 32 && KPv != 64) return 0;
    i64 grid = ((N + 15) / 16 + 3) / 4;
    const i64 cap = (i64)num_cus * (KPv == 64 ? 2 : 4);
    if (grid > cap) grid = cap;
    return (int)grid;
}

template <int KP>
static int launch_svd_apply_gram_t(const double* Xin, double* Xout, i64 N, const double* M, int ldm, int lin, int lout, double* Gp, int grid, hipStream_t st)
{
    constexpr int lds = (KP + 64) * (KP + 2) * (int)sizeof(double);
    static std::atomic<unsigned long long> attr_set{0};       // per device (DeviceOnce)
    if (DeviceOnce once{attr_set}) {
        SMK_HIP(hipFuncSetAttribute((const void*)svd_apply_gram_kernel<KP>, hipFuncAttributeMaxDynamicSharedMemorySize, lds));
        once.done();
    }
    svd_apply_gram_kernel<KP><<<(unsigned)grid, 256, lds, st>>>(Xin, Xout, N, M, ldm, lin, lout, Gp);
    SMK_HIP(hipGetLastError());
    return 0;
}

// *nblk_out partial sums in Gp (svd_apply_gram_blocks(..) x KP x KP doubles); returns 1 when this padded rank has no fused kernel
int launch_svd_apply_gram(const double* Xin, double* Xout, int KPv, i64 N, const double* M, int ldm, int lin, int lout, double* Gp, int* nblk_out,
                          int num_cus, hipStream_t st)
{
    const int grid = svd_apply_gram_blocks(KPv, N, num_cus);
    if (grid < 1) return 1;
    if (lin < 0 || lout < 0 || lin > KPv || lout > KPv || ldm < lout) { set_error("svd apply: M does not fit the factor"); return -100; }
    *nblk_out = grid;
    switch (KPv) {
        case 16: return launch_svd_apply_gram_t<16>(Xin, Xout, N, M, ldm, lin, lout, Gp, grid, st);
        case 32: return launch_svd_apply_gram_t<32>(Xin, Xout, N, M, ldm, lin, lout, Gp, grid, st);
        default: return launch_svd_apply_gram_t<64>(Xin, Xout, N, M, ldm, lin, lout, Gp, grid, st);
    }
}

int launch_svd_apply(const double* Xin, double* Xout, int KPv, i64 N, const double* M, int ldm, int lin, int lout, int num_cus, hipStream_t st)
{
    if (KPv != 8 && KPv != 16 && KPv != 32 && KPv != 64 && KPv != 128) { set_error("svd apply: padded rank must be 8 .. 128"); return -100; }
    if (lin < 0 || lout < 0 || lin > KPv || lout > KPv || ldm < lout) { set_error("svd apply: M does not fit the factor"); return -100; }
    KP_DISPATCH128(KPv, return launch_svd_apply_t<KP>(Xin, Xout, N, M, ldm, lin, lout, num_cus, st));
    return 0;
}

// ---------------------------------------------------------------------------------------------------------------------------
// The test matrix Omega (n x l) in the factor layout (l rows of a KP x n factor): the project's counter-based uniform values,
// entry (j, r) keyed by j * l + r, centred to [-0.5, 0.5) -- a non-negative Omega against a non-negative A puts every column
// of A Omega next to A 1.  Pad rows are written as zeros.
// ---------------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void svd_fill_centred_kernel(double* __restrict__ X, int KP, int l, i64 N, unsigned long long seed)
{
    const i64 total = N * KP;
    for (i64 idx = (i64)blockIdx.x * blockDim.x + threadIdx.x; idx < total; idx += (i64)gridDim.x * blockDim.x) {
        const i64 j = idx / KP;
        const int r = (int)(idx % KP);
        X[idx] = r < l ? (double)uniform_value(seed, (uint64_t)(j * l + r), 0) - 0.5 : 0.0;
    }
}

int launch_svd_fill_centred(double* X, int KP, int l, i64 N, unsigned long long seed, hipStream_t st)
{
    i64 grid = (N * KP + 255) / 256;
    if (grid > 4096) grid = 4096;
    if (grid < 1) return 0;
    svd_fill_centred_kernel<<<(unsigned)grid, 256, 0, st>>>(X, KP, l, N, seed);
    SMK_HIP(hipGetLastError());
    return 0;
}

// ---------------------------------------------------------------------------------------------------------------------------
// NNDSVD split, stage 1 and 2: per component (factor row) the sum of squares of the positive entries, of the negative entries,
// the largest positive entry and the largest magnitude of a negative one, over the N columns.  Stage 1: a workgroup takes a
// contiguous range of columns, thread (r, cl) every CL-th column of it, the CL column lanes are joined in LDS in order.
// Stage 2: one thread per component walks the workgroups' partials in order.  part: [nblk][4][KP], out: [4][KP].
// ---------------------------------------------------------------------------------------------------------------------------
template <int KP>
__global__ __launch_bounds__(256) void nndsvd_stats_kernel(const double* __restrict__ X, i64 N, int k, i64 cpb, double* __restrict__ part)
{
    constexpr int CL = 256 / KP;
    __shared__ double sh[4][256];
    const int r = threadIdx.x % KP, cl = threadIdx.x / KP;
    const i64 c0 = (i64)blockIdx.x * cpb;
    i64 c1 = c0 + cpb;
    if (c1 > N) c1 = N;
    double sp = 0.0, sn = 0.0, mp = 0.0, mn = 0.0;
    if (r < k)
        for (i64 c = c0 + cl; c < c1; c += CL) {
            const double x = X[c * KP + r];
            if (x > 0.0) { sp += x * x; mp = x > mp ? x : mp; }
            else if (x < 0.0) { sn += x * x; mn = -x > mn ? -x : mn; }
        }
    sh[0][threadIdx.x] = sp; sh[1][threadIdx.x] = sn; sh[2][threadIdx.x] = mp; sh[3][threadIdx.x] = mn;
    __syncthreads();
    if (cl == 0) {
        for (int u = 1; u < CL; ++u) {
            sp += sh[0][u * KP + r];
            sn += sh[1][u * KP + r];
            mp = sh[2][u * KP + r] > mp ? sh[2][u * KP + r] : mp;
            mn = sh[3][u * KP + r] > mn ? sh[3][u * KP + r] : mn;
        }
        double* o = part + (i64)blockIdx.x * 4 * KP;
        o[r] = sp; o[KP + r] = sn; o[2 * KP + r] = mp; o[3 * KP + r] = mn;
    }
}

__global__ __launch_bounds__(128) void nndsvd_stats_sum_kernel(const double* __restrict__ part, int nblk, int KP, double* __restrict__ out)
{
    const int r = threadIdx.x;
    if (r >= KP) return;
    double sp = 0.0, sn = 0.0, mp = 0.0, mn = 0.0;
    for (int b = 0; b < nblk; ++b) {
        const double* p = part + (i64)b * 4 * KP;
        sp += p[r];
        sn += p[KP + r];
        mp = p[2 * KP + r] > mp ? p[2 * KP + r] : mp;
        mn = p[3 * KP + r] > mn ? p[3 * KP + r] : mn;
    }
    out[r] = sp; out[KP + r] = sn; out[2 * KP + r] = mp; out[3 * KP + r] = mn;
}

int nndsvd_stats_blocks(i64 N) { const i64 b = (N + 1023) / 1024; return (int)(b < 1 ? 1 : b > 512 ? 512 : b); }
size_t nndsvd_stats_scratch_elems(int KP, i64 N) { return (size_t)nndsvd_stats_blocks(N) * 4 * KP; }

int launch_nndsvd_stats(const double* X, int KPv, int k, i64 N, double* scratch, double* out, hipStream_t st)
{
    const int nblk = nndsvd_stats_blocks(N);
    const i64 cpb = (N + nblk - 1) / nblk;
    KP_DISPATCH128(KPv, (nndsvd_stats_kernel<KP><<<nblk, 256, 0, st>>>(X, N, k, cpb, scratch)));
    SMK_HIP(hipGetLastError());
    nndsvd_stats_sum_kernel<<<1, 128, 0, st>>>(scratch, nblk, KPv, out);
    SMK_HIP(hipGetLastError());
    return 0;
}

// NNDSVD write, in place: component r of every column becomes part * scale[r], where part = |x| (mode 2), max(x, 0) (mode 1),
// max(-x, 0) (mode -1) or nothing (mode 0); a part below thr[r] is an exact zero, and every zero is replaced by `fill` (the
// mean of A under nndsvda, 0 otherwise).  prm: [3][KP] = mode, scale, thr.  Pad rows are written as zeros.
__global__ __launch_bounds__(256) void nndsvd_write_kernel(double* __restrict__ X, int KP, int k, i64 N, const double* __restrict__ prm, double fill)
{
    const i64 total = N * KP;
    for (i64 idx = (i64)blockIdx.x * blockDim.x + threadIdx.x; idx < total; idx += (i64)gridDim.x * blockDim.x) {
        const int r = (int)(idx % KP);
        double v = 0.0;
        if (r < k) {
            const double x = X[idx], mode = prm[r];
            double part = 0.0;
            if (mode == 2.0) part = fabs(x);
            else if (mode == 1.0) part = x > 0.0 ? x : 0.0;
            else if (mode == -1.0) part = x < 0.0 ? -x : 0.0;
            v = part < prm[2 * KP + r] ? 0.0 : part * prm[KP + r];
            if (!(v > 0.0)) v = fill;
        }
        X[idx] = v;
    }
}

int launch_nndsvd_write(double* X, int KP, int k, i64 N, const double* prm, double fill, hipStream_t st)
{
    i64 grid = (N * KP + 255) / 256;
    if (grid > 4096) grid = 4096;
    if (grid < 1) return 0;
    nndsvd_write_kernel<<<(unsigned)grid, 256, 0, st>>>(X, KP, k, N, prm, fill);
    SMK_HIP(hipGetLastError());
    return 0;
}

// ---------------------------------------------------------------------------------------------------------------------------
// Sum of the stored entries (mean(A) of nndsvda), fixed order: workgroup b sums the columns b, b + grid, ... of a column-major
// array (rows x cols, pitch ld, entries past `total` elements do not exist), thread t the rows t, t + 256, ...; the workgroups'
// sums are then added in order by launch_sum_partials.  Dense A: its stored fp32 / bf16 values; sparse A: `val` cut into
// columns of 65536 entries (duplicates add, absent entries are zeros).
// ---------------------------------------------------------------------------------------------------------------------------
template <typename T>
__global__ __launch_bounds__(256) void sum_entries_kernel(const T* __restrict__ A, i64 ld, i64 rows, i64 cols, i64 total, double* __restrict__ part)
{
    __shared__ double sh[16];
    double s = 0.0;
    for (i64 j = blockIdx.x; j < cols; j += gridDim.x)
        for (i64 r = threadIdx.x; r < rows; r += 256) {
            const i64 i = j * ld + r;
            if (i >= total) break;
            if constexpr (sizeof(T) == 2) s += (double)bf16_bits_to_f32(A[i]);
            else s += (double)A[i];
        }
    const double t = block_sum(s, sh);
    if (threadIdx.x == 0) part[blockIdx.x] = t;
}

int sum_entries_blocks(i64 cols) { return (int)(cols < 1 ? 1 : cols > 2048 ? 2048 : cols); }

int launch_sum_entries_dense(const void* A, int storage, i64 ld, i64 rows, i64 cols, double* part, double* out, hipStream_t st)
{
    const int nblk = sum_entries_blocks(cols);
    const i64 total = ld * cols;
    if (storage == STORE_BF16) sum_entries_kernel<unsigned short><<<nblk, 256, 0, st>>>((const unsigned short*)A, ld, rows, cols, total, part);
    else sum_entries_kernel<float><<<nblk, 256, 0, st>>>((const float*)A, ld, rows, cols, total, part);
    SMK_HIP(hipGetLastError());
    return launch_sum_partials(part, nblk, out, st);
}

int launch_sum_entries_sparse(const double* val, i64 nnz, double* part, double* out, hipStream_t st)
{
    const i64 chunk = 65536, cols = (nnz + chunk - 1) / chunk;
    const int nblk = sum_entries_blocks(cols);
    sum_entries_kernel<double><<<nblk, 256, 0, st>>>(val, chunk, chunk, cols, nnz, part);
    SMK_HIP(hipGetLastError());
    return launch_sum_partials(part, nblk, out, st);
}

}  // namespace smk
