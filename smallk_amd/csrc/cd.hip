// smallk_amd/csrc/cd.hip -- one sweep of cyclic coordinate descent over a factor (cd.cpp): scikit-learn's
// solver="cd" without the shuffle, with its L1 / L2 penalties.  The factor is fp64, column-major KP x N with leading dimension
// KP = kp_of(k), the layout of the solver's Wt / H; its columns are independent problems.  For every column x and t = 0 .. k-1
// in order, with G' = G + l2 I and R' = R - l1:
//     grad = sum_r G'[t, r] x[r] - R'[t]            (entries of x already updated in this sweep are used)
//     pg   = x[t] == 0 ? min(0, grad) : grad,       violation += |pg|
//     x[t] = max(x[t] - grad / G'[t, t], 0)         unless G'[t, t] == 0: then x[t] stays (its pg still counts)
// The violation leaves the launch as one partial sum per workgroup, added up in a fixed order (block_sum), and
// launch_cd_violation adds the partials in a fixed order: the same bits on every run, no floating-point atomics.
// Rows >= k of the factor, of G and of R never enter grad or the violation, whatever they hold; the factor's are written as zeros.
#include "devutil.h"

namespace smk {

// gs[t * KP + r] = G'[t, r] for t, r < k, zero elsewhere.  G: KP x KP, G[t * KP + r] = G[t, r].
template <int KP>
__device__ __forceinline__ void cd_stage_gram(double* gs, const double* __restrict__ G, int k, double l2)
{
    for (int i = threadIdx.x; i < KP * KP; i += blockDim.x) {
        const int t = i / KP, r = i % KP;
        double v = (t < k && r < k) ? G[i] : 0.0;
        if (t == r && t < k) v += l2;
        gs[i] = v;
    }
    __syncthreads();
}

// the coordinate step of the lane that owns x[t]: returns the new value, adds |pg| to viol
__device__ __forceinline__ double cd_step(double xt, double grad, double gtt, double& viol)
{
    const double pg = xt == 0.0 ? fmin(grad, 0.0) : grad;
    viol += fabs(pg);
    return gtt != 0.0 ? fmax(xt - grad / gtt, 0.0) : xt;
}

// MG = false: the column-tile pattern of hals_sweep_kernel -- LPC = KP / 4 adjacent lanes per column, four values each; per step a
//   32-byte LDS read of row t of G' (the same address across the columns of a wave), four multiply-adds and a DPP group sum.
// MG = true: the maintained gradient -- g = G' x - R' lives in the registers of the lanes that own its rows; per step the owner of t
//   forms delta = x_new - x_old, one cross-lane broadcast hands it to the group, every lane adds delta G'[:, t] (row t: G' is taken
//   as symmetric).  No reduction tree, but k broadcast steps up front to form g.
template <int KP, bool MG>
__global__ __launch_bounds__(256) void cd_sweep_kernel(double* __restrict__ X, int k, i64 N, PartialView R, const double* __restrict__ G,
                                                       double l1, double l2, double* __restrict__ viol_partials)
{
    constexpr int LPC = KP / 4;
    extern __shared__ __attribute__((aligned(16))) double gs[];   // KP * KP doubles
    __shared__ double sh[4];
    cd_stage_gram<KP>(gs, G, k, l2);
    const i64 gtid = (i64)blockIdx.x * blockDim.x + threadIdx.x;
    const i64 j = gtid / LPC;
    const int s = (int)(gtid % LPC);
    const bool valid = j < N;
    const i64 jc = valid ? j : (N - 1);          // whole waves take part in the cross-lane moves
    double x[4], b[4], viol = 0.0;
    load4(X + jc * KP + 4 * s, x);
    load_rhs4(R, jc, 4 * s, b);
#pragma unroll
    for (int e = 0; e < 4; ++e) {
        if (4 * s + e >= k) x[e] = 0.0;          // a select: pad rows may hold anything
        b[e] = (4 * s + e < k) ? b[e] - l1 : 0.0;
    }
    if constexpr (!MG) {
#pragma unroll
        for (int t = 0; t < KP; ++t) {
            if (t < k) {
                double g[4];
                load4(gs + t * KP + 4 * s, g);
                const double dot = group_sum<LPC>((g[0] * x[0] + g[1] * x[1]) + (g[2] * x[2] + g[3] * x[3]));
                if (s == t / 4) x[t % 4] = cd_step(x[t % 4], dot - b[t % 4], gs[t * KP + t], viol);
            }
        }
    } else {
        const int base = (threadIdx.x & 63) & ~(LPC - 1);        // first lane of this column's group
        double g[4] = {-b[0], -b[1], -b[2], -b[3]};
#pragma unroll
        for (int r = 0; r < KP; ++r) {
            if (r < k) {
                const double xr = __shfl(x[r % 4], base + r / 4, 64);
                double gr[4];
                load4(gs + r * KP + 4 * s, gr);
#pragma unroll
                for (int e = 0; e < 4; ++e) g[e] = __builtin_fma(gr[e], xr, g[e]);
            }
        }
#pragma unroll
        for (int t = 0; t < KP; ++t) {
            if (t < k) {
                double delta = 0.0;
                if (s == t / 4) {
                    const double xn = cd_step(x[t % 4], g[t % 4], gs[t * KP + t], viol);
                    delta = xn - x[t % 4];
                    x[t % 4] = xn;
                }
                delta = __shfl(delta, base + t / 4, 64);
                double gt[4];
                load4(gs + t * KP + 4 * s, gt);
#pragma unroll
                for (int e = 0; e < 4; ++e) g[e] = __builtin_fma(gt[e], delta, g[e]);
            }
        }
    }
    if (valid) store4(X + j * KP + 4 * s, x);
    const double tot = block_sum(valid ? viol : 0.0, sh);
    if (threadIdx.x == 0) viol_partials[blockIdx.x] = tot;
}

// out[0] = host_out[0] = the sum of n partials (block_sum_array's fixed order); host_out: pinned host memory or null
__global__ __launch_bounds__(256) void cd_violation_kernel(const double* __restrict__ part, int n, double* __restrict__ out, double* host_out)
{
    __shared__ double sh[12];
    const double t = block_sum_array(part, n, sh);
    if (threadIdx.x == 0) {
        out[0] = t;
        if (host_out) host_out[0] = t;
    }
}

int cd_sweep_blocks(int k, i64 N) { return (int)((N * (kp_of(k) / 4) + 255) / 256); }

template <int KP, bool MG>
static int launch_cd_sweep_t(double* X, int k, i64 N, PartialView R, const double* G, double l1, double l2, double* viol_partials, hipStream_t st)
{
    const int lds = KP * KP * (int)sizeof(double);
    if (lds > 48 * 1024) SMK_HIP(hipFuncSetAttribute((const void*)cd_sweep_kernel<KP, MG>, hipFuncAttributeMaxDynamicSharedMemorySize, lds));
    cd_sweep_kernel<KP, MG><<<cd_sweep_blocks(k, N), 256, lds, st>>>(X, k, N, R, G, l1, l2, viol_partials);
    SMK_HIP(hipGetLastError());
    return 0;
}

int launch_cd_sweep(double* X, int k, i64 N, PartialView R, const double* G, double l1, double l2, double* viol_partials, hipStream_t st,
                    int maintained)
{
    if (k < 1 || k > 128 || N < 1) { set_error("launch_cd_sweep: k in [1, 128] and N >= 1"); return -3; }
    const int KPv = kp_of(k);
    if (maintained) { KP_DISPATCH128(KPv, return (launch_cd_sweep_t<KP, true>(X, k, N, R, G, l1, l2, viol_partials, st))); }
    KP_DISPATCH128(KPv, return (launch_cd_sweep_t<KP, false>(X, k, N, R, G, l1, l2, viol_partials, st)));
    return 0;
}

int launch_cd_violation(const double* partials, int n, double* out, double* host_out, hipStream_t st)
{
    cd_violation_kernel<<<1, 256, 0, st>>>(partials, n, out, host_out);
    SMK_HIP(hipGetLastError());
    return 0;
}

}  // namespace smk
