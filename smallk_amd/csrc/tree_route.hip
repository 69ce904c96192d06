// smallk_amd/csrc/tree_route.hip -- the kernels of a tree router (tree_route.cpp): new documents (the columns of a
// resident sparse matrix) go down a fitted HierNMF2 tree in ONE launch.  At a split with child topic vectors w_l, w_r document a
// goes left iff h0 > h1, (h0, h1) = argmin_{h >= 0} ||a - [w_l w_r] h|| -- tree_partition's rule (hierclust.cpp) on the closed-form
// rank-2 solve of rank2_math.h, side 0: b = (w_l . a, w_r . a) over the stored entries, the left-hand side is the 2 x 2 Gram
// matrix of the pair, prepared once per router (tree_route_prepare_kernel) and read back per level.
//
// Work is cut as in kl_quotient_gather_kernel: SIXTEEN lanes own a document (a wave takes four), walk its entries in chunks of 16
// (coalesced rowidx / val loads, four chunks in flight), gather T[p][row] = (w_l[row], w_r[row]) as one 16-byte load, accumulate b0
// and b1 in fp64 per lane and close with the xor butterfly, so that every lane holds both sums, solves, and steps to the same
// child.  Every sum has a fixed order (chunk order per lane, lane order in the butterfly): the same bits on every run, no
// floating-point atomics.  The descent is bounded by the router's max_depth whatever the tables hold.  A long column takes its
// group longer; there is no wave-per-document path.
#include "tree_route.h"
#include "devutil.h"
#include "rank2_math.h"

namespace smk {

__device__ __forceinline__ double route_group_total(double v)
{
    v += __shfl_xor(v, 8, 64);
    v += __shfl_xor(v, 4, 64);
    v += __shfl_xor(v, 2, 64);
    v += __shfl_xor(v, 1, 64);
    return v;
}

// solve[p] = r2_prepare of the Gram triple of pair p (side 0); bad[p]: its "singular matrix" flag
__global__ __launch_bounds__(64) void tree_route_prepare_kernel(const double* __restrict__ gram, int pairs, R2Solve* __restrict__ solve,
                                                                int* __restrict__ bad)
{
    const int p = blockIdx.x * 64 + threadIdx.x;
    if (p >= pairs) return;
    const R2Solve s = r2_prepare(gram[3 * p], gram[3 * p + 1], gram[3 * p + 2], 0);
    solve[p] = s;
    bad[p] = s.bad ? 1 : 0;
}

__global__ __launch_bounds__(256) void tree_route_kernel(const i64* __restrict__ colptr, const unsigned* __restrict__ rowidx,
                                                         const double* __restrict__ val, i64 n, i64 m, const f64x2_t* __restrict__ T,
                                                         const R2Solve* __restrict__ solve, const int* __restrict__ child_pair,
                                                         const int* __restrict__ pair_nodes, int pairs, int max_depth,
                                                         int* __restrict__ leaf, int* __restrict__ depth, double* __restrict__ h)
{
    constexpr int U = 4;
    const i64 j = (i64)blockIdx.x * 16 + threadIdx.x / 16;
    const int l = threadIdx.x % 16;
    if (j >= n) return;                    // (the sixteen lanes of a group leave together)
    const i64 p0 = colptr[j], p1 = colptr[j + 1];
    int pair = 0, node = 0, d = 0;
    double x0 = 0.0, x1 = 0.0;
    while (d < max_depth && pair >= 0 && pair < pairs) {
        const R2Solve s = solve[pair];
        const f64x2_t* __restrict__ Tp = T + (i64)pair * m;
        double b0 = 0.0, b1 = 0.0;
        for (i64 e = p0; e < p1; e += 16 * U) {
            unsigned ri[U];
            double v[U];
            f64x2_t t[U];
            bool ok[U];
#pragma unroll
            for (int u = 0; u < U; ++u) {
                const i64 q = e + 16 * u + l;
                ok[u] = q < p1;
                const i64 qc = ok[u] ? q : p1 - 1;          // clamped, not predicated: the loads of a batch go out together
                ri[u] = rowidx[qc];
                v[u] = val[qc];
                ok[u] = ok[u] && (i64)ri[u] < m;
            }
#pragma unroll
            for (int u = 0; u < U; ++u) t[u] = Tp[ok[u] ? ri[u] : 0u];
#pragma unroll
            for (int u = 0; u < U; ++u)
                if (ok[u]) { b0 = __builtin_fma(v[u], t[u][0], b0); b1 = __builtin_fma(v[u], t[u][1], b1); }
        }
        b0 = route_group_total(b0);
        b1 = route_group_total(b1);
        r2_apply(s, 0, b0, b1, x0, x1);
        node = pair_nodes[2 * pair + (x0 > x1 ? 0 : 1)];
        ++d;
        pair = child_pair[node];
    }
    if (l == 0) {
        leaf[j] = node;
        if (depth) depth[j] = d;
        if (h) { h[2 * j] = x0; h[2 * j + 1] = x1; }
    }
}

size_t tree_route_solve_bytes() { return sizeof(R2Solve); }

int launch_tree_route_prepare(const double* gram, int pairs, void* solve, int* bad, hipStream_t st)
{
    if (pairs < 1) return 0;
    tree_route_prepare_kernel<<<(pairs + 63) / 64, 64, 0, st>>>(gram, pairs, (R2Solve*)solve, bad);
    SMK_HIP(hipGetLastError());
    return 0;
}

int launch_tree_route(const i64* colptr, const unsigned* rowidx, const double* val, i64 n, i64 m, const double* T, const void* solve,
                      const int* child_pair, const int* pair_nodes, int pairs, int max_depth, int* leaf, int* depth, double* h, hipStream_t st)
{
    if (n < 1) return 0;
    const i64 grid = (n + 15) / 16;
    tree_route_kernel<<<(unsigned)grid, 256, 0, st>>>(colptr, rowidx, val, n, m, (const f64x2_t*)T, (const R2Solve*)solve, child_pair, pair_nodes,
                                                      pairs, max_depth, leaf, depth, h);
    SMK_HIP(hipGetLastError());
    return 0;
}

}  // namespace smk
