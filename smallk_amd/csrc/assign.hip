// smallk_amd/csrc/assign.hip -- what a clustering user does with finished factors, on the device: the label and
// the memberships of every document (column of H), and the top terms of every topic (column of W).  The factors are read as fp64
// or fp32 in their "k-direction contiguous" layout -- column c of H at H + c * ld, row i of W at W + i * ld: the solver's resident
// H and Wt, a column-major H tensor, a row-major W tensor -- and widened to fp64 before anything is compared.  The comparisons are
// those of the host functions (flatclust.cpp: smk_compute_assignments, smk_compute_fuzzy_assignments, smk_top_terms) in the same
// order, so labels and top terms are the same integers and the memberships the same bits.  No floating-point atomics; every
// result is the same on every run and for every grid size.
#include "common.h"

#include <hipcub/hipcub.hpp>

namespace smk {

// ---- labels and memberships ------------------------------------------------------------------------------------------------
// A workgroup owns 256 consecutive columns and walks down them in strips of 16 rows: the strip is read cooperatively (sixteen
// consecutive lanes take the 16 consecutive elements of one column: whole 128-byte lines of fp64), stored in LDS with a pitch of
// 17 doubles (lane c reading its own column: 34 c mod 64 is a different bank pair for each lane of a half wave), and lane c then
// scans column c in increasing r -- `col[r] > mx` and `sum += col[r]` exactly as on the host.  Rows from k on are never read:
// the pad rows of a resident H are no candidates.  Memberships take a second walk (the sum must be complete first); with one
// strip (k <= 16) the strip is still in LDS and H is read once.
static constexpr int LAB_COLS = 256, LAB_ROWS = 16, LAB_PITCH = LAB_ROWS + 1;

template <typename T>
__global__ __launch_bounds__(256) void labels_kernel(const T* __restrict__ H, i64 ldc, int k, i64 n, unsigned* __restrict__ labels,
                                                     float* __restrict__ memb)
{
    __shared__ double sh[LAB_COLS * LAB_PITCH];
    __shared__ double inv_s[LAB_COLS];
    const i64 c0 = (i64)blockIdx.x * LAB_COLS;
    const int t = threadIdx.x;
    const i64 c = c0 + t;
    const int nstrip = (k + LAB_ROWS - 1) / LAB_ROWS;
    auto stage = [&](int r0) {
        for (int idx = t; idx < LAB_COLS * LAB_ROWS; idx += 256) {
            const int cl = idx / LAB_ROWS, r = idx % LAB_ROWS;
            if (c0 + cl < n && r0 + r < k) sh[cl * LAB_PITCH + r] = (double)H[(c0 + cl) * ldc + r0 + r];
        }
    };
    double mx = 0.0, sum = 0.0;
    unsigned best = 0;
    for (int s = 0; s < nstrip; ++s) {
        const int r0 = s * LAB_ROWS;
        if (s > 0) __syncthreads();                       // every lane has read the strip before
        stage(r0);
        __syncthreads();
        if (c < n) {
            const int re = k - r0 < LAB_ROWS ? k - r0 : LAB_ROWS;
            for (int r = 0; r < re; ++r) {
                const double v = sh[t * LAB_PITCH + r];
                sum += v;
                if (r0 + r == 0) mx = v;
                else if (v > mx) { mx = v; best = (unsigned)(r0 + r); }
            }
        }
    }
    if (c < n) labels[c] = best;
    if (!memb) return;                                    // (the same for every thread)
    inv_s[t] = 1.0 / sum;                                 // an all-zero column: inf, and 0 * inf = NaN as on the host
    for (int s = 0; s < nstrip; ++s) {
        const int r0 = s * LAB_ROWS;
        if (nstrip > 1) { __syncthreads(); stage(r0); }
        __syncthreads();
        for (int idx = t; idx < LAB_COLS * LAB_ROWS; idx += 256) {
            const int cl = idx / LAB_ROWS, r = idx % LAB_ROWS;
            if (c0 + cl < n && r0 + r < k) memb[(c0 + cl) * k + r0 + r] = (float)(sh[cl * LAB_PITCH + r] * inv_s[cl]);
        }
    }
}

// H: fp64 / fp32, column c at H + c * ldc (elements); labels: n; memb: k * n floats, document c at c * k, or null
int launch_labels(const void* H, int dtype, i64 ldc, int k, i64 n, unsigned* labels, float* memb, hipStream_t st)
{
    const i64 blocks = (n + LAB_COLS - 1) / LAB_COLS;
    if (blocks > 0x7FFFFFFFll) { set_error("labels: too many columns for one launch"); return -100; }
    if (dtype == DT_F64) labels_kernel<double><<<(unsigned)blocks, 256, 0, st>>>((const double*)H, ldc, k, n, labels, memb);
    else if (dtype == DT_F32) labels_kernel<float><<<(unsigned)blocks, 256, 0, st>>>((const float*)H, ldc, k, n, labels, memb);
    else { set_error("labels: factors are fp64 or fp32"); return -3; }
    SMK_HIP(hipGetLastError());
    return 0;
}

// ---- top terms ---------------------------------------------------------------------------------------------------------------
// The order of the host's partial_sort: a before b when d[a] > d[b] || (d[a] == d[b] && a < b).  With distinct indices it is a
// strict total order on everything but NaN (-0.0 == +0.0 as on the host), so "the best cnt of a set" does not depend on the order
// in which the set was seen.
__device__ __forceinline__ bool tt_before(double va, unsigned ia, double vb, unsigned ib) { return va > vb || (va == vb && ia < ib); }

static constexpr int TT_TOPICS = 16;                 // topics of a workgroup: 16 consecutive fp64 of a row of W = one 128-byte line
static constexpr int TT_TILE = 256;                  // rows of a tile: 16 steps of 16 rows (a lane: one topic, every 16th row)
static constexpr unsigned TT_NONE = 0xFFFFFFFFu;     // index of a slot that holds nothing (value -inf: after every real entry)

// slots per topic of the in-LDS selection: a power of two (the sort), at least cnt kept + 112 incoming (7 steps of 16 rows)
static inline int tt_slots(int cnt) { int p = 128; while (p < cnt + 112) p <<= 1; return p; }
static inline size_t tt_lds_bytes(int P) { return (size_t)TT_TOPICS * P * (sizeof(double) + sizeof(unsigned)) + TT_TOPICS * sizeof(int); }

// Selection: a workgroup owns the rows [g * rows_per_chunk, ...) and 16 consecutive topics.  Per topic it keeps P slots in LDS.
// An element enters (an integer LDS counter hands out the slot) when it comes before the topic's threshold, the cnt-th best of
// the last compaction (-inf before the first).  Before a run of `qs` steps (16 rows each) could overflow a topic's slots, all
// topics are compacted: padded with empty slots, sorted by tt_before (bitonic, in LDS), cut to the best cnt, thresholds renewed.
// An element that does not enter has cnt elements before it, so it is not among the best cnt; the end result is the sorted best
// cnt of the chunk whatever order the slots were filled in.  (P: tt_slots; qs: 7 or 4, cnt + 16 qs <= P.)
// idx_in == null: the row number is the index (stage one, reading W).  Otherwise rows are candidates of stage one, [row][k] values
// with their indices in idx_in at the same place (stage two).
// out != null: the workgroup writes final results, out[j * maxterms + q]; else candidates cand_val / cand_idx [(g * cnt + q) * k + j].
template <typename T>
__global__ __launch_bounds__(256) void topterms_select_kernel(const T* __restrict__ W, i64 ld, const unsigned* __restrict__ idx_in,
                                                              i64 nrows, int k, int cnt, int P, int qs, i64 rows_per_chunk,
                                                              double* __restrict__ cand_val, unsigned* __restrict__ cand_idx,
                                                              int* __restrict__ out, int maxterms)
{
    extern __shared__ __attribute__((aligned(16))) unsigned char tt_lds[];
    double* bv = (double*)tt_lds;                                   // [16][P]
    unsigned* bi = (unsigned*)(bv + (size_t)TT_TOPICS * P);         // [16][P]
    int* count = (int*)(bi + (size_t)TT_TOPICS * P);                // [16]
    const int t = threadIdx.x, tj = t & 15, tr = t >> 4;
    const int j0 = (int)blockIdx.y * TT_TOPICS;
    const int jt = j0 + tj;
    const bool topic_in = jt < k;
    const int jc = topic_in ? jt : k - 1;
    const i64 i0 = (i64)blockIdx.x * rows_per_chunk;
    i64 i1 = i0 + rows_per_chunk;
    if (i1 > nrows) i1 = nrows;
    if (t < TT_TOPICS) count[t] = 0;
    double tv = -__builtin_inf();
    unsigned ti = TT_NONE;

    // (after a barrier)  Only the occupied front of the slots is sorted: Ps = the power of two that holds the fullest topic (and cnt).
    auto compact = [&]() {
        int mc = cnt;
#pragma unroll
        for (int tp = 0; tp < TT_TOPICS; ++tp) mc = count[tp] > mc ? count[tp] : mc;
        int Ps = 2, lg = 1;
        while (Ps < mc && Ps < P) { Ps <<= 1; ++lg; }
        // empty slots behind the entries, then the bitonic network on all 16 topics at once, best first
        for (int e = t; e < TT_TOPICS * Ps; e += 256) {
            const int tp = e >> lg, sl = e & (Ps - 1);
            if (sl >= count[tp]) { bv[tp * P + sl] = -__builtin_inf(); bi[tp * P + sl] = TT_NONE; }
        }
        __syncthreads();
        const int half = Ps >> 1, lgh = lg - 1;
        for (int size = 2; size <= Ps; size <<= 1) {
            for (int stride = size >> 1; stride > 0; stride >>= 1) {
                for (int e = t; e < TT_TOPICS * half; e += 256) {
                    const int tp = e >> lgh, pr = e & (half - 1);
                    const int a = ((pr & ~(stride - 1)) << 1) | (pr & (stride - 1)), b = a + stride;
                    const bool best_first = (a & size) == 0;
                    const double va = bv[tp * P + a], vb = bv[tp * P + b];
                    const unsigned ia = bi[tp * P + a], ib = bi[tp * P + b];
                    const bool swap = best_first ? tt_before(vb, ib, va, ia) : tt_before(va, ia, vb, ib);
                    if (swap) { bv[tp * P + a] = vb; bi[tp * P + a] = ib; bv[tp * P + b] = va; bi[tp * P + b] = ia; }
                }
                __syncthreads();
            }
        }
        if (t < TT_TOPICS && count[t] > cnt) count[t] = cnt;
        __syncthreads();
        if (count[tj] >= cnt) { tv = bv[tj * P + cnt - 1]; ti = bi[tj * P + cnt - 1]; }
        __syncthreads();                                 // nobody fills a slot while a threshold is still being read
    };

    // a tile in registers, the next one in flight: every load unconditional at a clamped address, masked when it is used
    double cur[16], nxt[16];
    auto fetch = [&](i64 base, double (&v)[16]) {
#pragma unroll
        for (int q = 0; q < 16; ++q) {
            i64 r = base + 16 * q + tr;
            if (r > nrows - 1) r = nrows - 1;
            v[q] = (double)W[r * ld + jc];
        }
    };
    if (i0 < i1) fetch(i0, nxt);
    // steps since the slots were last checked, and until they are checked again: the first check comes as soon as cnt rows are
    // in and compacts whatever the fill, so that the chunk has thresholds early; from then on every qs steps
    int since = 0, limit = (cnt + 15) / 16 + 1;
    if (limit > qs) limit = qs;
    bool primed = false;
    for (i64 base = i0; base < i1; base += TT_TILE) {
#pragma unroll
        for (int q = 0; q < 16; ++q) cur[q] = nxt[q];
        if (base + TT_TILE < i1) fetch(base + TT_TILE, nxt);
#pragma unroll
        for (int q = 0; q < 16; ++q) {
            if (since == limit) {                        // (uniform) room for qs more steps of 16 rows in every topic?
                __syncthreads();
                const int full = (!primed || count[tj] + 16 * qs > P) ? 1 : 0;
                if (__syncthreads_or(full)) compact();
                primed = true;
                since = 0;
                limit = qs;
            }
            ++since;
            const i64 r = base + 16 * q + tr;
            const double v = cur[q];
            if (r < i1 && topic_in && (v > tv || v == tv)) {
                const unsigned id = idx_in ? idx_in[r * ld + jt] : (unsigned)r;
                if (tt_before(v, id, tv, ti)) {
                    const int sl = atomicAdd(&count[tj], 1);
                    if (sl < P) { bv[tj * P + sl] = v; bi[tj * P + sl] = id; }
                }
            }
        }
    }
    __syncthreads();
    compact();
    // the best cnt of every topic, in order (slots from count on hold the empty entry)
    for (int e = t; e < TT_TOPICS * cnt; e += 256) {
        const int tp = e & 15, q = e >> 4;
        if (j0 + tp >= k) continue;
        if (out) out[(i64)(j0 + tp) * maxterms + q] = (int)bi[tp * P + q];
        else {
            const i64 at = ((i64)blockIdx.x * cnt + q) * k + j0 + tp;
            cand_val[at] = bv[tp * P + q];
            cand_idx[at] = bi[tp * P + q];
        }
    }
}

// how stage one is cut: G row chunks (whole tiles), enough workgroups for four per CU, at most 1024 chunks
static void topterms_shape(i64 m, int k, int num_cus, i64* rows_per_chunk, int* G)
{
    const i64 tiles = (m + TT_TILE - 1) / TT_TILE;
    const i64 groups = (k + TT_TOPICS - 1) / TT_TOPICS;
    i64 want = ((i64)4 * num_cus + groups - 1) / groups;
    if (want < 1) want = 1;
    if (want > 1024) want = 1024;
    if (want > tiles) want = tiles;
    const i64 per = (tiles + want - 1) / want;
    *rows_per_chunk = per * TT_TILE;
    *G = (int)((tiles + per - 1) / per);
}

// bytes of the candidate workspace of launch_top_terms (0: one chunk, the selection writes the result itself)
size_t topterms_scratch_bytes(i64 m, int k, int maxterms, int num_cus)
{
    i64 per; int G;
    topterms_shape(m, k, num_cus, &per, &G);
    if (G <= 1) return 0;
    const i64 cnt = maxterms < m ? maxterms : m;
    return 2 * (size_t)G * cnt * k * (sizeof(double) + sizeof(unsigned));      // two sets: the merge levels go from one to the other
}

template <typename T>
static int topterms_launch(dim3 grid, int P, const T* W, i64 ld, const unsigned* idx_in, i64 nrows, int k, int cnt, i64 per, double* cv,
                           unsigned* ci, int* out, int maxterms, hipStream_t st)
{
    const size_t lds = tt_lds_bytes(P);
    if (lds > 64 * 1024) {
        static std::atomic<unsigned long long> attr_set{0};       // per device (DeviceOnce)
        if (DeviceOnce once{attr_set}) {
            SMK_HIP(hipFuncSetAttribute((const void*)topterms_select_kernel<T>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)tt_lds_bytes(tt_slots(TOPTERMS_CAP))));
            once.done();
        }
    }
    // steps of 16 rows between two looks at the fill of the slots: short runs, so that a compaction comes when the slots are nearly
    // full (P - 16 qs entries) and not whenever a worst-case run of all-entering rows would overflow them; cnt + 16 qs <= P
    const int qs = cnt <= 16 ? 7 : 4;
    topterms_select_kernel<T><<<grid, 256, lds, st>>>(W, ld, idx_in, nrows, k, cnt, P, qs, per, cv, ci, out, maxterms);
    SMK_HIP(hipGetLastError());
    return 0;
}

// W: fp64 / fp32, row i at W + i * ld (elements); out: topic j at out + j * maxterms, min(maxterms, m) slots written.
// maxterms <= TOPTERMS_CAP.  scratch: topterms_scratch_bytes, 16-byte aligned.
int launch_top_terms(const void* W, int dtype, i64 ld, i64 m, int k, int maxterms, void* scratch, int* out, int num_cus, hipStream_t st)
{
    if (m > 0x7FFFFFFFll) { set_error("top terms: more than 2^31 - 1 rows"); return -101; }
    if (maxterms > TOPTERMS_CAP) { set_error("top terms: the in-LDS selection holds at most 256 terms per topic"); return -101; }
    if (dtype != DT_F64 && dtype != DT_F32) { set_error("top terms: factors are fp64 or fp32"); return -3; }
    const int cnt = (int)(maxterms < m ? maxterms : m);
    const int P = tt_slots(cnt);
    i64 per; int G;
    topterms_shape(m, k, num_cus, &per, &G);
    const unsigned groups = (unsigned)((k + TT_TOPICS - 1) / TT_TOPICS);
    const size_t set = (size_t)G * cnt * k;                          // candidates of a set; the values of both sets, then the indices of both
    double* cv[2] = {(double*)scratch, (double*)scratch + set};
    unsigned* ci[2] = {(unsigned*)(cv[1] + set), (unsigned*)(cv[1] + set) + set};
    int* first_out = G <= 1 ? out : nullptr;
    int rc;
    if (dtype == DT_F64) rc = topterms_launch<double>(dim3((unsigned)G, groups), P, (const double*)W, ld, nullptr, m, k, cnt, per, cv[0], ci[0], first_out, maxterms, st);
    else rc = topterms_launch<float>(dim3((unsigned)G, groups), P, (const float*)W, ld, nullptr, m, k, cnt, per, cv[0], ci[0], first_out, maxterms, st);
    if (rc || G <= 1) return rc;
    // merge levels: the G * cnt candidates of a topic are rows of a [row][k] matrix again, cut into chunks of at least 16 candidate
    // lists; the level that is left with one chunk writes the result
    i64 rows = (i64)G * cnt;
    i64 rpc = (i64)16 * cnt > 2048 ? (i64)16 * cnt : 2048;
    rpc = (rpc + TT_TILE - 1) / TT_TILE * TT_TILE;
    for (int src = 0;; src ^= 1) {
        const i64 G2 = (rows + rpc - 1) / rpc;
        rc = topterms_launch<double>(dim3((unsigned)G2, groups), P, cv[src], k, ci[src], rows, k, cnt, rpc, cv[src ^ 1], ci[src ^ 1],
                                     G2 == 1 ? out : nullptr, maxterms, st);
        if (rc || G2 == 1) return rc;
        rows = G2 * cnt;
    }
}

// ---- more terms than the selection holds: a stable radix sort per topic (as sort.hip) ----------------------------------------
template <typename T>
__global__ __launch_bounds__(256) void topterms_keys_kernel(const T* __restrict__ W, i64 ld, int j, i64 m, double* __restrict__ keys,
                                                            int* __restrict__ idx)
{
    for (i64 i = (i64)blockIdx.x * 256 + threadIdx.x; i < m; i += (i64)gridDim.x * 256) {
        keys[i] = (double)W[i * ld + j] + 0.0;           // -0.0 -> +0.0: the radix order separates them and `>` does not
        idx[i] = (int)i;
    }
}

// descending keys, equal keys in index order = the host's order; the first min(maxterms, m) indices of every topic
int launch_top_terms_sorted(const void* W, int dtype, i64 ld, i64 m, int k, int maxterms, int* out, hipStream_t st)
{
    if (m > 0x7FFFFFFFll) { set_error("top terms: more than 2^31 - 1 rows"); return -101; }
    if (dtype != DT_F64 && dtype != DT_F32) { set_error("top terms: factors are fp64 or fp32"); return -3; }
    const size_t cnt = (size_t)(maxterms < m ? maxterms : m);
    double *keys = nullptr, *keys_out = nullptr;
    int *idx = nullptr, *idx_out = nullptr;
    void* temp = nullptr;
    size_t tb = 0;
    int rc = 0;
    auto fail = [&](const char* what) { set_error(std::string("top terms: ") + what); rc = -100; };
    if (hipcub::DeviceRadixSort::SortPairsDescending(nullptr, tb, keys, keys_out, idx, idx_out, (int)m, 0, 64, st) != hipSuccess) fail("hipcub size query");
    if (!rc && smk::dev_malloc(&keys, (size_t)m * 8) != hipSuccess) fail("hipMalloc");
    if (!rc && smk::dev_malloc(&keys_out, (size_t)m * 8) != hipSuccess) fail("hipMalloc");
    if (!rc && smk::dev_malloc(&idx, (size_t)m * 4) != hipSuccess) fail("hipMalloc");
    if (!rc && smk::dev_malloc(&idx_out, (size_t)m * 4) != hipSuccess) fail("hipMalloc");
    if (!rc && smk::dev_malloc(&temp, tb + 16) != hipSuccess) fail("hipMalloc");
    const unsigned grid = (unsigned)((m + 255) / 256 < 2048 ? (m + 255) / 256 : 2048);
    for (int j = 0; j < k && !rc; ++j) {
        if (dtype == DT_F64) topterms_keys_kernel<double><<<grid, 256, 0, st>>>((const double*)W, ld, j, m, keys, idx);
        else topterms_keys_kernel<float><<<grid, 256, 0, st>>>((const float*)W, ld, j, m, keys, idx);
        size_t t2 = tb;
        if (hipcub::DeviceRadixSort::SortPairsDescending(temp, t2, keys, keys_out, idx, idx_out, (int)m, 0, 64, st) != hipSuccess) { fail("hipcub radix sort"); break; }
        if (hipMemcpyAsync(out + (size_t)j * maxterms, idx_out, cnt * sizeof(int), hipMemcpyDeviceToDevice, st) != hipSuccess) { fail("copy"); break; }
    }
    if (hipStreamSynchronize(st) != hipSuccess && !rc) fail("sync");      // the buffers are freed below
    void* ptrs[] = {keys, keys_out, idx, idx_out, temp};
    for (void* p : ptrs) if (p) (void)smk::dev_free(p);
    return rc;
}

}  // namespace smk
