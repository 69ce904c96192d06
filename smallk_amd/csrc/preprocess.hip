// smallk_amd/csrc/preprocess.hip -- the passes of preprocess_tf (preprocessor/src/preprocess.cpp) on the device.
//
// The working matrix is CSC with one (row, count) pair per stored entry (uint2: x = row, y = count) and 32-bit column
// offsets, as in the reference's TermFrequencyMatrix.  Every pass that changes the matrix writes a new copy into the
// other half of a ping-pong pair; the driver (preprocess.cpp) swaps the halves.  Entry order inside a column never
// changes after the initial row sort, so the result is the reference's entry for entry.
//
// Row statistics (tot[r] = sum of counts, df[r] = number of entries) live in ONE 64-bit word per row, stat[r] =
// tot << 32 | df, so that an entry costs one integer atomic, not two: adding (count << 32 | 1) leaves df exact in the low
// word (df <= nnz < 2^31 never carries) and tot as the wrapping 32-bit sum of the reference in the high word.  They are
// computed ONCE, by a pass over every entry, and afterwards only corrected: pruning a row removes all of its entries (its
// word simply leaves with it), and pruning a column subtracts that column's entries from their rows.  Integer sums are exact
// in any order, so the words are the same bits as a recount.  (Measured: the full count costs the same with two u32
// atomics per entry; recounting every iteration costs it every iteration: DESIGN.md section 11.)
//
// Scores take one wave per column: the lanes compute the entries' terms, and every lane adds the squares in entry order
// (read lane by lane), so the sum is the reference's sequential sum and the same bits from run to run.
#include "common.h"
#include "preprocess.h"

#include <hipcub/hipcub.hpp>

namespace smk {
namespace {

constexpr int PP_BLOCK = 256;
constexpr int PP_WAVES = PP_BLOCK / 64;

inline unsigned grid_for(i64 work, i64 per_block, i64 cap)
{
    i64 g = (work + per_block - 1) / per_block;
    if (g < 1) g = 1;
    return (unsigned)(g < cap ? g : cap);
}
inline unsigned wave_grid(i64 cols) { return grid_for(cols, PP_WAVES, 65536); }
inline unsigned thread_grid(i64 n) { return grid_for(n, PP_BLOCK, 16384); }

// TermFrequencyMatrix::Init (common/src/term_frequency_matrix.cpp:53-95): boolean mode 1; negative 0; otherwise the value
// truncated toward zero.  The x86 conversion goes through a 64-bit integer; values it cannot hold (>= 2^63, inf, NaN) give
// the "integer indefinite", whose low 32 bits are 0.
__device__ inline unsigned to_count(double v, int boolean_mode)
{
    if (boolean_mode) return 1u;
    if (v < 0.0) return 0u;
    if (!(v < 9223372036854775808.0)) return 0u;
    return (unsigned)(unsigned long long)(long long)v;
}

// one wave per column: entries -> (row, count); a column whose rows decrease somewhere raises *unsorted
__global__ __launch_bounds__(PP_BLOCK) void pp_convert_kernel(const unsigned* __restrict__ cp, const unsigned* __restrict__ rows,
                                                              const double* __restrict__ data, unsigned width, int boolean_mode,
                                                              uint2* __restrict__ ent, unsigned* __restrict__ unsorted)
{
    const int lane = threadIdx.x & 63;
    for (i64 c = (i64)blockIdx.x * PP_WAVES + (threadIdx.x >> 6); c < width; c += (i64)gridDim.x * PP_WAVES) {
        const unsigned s = cp[c], e = cp[c + 1];
        bool bad = false;
        for (unsigned p = s + lane; p < e; p += 64) {
            const unsigned r = rows[p];
            ent[p] = make_uint2(r, to_count(data[p], boolean_mode));
            if (p > s && rows[p - 1] > r) bad = true;
        }
        if (__ballot(bad) && lane == 0) atomicOr(unsorted, 1u);
    }
}

__global__ __launch_bounds__(PP_BLOCK) void pp_split_kernel(const uint2* __restrict__ ent, i64 nnz, unsigned* __restrict__ k,
                                                            unsigned* __restrict__ v)
{
    for (i64 p = (i64)blockIdx.x * PP_BLOCK + threadIdx.x; p < nnz; p += (i64)gridDim.x * PP_BLOCK) {
        const uint2 x = ent[p];
        k[p] = x.x;
        v[p] = x.y;
    }
}

__global__ __launch_bounds__(PP_BLOCK) void pp_join_kernel(const unsigned* __restrict__ k, const unsigned* __restrict__ v, i64 nnz,
                                                           uint2* __restrict__ ent)
{
    for (i64 p = (i64)blockIdx.x * PP_BLOCK + threadIdx.x; p < nnz; p += (i64)gridDim.x * PP_BLOCK) ent[p] = make_uint2(k[p], v[p]);
}

__device__ inline unsigned long long stat_word(unsigned count) { return ((unsigned long long)count << 32) | 1ull; }

// the full count: one 64-bit integer atomic per entry (done once per call)
__global__ __launch_bounds__(PP_BLOCK) void pp_row_stats_kernel(const uint2* __restrict__ ent, i64 nnz, unsigned long long* __restrict__ stat)
{
    for (i64 p = (i64)blockIdx.x * PP_BLOCK + threadIdx.x; p < nnz; p += (i64)gridDim.x * PP_BLOCK) {
        const uint2 x = ent[p];
        atomicAdd(&stat[x.x], stat_word(x.y));
    }
}

// PruneRows' mask (preprocess.cpp:279-367): keep r iff tot[r] >= docs_per_term and df[r] < width; flag[height] = 0 closes the scan
__global__ __launch_bounds__(PP_BLOCK) void pp_row_keep_kernel(const unsigned long long* __restrict__ stat, unsigned height,
                                                               unsigned docs_per_term, unsigned width, unsigned* __restrict__ flag)
{
    for (i64 r = (i64)blockIdx.x * PP_BLOCK + threadIdx.x; r <= height; r += (i64)gridDim.x * PP_BLOCK) {
        bool keep = false;
        if (r < height) {
            const unsigned long long w = stat[r];
            keep = (unsigned)(w >> 32) >= docs_per_term && (unsigned)w < width;
        }
        flag[r] = keep ? 1u : 0u;
    }
}

// kept rows move to their new index with their statistics and term index
__global__ __launch_bounds__(PP_BLOCK) void pp_row_gather_kernel(const unsigned* __restrict__ flag, const unsigned* __restrict__ pos,
                                                                 unsigned height, const unsigned long long* __restrict__ stat,
                                                                 const unsigned* __restrict__ term, unsigned long long* __restrict__ stat2,
                                                                 unsigned* __restrict__ term2)
{
    for (i64 r = (i64)blockIdx.x * PP_BLOCK + threadIdx.x; r < height; r += (i64)gridDim.x * PP_BLOCK)
        if (flag[r]) {
            const unsigned j = pos[r];
            stat2[j] = stat[r];
            term2[j] = term[r];
        }
}

// one wave per column: number of entries whose row is kept; len[width] = 0 closes the scan
__global__ __launch_bounds__(PP_BLOCK) void pp_col_count_rows_kernel(const unsigned* __restrict__ cp, const uint2* __restrict__ ent,
                                                                     unsigned width, const unsigned* __restrict__ rflag,
                                                                     unsigned* __restrict__ len)
{
    const int lane = threadIdx.x & 63;
    for (i64 c = (i64)blockIdx.x * PP_WAVES + (threadIdx.x >> 6); c <= width; c += (i64)gridDim.x * PP_WAVES) {
        if (c == width) {
            if (lane == 0) len[c] = 0;
            continue;
        }
        const unsigned s = cp[c], e = cp[c + 1];
        unsigned n = 0;
        for (unsigned p = s + lane; p < e; p += 64) n += rflag[ent[p].x];
        for (int off = 32; off > 0; off >>= 1) n += __shfl_down(n, off, 64);
        if (lane == 0) len[c] = n;
    }
}

// one wave per column: the kept entries, in order, with renumbered rows
__global__ __launch_bounds__(PP_BLOCK) void pp_col_fill_rows_kernel(const unsigned* __restrict__ cp, const uint2* __restrict__ ent,
                                                                    unsigned width, const unsigned* __restrict__ rflag,
                                                                    const unsigned* __restrict__ rpos, const unsigned* __restrict__ cp2,
                                                                    uint2* __restrict__ ent2)
{
    const int lane = threadIdx.x & 63;
    const unsigned long long below = (1ull << lane) - 1ull;
    for (i64 c = (i64)blockIdx.x * PP_WAVES + (threadIdx.x >> 6); c < width; c += (i64)gridDim.x * PP_WAVES) {
        const unsigned s = cp[c], e = cp[c + 1];
        unsigned d = cp2[c];
        for (unsigned base = s; base < e; base += 64) {
            const unsigned p = base + lane;
            uint2 x = make_uint2(0u, 0u);
            bool keep = false;
            if (p < e) {
                x = ent[p];
                keep = rflag[x.x] != 0;
            }
            const unsigned long long m = __ballot(keep);
            if (keep) ent2[d + __popcll(m & below)] = make_uint2(rpos[x.x], x.y);
            d += (unsigned)__popcll(m);
        }
    }
}

// PrunableCols (preprocess.cpp:370-404): keep c iff it has at least terms_per_doc entries
__global__ __launch_bounds__(PP_BLOCK) void pp_col_keep_len_kernel(const unsigned* __restrict__ cp, unsigned width, unsigned terms_per_doc,
                                                                   unsigned* __restrict__ flag)
{
    for (i64 c = (i64)blockIdx.x * PP_BLOCK + threadIdx.x; c <= width; c += (i64)gridDim.x * PP_BLOCK)
        flag[c] = (c < width && cp[c + 1] - cp[c] >= terms_per_doc) ? 1u : 0u;
}

// the entries a column keeps: its length if kept, else 0 (len[width] = 0)
__global__ __launch_bounds__(PP_BLOCK) void pp_col_kept_len_kernel(const unsigned* __restrict__ cp, unsigned width,
                                                                   const unsigned* __restrict__ flag, unsigned* __restrict__ len)
{
    for (i64 c = (i64)blockIdx.x * PP_BLOCK + threadIdx.x; c <= width; c += (i64)gridDim.x * PP_BLOCK)
        len[c] = (c < width && flag[c]) ? cp[c + 1] - cp[c] : 0u;
}

// one wave per dropped column: its entries leave their rows' statistics
__global__ __launch_bounds__(PP_BLOCK) void pp_col_drop_stats_kernel(const unsigned* __restrict__ cp, const uint2* __restrict__ ent,
                                                                     unsigned width, const unsigned* __restrict__ flag,
                                                                     unsigned long long* __restrict__ stat)
{
    const int lane = threadIdx.x & 63;
    for (i64 c = (i64)blockIdx.x * PP_WAVES + (threadIdx.x >> 6); c < width; c += (i64)gridDim.x * PP_WAVES) {
        if (flag[c]) continue;
        const unsigned s = cp[c], e = cp[c + 1];
        for (unsigned p = s + lane; p < e; p += 64) {
            const uint2 x = ent[p];
            atomicAdd(&stat[x.x], 0ull - stat_word(x.y));          // exact: df >= 1 here, so the low word never borrows
        }
    }
}

// PruneCols (preprocess.cpp:406-443): one wave per kept column copies it to its new place; cp2[new_width] closes the offsets
__global__ __launch_bounds__(PP_BLOCK) void pp_col_copy_kernel(const unsigned* __restrict__ cp, const uint2* __restrict__ ent,
                                                               unsigned width, const unsigned* __restrict__ flag,
                                                               const unsigned* __restrict__ cpos, const unsigned* __restrict__ dst,
                                                               const unsigned* __restrict__ doc, unsigned* __restrict__ cp2,
                                                               uint2* __restrict__ ent2, unsigned* __restrict__ doc2)
{
    const int lane = threadIdx.x & 63;
    for (i64 c = (i64)blockIdx.x * PP_WAVES + (threadIdx.x >> 6); c <= width; c += (i64)gridDim.x * PP_WAVES) {
        if (c == width) {
            if (lane == 0) cp2[cpos[c]] = dst[c];
            continue;
        }
        if (!flag[c]) continue;
        const unsigned s = cp[c], e = cp[c + 1], d = dst[c];
        if (lane == 0) {
            cp2[cpos[c]] = d;
            doc2[cpos[c]] = doc[c];
        }
        for (unsigned p = s + lane; p < e; p += 64) ent2[d + (p - s)] = ent[p];
    }
}

__device__ inline unsigned long long mix64(unsigned long long z)
{
    z = (z ^ (z >> 30)) * 0xbf58476d1ce4e5b9ull;
    z = (z ^ (z >> 27)) * 0x94d049bb133111ebull;
    return z ^ (z >> 31);
}

// one wave per column: a 64-bit hash of its (position, row, count) sequence and its length.  The per-entry terms are
// added mod 2^64, so the lanes need no order; equal hashes are resolved by exact comparison afterwards.
__global__ __launch_bounds__(PP_BLOCK) void pp_hash_kernel(const unsigned* __restrict__ cp, const uint2* __restrict__ ent, unsigned width,
                                                           unsigned long long* __restrict__ hash, unsigned* __restrict__ idx)
{
    const int lane = threadIdx.x & 63;
    for (i64 c = (i64)blockIdx.x * PP_WAVES + (threadIdx.x >> 6); c < width; c += (i64)gridDim.x * PP_WAVES) {
        const unsigned s = cp[c], e = cp[c + 1];
        unsigned long long h = 0;
        for (unsigned p = s + lane; p < e; p += 64) {
            const uint2 x = ent[p];
            h += mix64(mix64(((unsigned long long)(p - s) << 32) ^ x.x) ^ ((unsigned long long)x.y * 0x9e3779b97f4a7c15ull));
        }
        for (int off = 32; off > 0; off >>= 1) h += __shfl_down(h, off, 64);
        if (lane == 0) {
            hash[c] = mix64(h ^ mix64((unsigned long long)(e - s) + 0x632be59bd9b4e019ull));
            idx[c] = (unsigned)c;
        }
    }
}

__device__ inline bool same_column(const unsigned* __restrict__ cp, const uint2* __restrict__ ent, unsigned a, unsigned b)
{
    const unsigned sa = cp[a], la = cp[a + 1] - sa, sb = cp[b], lb = cp[b + 1] - sb;
    if (la != lb) return false;
    for (unsigned t = 0; t < la; ++t) {
        const uint2 x = ent[sa + t], y = ent[sb + t];
        if (x.x != y.x || x.y != y.y) return false;
    }
    return true;
}

// last position of the run of equal hashes that holds position i (the hashes are sorted)
__device__ inline unsigned run_last(const unsigned long long* __restrict__ hs, unsigned i, unsigned n)
{
    const unsigned long long h = hs[i];
    unsigned lo = i + 1, hi = n;
    while (lo < hi) {
        const unsigned mid = lo + ((hi - lo) >> 1);
        if (hs[mid] == h) lo = mid + 1; else hi = mid;
    }
    return lo - 1;
}

// Duplicate check, step 1.  Within a run of equal hashes the stable sort keeps increasing column order, so the run's last
// member has the largest column index: every other member is compared with it once.  Equal: dropped.  Different (a hash
// collision): marked for step 2.
__global__ __launch_bounds__(PP_BLOCK) void pp_dup_rep_kernel(const unsigned* __restrict__ cp, const uint2* __restrict__ ent,
                                                              const unsigned long long* __restrict__ hs, const unsigned* __restrict__ idx,
                                                              unsigned n, unsigned* __restrict__ keep, unsigned* __restrict__ differ)
{
    for (i64 i = (i64)blockIdx.x * PP_BLOCK + threadIdx.x; i + 1 < n; i += (i64)gridDim.x * PP_BLOCK) {
        if (hs[i] != hs[i + 1]) continue;
        const unsigned rep = run_last(hs, (unsigned)i, n);
        if (same_column(cp, ent, idx[i], idx[rep])) keep[idx[i]] = 0u;
        else differ[i] = 1u;
    }
}

// Duplicate check, step 2: a member that differs from its run's last member is dropped iff a later member that differs too
// (a larger column index) holds the same entries.  Nothing to do unless 64-bit hashes of different columns collided.
__global__ __launch_bounds__(PP_BLOCK) void pp_dup_pairs_kernel(const unsigned* __restrict__ cp, const uint2* __restrict__ ent,
                                                                const unsigned long long* __restrict__ hs, const unsigned* __restrict__ idx,
                                                                unsigned n, const unsigned* __restrict__ differ, unsigned* __restrict__ keep)
{
    for (i64 i = (i64)blockIdx.x * PP_BLOCK + threadIdx.x; i + 1 < n; i += (i64)gridDim.x * PP_BLOCK) {
        if (!differ[i]) continue;
        const unsigned rep = run_last(hs, (unsigned)i, n);
        for (unsigned k = (unsigned)i + 1; k < rep; ++k)
            if (differ[k] && same_column(cp, ent, idx[i], idx[k])) {
                keep[idx[i]] = 0u;
                break;
            }
    }
}

// scores (preprocess.cpp:186-232): idf[r] = log(width / df[r])
__global__ __launch_bounds__(PP_BLOCK) void pp_idf_kernel(const unsigned long long* __restrict__ stat, unsigned height, unsigned width,
                                                          double* __restrict__ idf)
{
    for (i64 r = (i64)blockIdx.x * PP_BLOCK + threadIdx.x; r < height; r += (i64)gridDim.x * PP_BLOCK)
        idf[r] = log((double)width / (double)(unsigned)stat[r]);
}

__device__ inline double read_lane(double v, int k)
{
    const long long b = __double_as_longlong(v);
    const unsigned lo = (unsigned)__builtin_amdgcn_readlane((int)(unsigned)b, k);
    const unsigned hi = (unsigned)__builtin_amdgcn_readlane((int)(unsigned)(b >> 32), k);
    return __longlong_as_double((long long)(((unsigned long long)hi << 32) | lo));
}

// one wave per column: s = (1 + log(count)) * idf[row] by the lanes; the sum of s^2 in entry order (every lane adds the 64
// squares of a chunk lane by lane, so all lanes hold the same sequential sum); D = 1 / sqrt(sum); s *= D.  No contraction
// into fma (the reference's x86 build has none), and NaN written as the x86 default NaN (sign bit set), the value the
// reference computes wherever a NaN arises here (-inf * 0, 0 * inf, and everything a NaN propagates into).
__global__ __launch_bounds__(PP_BLOCK) void pp_score_kernel(const unsigned* __restrict__ cp, const uint2* __restrict__ ent, unsigned width,
                                                            const double* __restrict__ idf, double* __restrict__ score)
{
#pragma clang fp contract(off)
    const int lane = threadIdx.x & 63;
    for (i64 c = (i64)blockIdx.x * PP_WAVES + (threadIdx.x >> 6); c < width; c += (i64)gridDim.x * PP_WAVES) {
        const unsigned s = cp[c], e = cp[c + 1];
        double sum_sq = 0.0;
        for (unsigned base = s; base < e; base += 64) {
            const unsigned p = base + lane;
            double v = 0.0;
            if (p < e) {
                const uint2 x = ent[p];
                v = 1.0 + log((double)x.y);
                v *= idf[x.x];
                score[p] = v;
            }
            const double sq = v * v;
            const int cnt = (int)(e - base < 64 ? e - base : 64);
            for (int k = 0; k < cnt; ++k) sum_sq += read_lane(sq, k);
        }
        const double D = 1.0 / sqrt(sum_sq);
        for (unsigned p = s + lane; p < e; p += 64) {
            double v = score[p] * D;
            if (v != v) v = __longlong_as_double((long long)0xFFF8000000000000ull);
            score[p] = v;
        }
    }
}

__global__ __launch_bounds__(PP_BLOCK) void pp_iota_kernel(unsigned* __restrict__ out, unsigned n)
{
    for (i64 i = (i64)blockIdx.x * PP_BLOCK + threadIdx.x; i < n; i += (i64)gridDim.x * PP_BLOCK) out[i] = (unsigned)i;
}

__global__ __launch_bounds__(PP_BLOCK) void pp_export_kernel(const unsigned* __restrict__ cp, unsigned width, const uint2* __restrict__ ent,
                                                             i64 nnz, i64* __restrict__ colptr, unsigned* __restrict__ rows)
{
    const i64 n = nnz > (i64)width + 1 ? nnz : (i64)width + 1;
    for (i64 i = (i64)blockIdx.x * PP_BLOCK + threadIdx.x; i < n; i += (i64)gridDim.x * PP_BLOCK) {
        if (i <= width && colptr) colptr[i] = (i64)cp[i];
        if (i < nnz) rows[i] = ent[i].x;
    }
}

}  // namespace

#define PP_LAUNCH_CHECK()                                                                     \
    do {                                                                                      \
        hipError_t _e = hipGetLastError();                                                    \
        if (_e != hipSuccess) {                                                               \
            set_error(std::string("preprocess kernel launch: ") + hipGetErrorString(_e));     \
            return -100;                                                                      \
        }                                                                                     \
    } while (0)

int PpScan::exclusive(const unsigned* in, unsigned* out, i64 count, hipStream_t st)
{
    size_t need = 0;
    SMK_HIP(hipcub::DeviceScan::ExclusiveSum(nullptr, need, in, out, (int)count, st));
    if (need > cap) {
        if (temp) (void)dev_free(temp);
        temp = nullptr;
        cap = 0;
        SMK_HIP(dev_malloc(&temp, need));
        cap = need;
    }
    SMK_HIP(hipcub::DeviceScan::ExclusiveSum(temp, need, in, out, (int)count, st));
    return 0;
}

int PpScan::sort_pairs(const unsigned long long* kin, unsigned long long* kout, const unsigned* vin, unsigned* vout, i64 n,
                       hipStream_t st)
{
    size_t need = 0;
    SMK_HIP(hipcub::DeviceRadixSort::SortPairs(nullptr, need, kin, kout, vin, vout, (int)n, 0, 64, st));
    if (need > cap) {
        if (temp) (void)dev_free(temp);
        temp = nullptr;
        cap = 0;
        SMK_HIP(dev_malloc(&temp, need));
        cap = need;
    }
    SMK_HIP(hipcub::DeviceRadixSort::SortPairs(temp, need, kin, kout, vin, vout, (int)n, 0, 64, st));
    return 0;
}

void PpScan::release()
{
    if (temp) (void)dev_free(temp);
    temp = nullptr;
    cap = 0;
}

int pp_convert(const unsigned* cp, const unsigned* rows, const double* data, unsigned width, int boolean_mode, uint2* ent,
               unsigned* unsorted, hipStream_t st)
{
    pp_convert_kernel<<<wave_grid(width), PP_BLOCK, 0, st>>>(cp, rows, data, width, boolean_mode, ent, unsorted);
    PP_LAUNCH_CHECK();
    return 0;
}

// SortRows (term_frequency_matrix.cpp:143): a stable segmented radix sort by row, one segment per column
int pp_sort_columns(const unsigned* cp, unsigned width, i64 nnz, unsigned height, uint2* ent, hipStream_t st)
{
    if (nnz <= 0) return 0;
    unsigned *k = nullptr, *v = nullptr, *k2 = nullptr, *v2 = nullptr;
    void* temp = nullptr;
    size_t need = 0;
    int bits = 1;
    while (((i64)1 << bits) < (i64)height && bits < 32) ++bits;
    int rc = 0;
    auto fail = [&](const char* what, hipError_t e) {
        if (!rc) set_error(std::string("preprocess row sort: ") + what + ": " + hipGetErrorString(e));
        rc = -100;
    };
    hipError_t e = hipcub::DeviceSegmentedRadixSort::SortPairs(nullptr, need, k, k2, v, v2, (int)nnz, (int)width, cp, cp + 1, 0,
                                                               bits, st);
    if (e != hipSuccess) fail("size query", e);
    if (!rc && (e = dev_malloc(&k, (size_t)nnz * 4)) != hipSuccess) fail("hipMalloc", e);
    if (!rc && (e = dev_malloc(&v, (size_t)nnz * 4)) != hipSuccess) fail("hipMalloc", e);
    if (!rc && (e = dev_malloc(&k2, (size_t)nnz * 4)) != hipSuccess) fail("hipMalloc", e);
    if (!rc && (e = dev_malloc(&v2, (size_t)nnz * 4)) != hipSuccess) fail("hipMalloc", e);
    if (!rc && (e = dev_malloc(&temp, need + 16)) != hipSuccess) fail("hipMalloc", e);
    if (!rc) {
        pp_split_kernel<<<thread_grid(nnz), PP_BLOCK, 0, st>>>(ent, nnz, k, v);
        e = hipcub::DeviceSegmentedRadixSort::SortPairs(temp, need, k, k2, v, v2, (int)nnz, (int)width, cp, cp + 1, 0, bits, st);
        if (e != hipSuccess) fail("sort", e);
    }
    if (!rc) {
        pp_join_kernel<<<thread_grid(nnz), PP_BLOCK, 0, st>>>(k2, v2, nnz, ent);
        if ((e = hipStreamSynchronize(st)) != hipSuccess) fail("sync", e);
    }
    void* ptrs[] = {k, v, k2, v2, temp};
    for (void* p : ptrs)
        if (p) (void)dev_free(p);
    return rc;
}

int pp_row_stats(const uint2* ent, i64 nnz, unsigned long long* stat, hipStream_t st)
{
    if (nnz <= 0) return 0;
    pp_row_stats_kernel<<<thread_grid(nnz), PP_BLOCK, 0, st>>>(ent, nnz, stat);
    PP_LAUNCH_CHECK();
    return 0;
}

int pp_row_keep(const unsigned long long* stat, unsigned height, unsigned docs_per_term, unsigned width, unsigned* flag, hipStream_t st)
{
    pp_row_keep_kernel<<<thread_grid((i64)height + 1), PP_BLOCK, 0, st>>>(stat, height, docs_per_term, width, flag);
    PP_LAUNCH_CHECK();
    return 0;
}

int pp_row_gather(const unsigned* flag, const unsigned* pos, unsigned height, const unsigned long long* stat, const unsigned* term,
                  unsigned long long* stat2, unsigned* term2, hipStream_t st)
{
    pp_row_gather_kernel<<<thread_grid(height), PP_BLOCK, 0, st>>>(flag, pos, height, stat, term, stat2, term2);
    PP_LAUNCH_CHECK();
    return 0;
}

int pp_col_count_rows(const unsigned* cp, const uint2* ent, unsigned width, const unsigned* rflag, unsigned* len, hipStream_t st)
{
    pp_col_count_rows_kernel<<<wave_grid((i64)width + 1), PP_BLOCK, 0, st>>>(cp, ent, width, rflag, len);
    PP_LAUNCH_CHECK();
    return 0;
}

int pp_col_fill_rows(const unsigned* cp, const uint2* ent, unsigned width, const unsigned* rflag, const unsigned* rpos,
                     const unsigned* cp2, uint2* ent2, hipStream_t st)
{
    pp_col_fill_rows_kernel<<<wave_grid(width), PP_BLOCK, 0, st>>>(cp, ent, width, rflag, rpos, cp2, ent2);
    PP_LAUNCH_CHECK();
    return 0;
}

int pp_col_keep_len(const unsigned* cp, unsigned width, unsigned terms_per_doc, unsigned* flag, hipStream_t st)
{
    pp_col_keep_len_kernel<<<thread_grid((i64)width + 1), PP_BLOCK, 0, st>>>(cp, width, terms_per_doc, flag);
    PP_LAUNCH_CHECK();
    return 0;
}

int pp_col_kept_len(const unsigned* cp, unsigned width, const unsigned* flag, unsigned* len, hipStream_t st)
{
    pp_col_kept_len_kernel<<<thread_grid((i64)width + 1), PP_BLOCK, 0, st>>>(cp, width, flag, len);
    PP_LAUNCH_CHECK();
    return 0;
}

int pp_col_drop_stats(const unsigned* cp, const uint2* ent, unsigned width, const unsigned* flag, unsigned long long* stat, hipStream_t st)
{
    pp_col_drop_stats_kernel<<<wave_grid(width), PP_BLOCK, 0, st>>>(cp, ent, width, flag, stat);
    PP_LAUNCH_CHECK();
    return 0;
}

int pp_col_copy(const unsigned* cp, const uint2* ent, unsigned width, const unsigned* flag, const unsigned* cpos, const unsigned* dst,
                const unsigned* doc, unsigned* cp2, uint2* ent2, unsigned* doc2, hipStream_t st)
{
    pp_col_copy_kernel<<<wave_grid((i64)width + 1), PP_BLOCK, 0, st>>>(cp, ent, width, flag, cpos, dst, doc, cp2, ent2, doc2);
    PP_LAUNCH_CHECK();
    return 0;
}

int pp_hash(const unsigned* cp, const uint2* ent, unsigned width, unsigned long long* hash, unsigned* idx, hipStream_t st)
{
    pp_hash_kernel<<<wave_grid(width), PP_BLOCK, 0, st>>>(cp, ent, width, hash, idx);
    PP_LAUNCH_CHECK();
    return 0;
}

int pp_dup_resolve(const unsigned* cp, const uint2* ent, const unsigned long long* hs, const unsigned* idx, unsigned n,
                   unsigned* keep, unsigned* differ, hipStream_t st)
{
    SMK_HIP(hipMemsetD32Async((hipDeviceptr_t)keep, 1u, (size_t)n, st));
    SMK_HIP(hipMemsetAsync(keep + n, 0, 4, st));                       // keep[n] = 0 closes the scan
    SMK_HIP(hipMemsetAsync(differ, 0, (size_t)n * 4 + 4, st));
    pp_dup_rep_kernel<<<thread_grid(n), PP_BLOCK, 0, st>>>(cp, ent, hs, idx, n, keep, differ);
    pp_dup_pairs_kernel<<<thread_grid(n), PP_BLOCK, 0, st>>>(cp, ent, hs, idx, n, differ, keep);
    PP_LAUNCH_CHECK();
    return 0;
}

int pp_scores(const unsigned* cp, const uint2* ent, unsigned width, const unsigned long long* stat, unsigned height, double* idf,
              double* score, hipStream_t st)
{
    if (height > 0) pp_idf_kernel<<<thread_grid(height), PP_BLOCK, 0, st>>>(stat, height, width, idf);
    pp_score_kernel<<<wave_grid(width), PP_BLOCK, 0, st>>>(cp, ent, width, idf, score);
    PP_LAUNCH_CHECK();
    return 0;
}

int pp_iota(unsigned* out, unsigned n, hipStream_t st)
{
    pp_iota_kernel<<<thread_grid(n), PP_BLOCK, 0, st>>>(out, n);
    PP_LAUNCH_CHECK();
    return 0;
}

int pp_export(const unsigned* cp, unsigned width, const uint2* ent, i64 nnz, i64* colptr, unsigned* rows, hipStream_t st)
{
    pp_export_kernel<<<thread_grid(nnz > (i64)width + 1 ? nnz : (i64)width + 1), PP_BLOCK, 0, st>>>(cp, width, ent, nnz, colptr, rows);
    PP_LAUNCH_CHECK();
    return 0;
}

}  // namespace smk
