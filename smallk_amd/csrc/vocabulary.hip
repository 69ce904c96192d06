// smallk_amd/csrc/vocabulary.hip -- new documents against a fitted term set and idf.
//
// The input is the (row, count) CSC of preprocess.hip after its convert (and row sort, where needed), rows in the ORIGINAL
// term numbering.  Two passes over its entries:
//   count  one wave per column: gather old_to_new[row], ballot, popcount -> the column's surviving length and keep flag;
//   fill   one wave per kept column streams the column once in 64-entry chunks: the ballot prefix is the entry's compacted
//          slot, the lane writes (new row, count) and the raw score there, every lane adds the chunk's squares in entry
//          order (read lane by lane, as pp_score_kernel does), and the wave rescales the slots it has just written.
// A filtered lane, and a lane past the column's end, contributes an exact +0.0 to the sum.  The running sum is +0.0 or larger (or NaN) at every step, and
// x + 0.0 == x bit for bit for such x, so the sum is the one pp_score_kernel forms over the surviving entries alone: a fit's
// own documents come out with the fit's bits.  No atomics anywhere.
#include "common.h"
#include "vocabulary.h"

namespace smk {
namespace {

constexpr int VOC_BLOCK = 256;
constexpr int VOC_WAVES = VOC_BLOCK / 64;
constexpr int VOC_U = 4;                              // chunks of 64 entries a wave has in flight per load stage

inline unsigned grid_for(i64 work, i64 per_block, i64 cap)
{
    i64 g = (work + per_block - 1) / per_block;
    if (g < 1) g = 1;
    return (unsigned)(g < cap ? g : cap);
}
inline unsigned wave_grid(i64 cols) { return grid_for(cols, VOC_WAVES, 65536); }
inline unsigned thread_grid(i64 n) { return grid_for(n, VOC_BLOCK, 16384); }

__global__ __launch_bounds__(VOC_BLOCK) void voc_clear_kernel(unsigned* __restrict__ old_to_new, unsigned height_in)
{
    for (i64 r = (i64)blockIdx.x * VOC_BLOCK + threadIdx.x; r < height_in; r += (i64)gridDim.x * VOC_BLOCK) old_to_new[r] = VOC_PRUNED;
}

// term is strictly ascending and below height_in (checked by the host before the launch): no two threads write one word
__global__ __launch_bounds__(VOC_BLOCK) void voc_scatter_kernel(const unsigned* __restrict__ term, unsigned height,
                                                                unsigned* __restrict__ old_to_new)
{
    for (i64 i = (i64)blockIdx.x * VOC_BLOCK + threadIdx.x; i < height; i += (i64)gridDim.x * VOC_BLOCK) old_to_new[term[i]] = (unsigned)i;
}

// one wave per column: the number of entries whose term survived the fit.  VOC_U chunks of 64 entries are loaded before the
// first gather is issued, so a long column pays the load and gather latencies once per VOC_U chunks.
__global__ __launch_bounds__(VOC_BLOCK) void voc_count_kernel(const unsigned* __restrict__ cp, const uint2* __restrict__ ent, unsigned width,
                                                              const unsigned* __restrict__ old_to_new, unsigned min_terms,
                                                              unsigned* __restrict__ flag, unsigned* __restrict__ len)
{
    const int lane = threadIdx.x & 63;
    for (i64 c = (i64)blockIdx.x * VOC_WAVES + (threadIdx.x >> 6); c <= width; c += (i64)gridDim.x * VOC_WAVES) {
        unsigned n = 0;
        bool keep_col = false;
        if (c < width) {
            const unsigned s = cp[c], e = cp[c + 1];
            for (unsigned base = s; base < e; base += 64 * VOC_U) {
                unsigned row[VOC_U], nr[VOC_U];
#pragma unroll
                for (int j = 0; j < VOC_U; ++j) {
                    const unsigned p = base + 64 * j + lane;
                    row[j] = p < e ? ent[p].x : VOC_PRUNED;
                }
#pragma unroll
                for (int j = 0; j < VOC_U; ++j) nr[j] = row[j] != VOC_PRUNED ? old_to_new[row[j]] : VOC_PRUNED;
#pragma unroll
                for (int j = 0; j < VOC_U; ++j) n += (unsigned)__popcll(__ballot(nr[j] != VOC_PRUNED));
            }
            keep_col = n >= min_terms;
        }
        if (lane == 0) {
            flag[c] = keep_col ? 1u : 0u;
            len[c] = keep_col ? n : 0u;
        }
    }
}

__device__ inline double read_lane(double v, int k)
{
    const long long b = __double_as_longlong(v);
    const unsigned lo = (unsigned)__builtin_amdgcn_readlane((int)(unsigned)b, k);
    const unsigned hi = (unsigned)__builtin_amdgcn_readlane((int)(unsigned)(b >> 32), k);
    return __longlong_as_double((long long)(((unsigned long long)hi << 32) | lo));
}

// the loads of one super-chunk (VOC_U chunks of 64 entries from `base`), one stage each: the pairs, the gathered new rows, the
// gathered idf.  A lane past the column's end loads nothing and holds VOC_PRUNED.
__device__ inline void voc_load_ent(const uint2* __restrict__ ent, unsigned base, unsigned e, int lane, uint2 (&x)[VOC_U])
{
#pragma unroll
    for (int j = 0; j < VOC_U; ++j) {
        const unsigned p = base + 64 * j + lane;
        x[j] = p < e ? ent[p] : make_uint2(VOC_PRUNED, 0u);
    }
}
__device__ inline void voc_load_rows(const unsigned* __restrict__ old_to_new, unsigned base, unsigned e, int lane, const uint2 (&x)[VOC_U],
                                     unsigned (&nr)[VOC_U])
{
#pragma unroll
    for (int j = 0; j < VOC_U; ++j) {
        const unsigned p = base + 64 * j + lane;
        nr[j] = p < e ? old_to_new[x[j].x] : VOC_PRUNED;
    }
}
__device__ inline void voc_load_idf(const double* __restrict__ idf, const unsigned (&nr)[VOC_U], double (&w)[VOC_U])
{
#pragma unroll
    for (int j = 0; j < VOC_U; ++j) w[j] = nr[j] != VOC_PRUNED ? idf[nr[j]] : 0.0;
}

// one wave per kept column.  s = (1 + log(count)) * idf[new row], the sum of s^2 in entry order, D = 1 / sqrt(sum), s *= D:
// the operations of pp_score_kernel in its order, without contraction into fma, NaN written as the x86 default NaN.
// The sum makes a column sequential, so a long column is a chain of chunks and its time is the chunk's latency: the three
// dependent loads of an entry (pair -> new row -> idf) are therefore issued three, two and one super-chunks ahead of the
// super-chunk being summed.
__global__ __launch_bounds__(VOC_BLOCK) void voc_fill_score_kernel(const unsigned* __restrict__ cp, const uint2* __restrict__ ent, unsigned width,
                                                                   const unsigned* __restrict__ old_to_new, const double* __restrict__ idf,
                                                                   const unsigned* __restrict__ flag, const unsigned* __restrict__ cpos,
                                                                   const unsigned* __restrict__ dst, unsigned* __restrict__ cp2,
                                                                   uint2* __restrict__ ent2, double* score, unsigned* __restrict__ doc2)
{
#pragma clang fp contract(off)
    constexpr unsigned SUPER = 64 * VOC_U;
    const int lane = threadIdx.x & 63;
    const unsigned long long below = (1ull << lane) - 1ull;
    for (i64 c = (i64)blockIdx.x * VOC_WAVES + (threadIdx.x >> 6); c <= width; c += (i64)gridDim.x * VOC_WAVES) {
        if (c == width) {
            if (lane == 0) cp2[cpos[c]] = dst[c];
            continue;
        }
        if (!flag[c]) continue;
        const unsigned s = cp[c], e = cp[c + 1], d0 = dst[c];
        if (lane == 0) {
            cp2[cpos[c]] = d0;
            doc2[cpos[c]] = (unsigned)c;
        }
        unsigned d = d0;
        double sum_sq = 0.0;
        // x0 / nr0 / w0: the super-chunk at `base`; x1 / nr1: the next one; x2: the one after (nnz < 2^31: base + 3 SUPER fits)
        uint2 x0[VOC_U], x1[VOC_U], x2[VOC_U], x3[VOC_U];
        unsigned nr0[VOC_U], nr1[VOC_U], nr2[VOC_U];
        double w0[VOC_U], w1[VOC_U];
        voc_load_ent(ent, s, e, lane, x0);
        voc_load_ent(ent, s + SUPER, e, lane, x1);
        voc_load_ent(ent, s + 2 * SUPER, e, lane, x2);
        voc_load_rows(old_to_new, s, e, lane, x0, nr0);
        voc_load_rows(old_to_new, s + SUPER, e, lane, x1, nr1);
        voc_load_idf(idf, nr0, w0);
        for (unsigned base = s; base < e; base += SUPER) {
            voc_load_ent(ent, base + 3 * SUPER, e, lane, x3);
            voc_load_rows(old_to_new, base + 2 * SUPER, e, lane, x2, nr2);
            voc_load_idf(idf, nr1, w1);
#pragma unroll
            for (int j = 0; j < VOC_U; ++j) {
                const unsigned cb = base + 64 * j;
                if (cb >= e) break;
                const bool keep = nr0[j] != VOC_PRUNED;
                const unsigned long long m = __ballot(keep);
                if (m == 0ull) continue;
                double v = 0.0;
                if (keep) {
                    const unsigned slot = d + (unsigned)__popcll(m & below);
                    v = 1.0 + log((double)x0[j].y);
                    v *= w0[j];
                    ent2[slot] = make_uint2(nr0[j], x0[j].y);
                    score[slot] = v;
                }
                // exactly +0.0 in a filtered lane and in a lane past the column's end: all 64 lanes are added, with constant
                // lane numbers (no loop, no lane index in a scalar register: the chain of 64 additions is what remains)
                const double sq = v * v;
#pragma unroll
                for (int k = 0; k < 64; ++k) sum_sq += read_lane(sq, k);
                d += (unsigned)__popcll(m);
            }
#pragma unroll
            for (int j = 0; j < VOC_U; ++j) {
                x0[j] = x1[j]; x1[j] = x2[j]; x2[j] = x3[j];
                nr0[j] = nr1[j]; nr1[j] = nr2[j];
                w0[j] = w1[j];
            }
        }
        const double D = 1.0 / sqrt(sum_sq);
        __threadfence_block();                                  // a slot is rescaled by another lane than the one that wrote it
        for (unsigned p = d0 + lane; p < d; p += 64) {
            double v = score[p] * D;
            if (v != v) v = __longlong_as_double((long long)0xFFF8000000000000ull);
            score[p] = v;
        }
    }
}

__global__ __launch_bounds__(VOC_BLOCK) void voc_narrow_kernel(const long long* __restrict__ in, i64 n, unsigned* __restrict__ out)
{
    for (i64 i = (i64)blockIdx.x * VOC_BLOCK + threadIdx.x; i < n; i += (i64)gridDim.x * VOC_BLOCK) out[i] = (unsigned)in[i];
}

}  // namespace

#define VOC_LAUNCH_CHECK()                                                                    \
    do {                                                                                      \
        hipError_t _e = hipGetLastError();                                                    \
        if (_e != hipSuccess) {                                                               \
            set_error(std::string("vocabulary kernel launch: ") + hipGetErrorString(_e));     \
            return -100;                                                                      \
        }                                                                                     \
    } while (0)

int voc_scatter(const unsigned* term, unsigned height, unsigned height_in, unsigned* old_to_new, hipStream_t st)
{
    voc_clear_kernel<<<thread_grid(height_in), VOC_BLOCK, 0, st>>>(old_to_new, height_in);
    voc_scatter_kernel<<<thread_grid(height), VOC_BLOCK, 0, st>>>(term, height, old_to_new);
    VOC_LAUNCH_CHECK();
    return 0;
}

int voc_count(const unsigned* cp, const uint2* ent, unsigned width, const unsigned* old_to_new, unsigned min_terms, unsigned* flag,
              unsigned* len, hipStream_t st)
{
    voc_count_kernel<<<wave_grid((i64)width + 1), VOC_BLOCK, 0, st>>>(cp, ent, width, old_to_new, min_terms, flag, len);
    VOC_LAUNCH_CHECK();
    return 0;
}

int voc_fill_score(const unsigned* cp, const uint2* ent, unsigned width, const unsigned* old_to_new, const double* idf,
                   const unsigned* flag, const unsigned* cpos, const unsigned* dst, unsigned* cp2, uint2* ent2, double* score,
                   unsigned* doc2, hipStream_t st)
{
    voc_fill_score_kernel<<<wave_grid((i64)width + 1), VOC_BLOCK, 0, st>>>(cp, ent, width, old_to_new, idf, flag, cpos, dst, cp2, ent2, score,
                                                                           doc2);
    VOC_LAUNCH_CHECK();
    return 0;
}

int voc_narrow_i64(const long long* in, i64 n, unsigned* out, hipStream_t st)
{
    if (n <= 0) return 0;
    voc_narrow_kernel<<<thread_grid(n), VOC_BLOCK, 0, st>>>(in, n, out);
    VOC_LAUNCH_CHECK();
    return 0;
}

}  // namespace smk
