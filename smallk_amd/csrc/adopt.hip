// smallk_amd/csrc/adopt.hip -- data that is already in device memory: strided views of fp64 / fp32 / bf16 / fp16 elements
// (a torch tensor's data_ptr and strides) into and out of the library's own layouts, and CSC arrays with 32- or 64-bit indices
// checked and converted.  One tile kernel serves every dense direction ("Device tensors in and out"):
//   * a 64 x 64 tile per workgroup of 256 threads, as transpose_kernel and fill_planted_kernel;
//   * the tile is read along the source's unit-stride dimension ("i"), four consecutive elements per lane;
//   * a destination whose unit-stride dimension is i too is written straight from the registers;
//   * a destination whose unit-stride dimension is the other one ("j") gets the tile through LDS, stored transposed with a
//     pitch of 65 (33) words so that a lane reads its four j-neighbours from one row; 16-bit elements are packed in pairs
//     along j BEFORE they are written to LDS, so no two lanes ever write halves of one bank word;
//   * both destinations at once = the fused form of launch_adopt_dense (A and the stored transpose from one read of the source);
//   * a 4-element access is one instruction (8 / 16 / 2 x 16 bytes) only where the base pointer and the leading stride are
//     aligned to it (tile offsets are multiples of 64 elements); a slice such as X[1:, 3:] takes four element-sized accesses.
// Views with no unit stride (X[:, ::2]), or whose source AND destination cannot be put in tile form, take plain_kernel.
// Conversion: to fp64 exactly; to anything narrower through fp32 (fp64 -> fp32 round-to-nearest-even, then fp32 -> bf16 / fp16
// round-to-nearest-even) -- store_cast<T>((float)x) of the host upload path, bit for bit.  Pad rows and columns of a destination
// are never written.
#include "common.h"
#include "devutil.h"

#include <type_traits>

namespace smk {

namespace {

struct bf16_t { unsigned short b; };

template <typename S> __device__ __forceinline__ float to_f32(S s) { return (float)s; }                // fp64: rounds to nearest even; fp16: exact
template <> __device__ __forceinline__ float to_f32<bf16_t>(bf16_t s) { return bf16_bits_to_f32(s.b); }

template <typename D> __device__ __forceinline__ D from_f32(float f) { return (D)f; }                  // fp16: rounds to nearest even
template <> __device__ __forceinline__ bf16_t from_f32<bf16_t>(float f) { return bf16_t{f32_to_bf16_rne(f)}; }

template <typename D, typename S>
__device__ __forceinline__ D convert(S s)
{
    if constexpr (std::is_same<D, S>::value) return s;
    else if constexpr (std::is_same<D, double>::value) return (double)to_f32(s);
    else return from_f32<D>(to_f32(s));
}

// four consecutive elements as one access where `vec` (the caller has checked the alignment), else one by one
template <typename T> struct alignas(sizeof(T) * 4 > 16 ? 16 : sizeof(T) * 4) Quad { T v[4]; };

constexpr int TILE = 64;

// src: unit stride along i, s_j elements between consecutive j.  dir (may be null): unit stride along i, dir_ldj along j.
// tr (may be null): unit stride along j, tr_ldi along i.  vec bits: 1 source, 2 dir, 4 tr.
template <typename S, typename D>
__global__ __launch_bounds__(256) void tile_convert_kernel(const S* __restrict__ src, i64 s_j, D* __restrict__ dir, i64 dir_ldj,
                                                           D* __restrict__ tr, i64 tr_ldi, i64 ni, i64 nj, int vec)
{
    // what one LDS word holds: the element itself, or two 16-bit elements (j even in the low half)
    using L = typename std::conditional<sizeof(D) == 2, unsigned, D>::type;
    constexpr int PER = sizeof(D) == 2 ? 2 : 1;          // elements along j per LDS word
    constexpr int PITCH = TILE / PER + 1;
    __shared__ L tile[TILE][PITCH];                      // [i][j / PER]

    const i64 i0 = (i64)blockIdx.x * TILE, j0 = (i64)blockIdx.y * TILE;
    const int t = threadIdx.x;
    const int ti = (t & 15) * 4, tj = t >> 4;            // four i-neighbours; rows j = 32 h + 2 tj + {0, 1}
    const i64 i = i0 + ti;
    const bool full_i = i + 3 < ni;

#pragma unroll
    for (int h = 0; h < 2; ++h) {
        D out[2][4];
#pragma unroll
        for (int q = 0; q < 2; ++q) {
            const i64 j = j0 + 32 * h + 2 * tj + q;
            S in[4];
            if (j < nj && full_i && (vec & 1)) {
                const Quad<S> v = *(const Quad<S>*)(src + j * s_j + i);
#pragma unroll
                for (int e = 0; e < 4; ++e) in[e] = v.v[e];
            } else {
#pragma unroll
                for (int e = 0; e < 4; ++e) in[e] = (j < nj && i + e < ni) ? src[j * s_j + i + e] : S{};
            }
#pragma unroll
            for (int e = 0; e < 4; ++e) out[q][e] = convert<D>(in[e]);
            if (dir && j < nj) {
                D* p = dir + j * dir_ldj + i;
                if (full_i && (vec & 2)) {
                    Quad<D> v;
#pragma unroll
                    for (int e = 0; e < 4; ++e) v.v[e] = out[q][e];
                    *(Quad<D>*)p = v;
                } else {
#pragma unroll
                    for (int e = 0; e < 4; ++e) if (i + e < ni) p[e] = out[q][e];
                }
            }
        }
        if (tr) {
            const int jl = 32 * h + 2 * tj;              // local j of out[0]
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                if constexpr (PER == 2) {
                    tile[ti + e][jl >> 1] = (unsigned)__builtin_bit_cast(unsigned short, out[0][e]) |
                                            ((unsigned)__builtin_bit_cast(unsigned short, out[1][e]) << 16);
                } else {
                    tile[ti + e][jl] = out[0][e];
                    tile[ti + e][jl + 1] = out[1][e];
                }
            }
        }
    }
    if (!tr) return;                                     // uniform over the grid
    __syncthreads();
    // the transposed side: a lane takes four j-neighbours of one i
    const int uj = (t & 15) * 4, ui = t >> 4;
    const i64 j = j0 + uj;
    const bool full_j = j + 3 < nj;
#pragma unroll
    for (int r = 0; r < 4; ++r) {
        const int il = ui + 16 * r;
        const i64 ig = i0 + il;
        if (ig >= ni) continue;
        Quad<D> v;
        if constexpr (PER == 2) {
            const unsigned w0 = tile[il][uj >> 1], w1 = tile[il][(uj >> 1) + 1];
            v.v[0] = __builtin_bit_cast(D, (unsigned short)(w0 & 0xFFFFu));
            v.v[1] = __builtin_bit_cast(D, (unsigned short)(w0 >> 16));
            v.v[2] = __builtin_bit_cast(D, (unsigned short)(w1 & 0xFFFFu));
            v.v[3] = __builtin_bit_cast(D, (unsigned short)(w1 >> 16));
        } else {
#pragma unroll
            for (int e = 0; e < 4; ++e) v.v[e] = tile[il][uj + e];
        }
        D* p = tr + ig * tr_ldi + j;
        if (full_j && (vec & 4)) {
            *(Quad<D>*)p = v;
        } else {
#pragma unroll
            for (int e = 0; e < 4; ++e) if (j + e < nj) p[e] = v.v[e];
        }
    }
}

// any strides (0 included): one element per thread and step, the index that runs fastest is the one the caller names
template <typename S, typename D>
__global__ __launch_bounds__(256) void plain_convert_kernel(const S* __restrict__ src, i64 s_f, i64 s_o, D* __restrict__ dst, i64 d_f,
                                                            i64 d_o, i64 nf, i64 no)
{
    const i64 total = nf * no;
    for (i64 idx = (i64)blockIdx.x * blockDim.x + threadIdx.x; idx < total; idx += (i64)gridDim.x * blockDim.x) {
        const i64 o = idx / nf, f = idx - o * nf;
        dst[f * d_f + o * d_o] = convert<D>(src[f * s_f + o * s_o]);
    }
}

inline bool aligned4(const void* p, i64 ld_elems, size_t es)
{
    const size_t a = es * 4 > 16 ? 16 : es * 4;
    return p && (uintptr_t)p % a == 0 && ((size_t)ld_elems * es) % a == 0;
}

template <typename S, typename D>
int launch_tile(const void* src, i64 s_j, void* dir, i64 dir_ldj, void* tr, i64 tr_ldi, i64 ni, i64 nj, hipStream_t st)
{
    const i64 gi = (ni + TILE - 1) / TILE, gj = (nj + TILE - 1) / TILE;
    if (gi > 0x7FFFFFFF || gj > 65535) return 1;                         // the caller takes the plain path
    const int vec = (aligned4(src, s_j, sizeof(S)) ? 1 : 0) | (aligned4(dir, dir_ldj, sizeof(D)) ? 2 : 0) |
                    (aligned4(tr, tr_ldi, sizeof(D)) ? 4 : 0);
    tile_convert_kernel<S, D><<<dim3((unsigned)gi, (unsigned)gj), 256, 0, st>>>((const S*)src, s_j, (D*)dir, dir_ldj, (D*)tr, tr_ldi,
                                                                                  ni, nj, vec);
    SMK_HIP(hipGetLastError());
    return 0;
}

template <typename S, typename D>
int launch_plain(const void* src, i64 s_f, i64 s_o, void* dst, i64 d_f, i64 d_o, i64 nf, i64 no, hipStream_t st)
{
    const i64 blocks = (nf * no + 255) / 256;
    plain_convert_kernel<S, D><<<(unsigned)(blocks < 8192 ? blocks : 8192), 256, 0, st>>>((const S*)src, s_f, s_o, (D*)dst, d_f, d_o, nf, no);
    SMK_HIP(hipGetLastError());
    return 0;
}

// CALL is a statement that uses the types S and D
#define SMK_DT_CASE(V, TYPE, NAME, BODY) case V: { using NAME = TYPE; BODY; } break;
#define SMK_DT_SWITCH(DT, NAME, BODY)                                  \
    switch (DT) {                                                      \
        SMK_DT_CASE(DT_F64, double, NAME, BODY)                        \
        SMK_DT_CASE(DT_F32, float, NAME, BODY)                         \
        SMK_DT_CASE(DT_BF16, bf16_t, NAME, BODY)                       \
        SMK_DT_CASE(DT_F16, _Float16, NAME, BODY)                      \
        default: set_error("unknown element type"); return -3;         \
    }

// the source's unit-stride dimension as i: 0 rows, 1 columns, -1 none
inline int unit_dim(i64 rs, i64 cs, i64 rows, i64 cols)
{
    if (rs == 1 && cs == 1) return rows >= cols ? 0 : 1;
    return rs == 1 ? 0 : cs == 1 ? 1 : -1;
}

}  // namespace

int launch_strided_convert(const void* src, int src_dtype, i64 src_rs, i64 src_cs, void* dst, int dst_dtype, i64 dst_rs, i64 dst_cs,
                           i64 rows, i64 cols, hipStream_t st)
{
    if (rows <= 0 || cols <= 0) return 0;
    const int ud = unit_dim(src_rs, src_cs, rows, cols);
    int rc = 1;
    if (ud >= 0) {
        const i64 s_j = ud == 0 ? src_cs : src_rs, ni = ud == 0 ? rows : cols, nj = ud == 0 ? cols : rows;
        const i64 d_i = ud == 0 ? dst_rs : dst_cs, d_j = ud == 0 ? dst_cs : dst_rs;
        if (d_i == 1 || d_j == 1) {
            void* dir = d_i == 1 ? dst : nullptr;
            void* tr = d_i == 1 ? nullptr : dst;
            SMK_DT_SWITCH(src_dtype, S, SMK_DT_SWITCH(dst_dtype, D, rc = (launch_tile<S, D>(src, s_j, dir, d_j, tr, d_i, ni, nj, st))))
        }
    }
    if (rc != 1) return rc;
    // the plain path: fastest along the destination's smaller stride
    const bool rows_fast = dst_rs <= dst_cs;
    const i64 nf = rows_fast ? rows : cols, no = rows_fast ? cols : rows;
    SMK_DT_SWITCH(src_dtype, S, SMK_DT_SWITCH(dst_dtype, D, rc = (launch_plain<S, D>(src, rows_fast ? src_rs : src_cs, rows_fast ? src_cs : src_rs, dst,
                                                                                   rows_fast ? dst_rs : dst_cs, rows_fast ? dst_cs : dst_rs, nf, no, st))))
    return rc;
}

int launch_adopt_dense(const void* src, int src_dtype, i64 src_rs, i64 src_cs, void* A, i64 ldA, void* At, i64 ldAt, int storage, i64 rows,
                       i64 cols, hipStream_t st)
{
    if (rows <= 0 || cols <= 0) return 0;
    const int dst_dtype = storage == STORE_BF16 ? DT_BF16 : DT_F32;
    const int ud = unit_dim(src_rs, src_cs, rows, cols);
    if (ud >= 0) {
        // column-major source: A straight from the registers, A' through LDS; row-major source: the other way round
        const i64 s_j = ud == 0 ? src_cs : src_rs, ni = ud == 0 ? rows : cols, nj = ud == 0 ? cols : rows;
        void* dir = ud == 0 ? A : At;
        void* tr = ud == 0 ? At : A;
        const i64 dir_ld = ud == 0 ? ldA : ldAt, tr_ld = ud == 0 ? ldAt : ldA;
        int rc = 1;
        SMK_DT_SWITCH(src_dtype, S, SMK_DT_SWITCH(dst_dtype, D, rc = (launch_tile<S, D>(src, s_j, dir, dir_ld, tr, tr_ld, ni, nj, st))))
        if (rc != 1) return rc;
    }
    int rc = launch_strided_convert(src, src_dtype, src_rs, src_cs, A, dst_dtype, 1, ldA, rows, cols, st);
    if (!rc && At) rc = launch_strided_convert(src, src_dtype, src_rs, src_cs, At, dst_dtype, ldAt, 1, rows, cols, st);
    return rc;
}

// ---- CSC arrays in device memory ---------------------------------------------------------------------------------------------
namespace {

// flag bits: 1 offsets not monotone, 2 offsets do not run from 0 to nnz, 4 a row index >= height (or negative), 8 an offset that
// does not fit 32 bits (or negative).  Reads offsets[0 .. width] and rows[0 .. nnz) and nothing else.
template <typename IO, typename IR>
__global__ __launch_bounds__(256) void csc_validate_kernel(const IO* __restrict__ offsets, i64 width, i64 nnz, const IR* __restrict__ rows,
                                                           i64 height, unsigned* __restrict__ flag)
{
    unsigned bad = 0;
    const i64 stride = (i64)gridDim.x * blockDim.x, t0 = (i64)blockIdx.x * blockDim.x + threadIdx.x;
    for (i64 c = t0; c <= width; c += stride) {
        const i64 v = (i64)offsets[c];
        if (v < 0 || v > 0xFFFFFFFFll) bad |= 8u;
        if (c > 0 && v < (i64)offsets[c - 1]) bad |= 1u;
        if ((c == 0 && v != 0) || (c == width && v != nnz)) bad |= 2u;
    }
    for (i64 p = t0; p < nnz; p += stride) {
        const i64 r = (i64)rows[p];
        if (r < 0 || r >= height) bad |= 4u;
    }
    if (bad) atomicOr(flag, bad);
}

template <typename I, typename O>
__global__ __launch_bounds__(256) void index_convert_kernel(const I* __restrict__ in, O* __restrict__ out, i64 n)
{
    for (i64 p = (i64)blockIdx.x * blockDim.x + threadIdx.x; p < n; p += (i64)gridDim.x * blockDim.x) out[p] = (O)in[p];
}

inline unsigned blocks_for(i64 n) { const i64 b = (n + 255) / 256; return (unsigned)(b < 1 ? 1 : b < 4096 ? b : 4096); }

}  // namespace

int launch_csc_validate(const void* offsets, int idx_type, i64 width, i64 nnz, const void* rows, int row_idx_type, i64 height, unsigned* flag,
                        hipStream_t st)
{
    SMK_HIP(hipMemsetAsync(flag, 0, sizeof(unsigned), st));
    const unsigned g = blocks_for(nnz > width + 1 ? nnz : width + 1);
    if (idx_type == IDX_I64 && row_idx_type == IDX_I64)
        csc_validate_kernel<long long, long long><<<g, 256, 0, st>>>((const long long*)offsets, width, nnz, (const long long*)rows, height, flag);
    else if (idx_type == IDX_I64)
        csc_validate_kernel<long long, int><<<g, 256, 0, st>>>((const long long*)offsets, width, nnz, (const int*)rows, height, flag);
    else if (row_idx_type == IDX_I64)
        csc_validate_kernel<int, long long><<<g, 256, 0, st>>>((const int*)offsets, width, nnz, (const long long*)rows, height, flag);
    else
        csc_validate_kernel<int, int><<<g, 256, 0, st>>>((const int*)offsets, width, nnz, (const int*)rows, height, flag);
    SMK_HIP(hipGetLastError());
    return 0;
}

// validated arrays -> the resident layout: 64-bit offsets, 32-bit row indices
int launch_csc_convert(const void* offsets, int idx_type, i64 width, i64 nnz, const void* rows, int row_idx_type, i64* colptr, unsigned* rowidx,
                       hipStream_t st)
{
    if (idx_type == IDX_I64) index_convert_kernel<long long, i64><<<blocks_for(width + 1), 256, 0, st>>>((const long long*)offsets, colptr, width + 1);
    else index_convert_kernel<int, i64><<<blocks_for(width + 1), 256, 0, st>>>((const int*)offsets, colptr, width + 1);
    SMK_HIP(hipGetLastError());
    if (nnz > 0) {
        if (row_idx_type == IDX_I64) index_convert_kernel<long long, unsigned><<<blocks_for(nnz), 256, 0, st>>>((const long long*)rows, rowidx, nnz);
        else index_convert_kernel<int, unsigned><<<blocks_for(nnz), 256, 0, st>>>((const int*)rows, rowidx, nnz);
        SMK_HIP(hipGetLastError());
    }
    return 0;
}

}  // namespace smk
