// smallk_amd/csrc/matrix.cpp -- the resident matrix of the C ABI (include/smallk_amd.h): dense A with or without its
// stored transpose, sparse A as CSC(A) + CSC(A'), uploads, fills, column subsets, and the parts built on first use
// (stored transpose of a single copy, segment plans, scale and norms, host copy of the CSC).
#include "entry.h"

#include <cmath>
#include <cstdio>
#include <cstring>
#include <functional>
#include <mutex>
#include <string>

namespace smk {

// a matrix of the calling thread's context, registered with it; nothing allocated yet
static smk_matrix* new_matrix(i64 m, i64 n_global, i64 c0, i64 n, int storage, bool sparse = false, i64 nnz = 0)
{
    smk_matrix* a = new smk_matrix;
    a->m = m; a->n_global = n_global; a->c0 = c0; a->n = n; a->storage = storage; a->sparse = sparse; a->nnz = nnz;
    a->st = ctx().stream;
    register_matrix(a);
    return a;
}

// a single-copy matrix meets a consumer of the stored transpose (BPP, RANK2, the accurate form, column subsets): allocate and fill
// it now; solvers already planned on the transposed source keep reading A (their plans say so)
int matrix_materialize_transpose(const smk_matrix* ca)
{
    smk_matrix* a = const_cast<smk_matrix*>(ca);       // the lazily built parts of a matrix (scales, blocked CSC, segment plans) are filled the same way
    static std::mutex mu;
    std::lock_guard<std::mutex> lk(mu);
    if (!a->single || a->At) return 0;
    const size_t es = (size_t)elem_size(a->storage);
    hipStream_t st = matrix_stream(a);
    if (a->own.dev((unsigned char**)&a->At, (size_t)a->ldAt * a->colsAt * es)) { set_error("no memory for the stored transpose of a single-copy matrix"); return SMK_DEVICE_ERROR; }
    SMK_HIP(hipMemsetAsync(a->At, 0, (size_t)a->ldAt * a->colsAt * es, st));
    const int rc = launch_transpose_store(a->A, a->ldA, a->At, a->ldAt, a->storage, a->m, a->n, st);
    if (rc) return rc;
    SMK_HIP(hipStreamSynchronize(st));
    a->single = false;
    return 0;
}

int ensure_seg_plans(const smk_matrix* a)
{
    // lazily built part of a shared, nominally const matrix: same lock discipline as matrix_materialize_transpose
    static std::mutex mu;
    std::lock_guard<std::mutex> lk(mu);
    if (a->seg_tried) return 0;
    a->seg_tried = true;
    const bool seg_on = sw::spmm_seg();
    hipStream_t bst = matrix_stream(a);
    if (seg_on && (build_seg_plan(a->n, a->nnz, a->colptr, a->rowidx, &a->segA, bst) ||
                   build_seg_plan(a->m, a->nnz, a->colptr_t, a->rowidx_t, &a->segAt, bst))) {
        free_seg_plan(&a->segA);
        free_seg_plan(&a->segAt);
    }
    return 0;
}

// One pass over a dense A at HBM rate, once per matrix contents: the column maxima of |A| give
//   ascale          power of two with max |A| ascale in [2^13, 2^14) (fp16 two-term products; 1 for an all-zero matrix)
//   col_spread_log2 log2 of (largest / smallest non-zero column maximum): how far apart the column scales are
int matrix_measure_scale(const smk_matrix* a, hipStream_t st)
{
    Scratch<unsigned> d;
    SMK_HIP(smk::dev_malloc(d.put(), 2 * sizeof(unsigned)));
    unsigned bits[2] = {0, 0};
    int rc = launch_colrange(a->A, a->storage, a->ldA, a->m, a->n, d, st);
    if (!rc && hipMemcpyAsync(bits, d, sizeof(bits), hipMemcpyDeviceToHost, st) != hipSuccess) rc = SMK_DEVICE_ERROR;
    if (!rc && hipStreamSynchronize(st) != hipSuccess) rc = SMK_DEVICE_ERROR;
    if (rc) { set_error("could not measure max |A|"); return rc; }
    float mx, mn;
    memcpy(&mx, &bits[0], sizeof(mx));
    memcpy(&mn, &bits[1], sizeof(mn));
    float sc = 1.f;
    int spread = 0;
    if (mx > 0.f && std::isfinite(mx)) {
        int ex = 0;
        (void)frexpf(mx, &ex);                     // mx = f 2^ex, f in [0.5, 1)
        sc = ldexpf(1.f, 14 - ex);
        if (bits[1] != 0xFFFFFFFFu && mn > 0.f) { int en = 0; (void)frexpf(mn, &en); spread = ex - en; }
    }
    a->ascale = sc;
    a->col_spread_log2 = spread;
    return 0;
}

// One pass over A and one over A' at HBM rate, once per matrix contents: the largest 2-norm of a column and of a row
// (what bounds the NNLS solutions from above, NnlsPack)
int matrix_measure_norms(const smk_matrix* a, hipStream_t st)
{
    Scratch<double> d;
    SMK_HIP(smk::dev_malloc(d.put(), 2 * sizeof(double)));
    double v[2] = {0.0, 0.0};
    int rc = launch_colnorm2_max(a->A, a->storage, a->ldA, a->m, a->n, d, st);
    if (!rc) rc = launch_colnorm2_max(a->At, a->storage, a->ldAt, a->n, a->m, d + 1, st);
    if (!rc && hipMemcpyAsync(v, d, sizeof(v), hipMemcpyDeviceToHost, st) != hipSuccess) rc = SMK_DEVICE_ERROR;
    if (!rc && hipStreamSynchronize(st) != hipSuccess) rc = SMK_DEVICE_ERROR;
    if (rc) { set_error("could not measure the column / row norms of A"); return rc; }
    a->colnorm_max = std::sqrt(v[0]);
    a->rownorm_max = std::sqrt(v[1]);
    return 0;
}

// ---- views in device memory handed in by a caller ------------------------------------------------------------------------
// last element of a rows x cols view, in bytes from its first one, and whether [offset, offset + that + elem_size) stays inside
// alloc_bytes; every step in 64-bit integers with the overflow checked (a view of 2^40 elements is ordinary arithmetic here)
static bool strided_extent_fits(i64 rows, i64 cols, i64 rs, i64 cs, i64 es, i64 offset_bytes, i64 alloc_bytes)
{
    if (rows <= 0 || cols <= 0 || rs < 0 || cs < 0 || es <= 0 || offset_bytes < 0 || alloc_bytes < 0) return false;
    i64 a, b, last, end;
    if (__builtin_mul_overflow(rows - 1, rs, &a) || __builtin_mul_overflow(cols - 1, cs, &b) || __builtin_add_overflow(a, b, &last) ||
        __builtin_add_overflow(last, (i64)1, &last) || __builtin_mul_overflow(last, es, &end) || __builtin_add_overflow(end, offset_bytes, &end))
        return false;
    return end <= alloc_bytes;
}

int check_device_view(const void* p, int dtype, i64 rows, i64 cols, i64 rs, i64 cs, bool output, const char* what)
{
    const std::string w(what);
    if (!p) { set_error(w + ": null pointer"); return SMK_BAD_PARAM; }
    const int es = dtype_size(dtype);
    if (!es) { set_error(w + ": unknown element type"); return SMK_BAD_PARAM; }
    if (rs < 0 || cs < 0) { set_error(w + ": negative stride"); return SMK_BAD_PARAM; }
    if (output && ((rs == 0 && rows > 1) || (cs == 0 && cols > 1) || (rows > 1 && cols > 1 && rs == cs))) {
        set_error(w + ": the elements of an output overlap");
        return SMK_BAD_PARAM;
    }
    int dev = -1;
    hipPointerAttribute_t at;
    if (hipGetDevice(&dev) != hipSuccess || hipPointerGetAttributes(&at, p) != hipSuccess || at.type != hipMemoryTypeDevice || at.device != dev) {
        (void)hipGetLastError();              // a host pointer is reported as an error by some runtimes: it is not one of ours
        set_error(w + ": not a pointer to memory of the current device");
        return SMK_BAD_PARAM;
    }
    hipDeviceptr_t base = nullptr;
    size_t size = 0;
    if (hipMemGetAddressRange(&base, &size, (hipDeviceptr_t)p) != hipSuccess) {
        (void)hipGetLastError();
        set_error(w + ": the allocation behind the pointer is unknown to the runtime");
        return SMK_BAD_PARAM;
    }
    if (!strided_extent_fits(rows, cols, rs, cs, es, (i64)((const char*)p - (const char*)base), (i64)size)) {
        set_error(w + ": the strided extent leaves the allocation");
        return SMK_BAD_PARAM;
    }
    return SMK_OK;
}

int join_caller_stream(Owned& own, hipStream_t lib, void* caller_stream)
{
    hipStream_t caller = (hipStream_t)caller_stream;
    if (caller == lib) return 0;
    hipEvent_t ev;
    if (own.event(&ev, hipEventDisableTiming)) return SMK_DEVICE_ERROR;
    SMK_HIP(hipEventRecord(ev, caller));
    SMK_HIP(hipStreamWaitEvent(lib, ev, 0));
    return 0;
}

}  // namespace smk

extern "C" {

int smk_strided_extent_fits(int64_t rows, int64_t cols, int64_t row_stride, int64_t col_stride, int64_t elem_size, int64_t offset_bytes,
                            int64_t alloc_bytes)
{
    return strided_extent_fits(rows, cols, row_stride, col_stride, elem_size, offset_bytes, alloc_bytes) ? 1 : 0;
}

static thread_local bool g_create_single = false;
int smk_matrix_create(smk_matrix** out, int64_t height, int64_t width_global, int64_t col0, int64_t ncols_local,
                      int storage)
{
    if (!out) return SMK_BAD_PARAM;
    *out = nullptr;
    if (int rc = require_init()) return rc;
    if (height <= 0 || width_global <= 0 || ncols_local <= 0 || col0 < 0 || col0 + ncols_local > width_global ||
        (storage != SMK_STORE_F32 && storage != SMK_STORE_BF16))
        return SMK_BAD_PARAM;
    smk_matrix* a = new_matrix(height, width_global, col0, ncols_local, storage);
    // rows of A padded to COL_PAD, not ROW_PAD: a single-copy matrix is also read through the transposed source, whose tiles are
    // 128 ROWS of A and whose chunked passes (sharded runs, chunk_rows) run to round_up(m, COL_PAD) -- with 128-row padding a
    // height with 0 < m mod 256 <= 128 let the last tile read 128 rows past the column (the next column's data; past the
    // allocation in the last column).  The pad rows are zero like every other pad.
    a->ldA = round_up(height, COL_PAD);      a->colsA = round_up(ncols_local, COL_PAD);
    a->ldAt = round_up(ncols_local, ROW_PAD); a->colsAt = round_up(height, COL_PAD);
    const size_t es = (size_t)elem_size(storage);
    // A column stride that is a multiple of 1 MiB gets ROW_PAD more (zero) rows: with the 128 columns of a workgroup's stage
    // exactly 2^20 bytes apart the W'A pass of C4 runs 3 % slower (11.3 -> 10.95 ms) and that of a C4 shard 8 % (1.60 ->
    // 1.47 ms; bench.py --emulate-world 8: 3.28 -> 3.15 ms per rank).  Smaller power-of-two strides are best left alone
    // (C3: 128 KiB and 32 KiB strides, skewed: 1200 -> 1130 / 980 it/s); 256 and 384 rows more gain less than 128.
    // SMK_LD_SKEW=0 turns it off, =n asks for n rows.  (profiles/r04_leading_dimension_skew.txt)
    {
        const i64 skew = sw::ld_skew().set ? sw::ld_skew().v / ROW_PAD * ROW_PAD : ROW_PAD;
        if (skew > 0 && ((size_t)a->ldA * es) % ((size_t)1 << 20) == 0) a->ldA += skew;
        if (skew > 0 && ((size_t)a->ldAt * es) % ((size_t)1 << 20) == 0) a->ldAt += skew;
    }
    {   // SMK_SINGLE_COPY=1: dense matrices are created without the stored transpose (smk_matrix_create_single_copy asks for it explicitly)
        a->single = g_create_single || sw::single_copy();
    }
    if (a->own.dev((unsigned char**)&a->A, (size_t)a->ldA * a->colsA * es)) { smk_matrix_destroy(a); return SMK_DEVICE_ERROR; }
    if (!a->single && a->own.dev((unsigned char**)&a->At, (size_t)a->ldAt * a->colsAt * es)) {
        // A fits, A and A' together do not: the matrix becomes a single copy (MU, HALS and BPP with the 16-bit product forms run
        // on it as they are; RANK2 and the accurate form will ask for the transpose and report the allocation failure then)
        (void)hipGetLastError();
        a->own.drop(&a->At);
        a->single = true;
    }
    hipError_t e1 = hipMemsetAsync(a->A, 0, (size_t)a->ldA * a->colsA * es, ctx().stream);
    if (e1 == hipSuccess && a->At) e1 = hipMemsetAsync(a->At, 0, (size_t)a->ldAt * a->colsAt * es, ctx().stream);
    if (e1 != hipSuccess) {
        set_error(std::string("hipMemsetAsync(A): ") + hipGetErrorString(e1));
        smk_matrix_destroy(a);
        return SMK_DEVICE_ERROR;
    }
    *out = a;
    return SMK_OK;
}

int smk_matrix_create_single_copy(smk_matrix** out, int64_t height, int64_t width_global, int64_t col0, int64_t ncols_local,
                                  int storage)
{
    g_create_single = true;
    const int rc = smk_matrix_create(out, height, width_global, col0, ncols_local, storage);
    g_create_single = false;
    return rc;
}
int smk_matrix_is_single_copy(const smk_matrix* a) { return a && a->single ? 1 : 0; }
// bytes of HBM the resident matrix occupies (A, the stored transpose when there is one, the CSC arrays of a sparse matrix)
int64_t smk_matrix_device_bytes(const smk_matrix* a)
{
    if (!a) return 0;
    if (a->sparse) return (int64_t)((size_t)(a->n + 1 + a->m + 1) * sizeof(i64) + 2 * (size_t)a->nnz * (sizeof(unsigned) + sizeof(double)));
    const size_t es = (size_t)elem_size(a->storage);
    return (int64_t)((size_t)a->ldA * a->colsA * es + (a->At ? (size_t)a->ldAt * a->colsAt * es : 0));
}

static int matrix_make_transpose(smk_matrix* a)
{
    if (a->single) return 0;
    return launch_transpose_store(a->A, a->ldA, a->At, a->ldAt, a->storage, a->m, a->n, ctx().stream);
}

// ---- host fp64 -> resident matrix ---------------------------------------------------------------------------------------
// The reference wraps the caller's buffer as a view, no copy (common/src/nmf.cpp:224-226); here A has to cross PCIe once, and this
// is the path every reference caller takes (nmf/src/main.cpp:218-233, smallk.cpp:604-619, smallk_lib.pyx:769).  The loop is plain:
// hipMemcpy2DAsync straight from the caller's pageable buffer into one 64 MB device staging buffer, conversion to the stored type,
// synchronise, next chunk; the stored transpose in one device pass at the end.  Round 6 MEASURED it before replacing it
// (profiles/r06_upload_rates.txt, bench.py --api-path): 50 - 55 GB/s on C3's 8.6 GB, on a C4 shard's 17 GB and on C2's 0.27 GB -- the
// runtime pins the pageable pages in place piece by piece and the per-chunk synchronisation costs nothing measurable.  Two
// pipelined variants were built and timed against it on the same box: pinned staging buffers filled by 2 - 16 host threads with the
// transfer and the conversion overlapped (41 GB/s whatever the thread count, 10 - 19 GB/s on C2's matrix: the pinned allocations)
// and hipHostRegister of each chunk of the caller's buffer (52 GB/s).  Both slower, both removed.
int smk_matrix_upload_f64(smk_matrix* a, const double* host, int64_t ld)
{
    if (a) { a->ascale = 0.f; a->col_spread_log2 = -1; a->colnorm_max = a->rownorm_max = -1.0; a->kl_negative = -1; }     // new contents: scale, column spread and norms are measured again on first use
    if (!a || !host || ld < a->m || a->sparse) return SMK_BAD_PARAM;
    const size_t budget = (size_t)64 << 20;   // staging bytes
    i64 chunk = (i64)(budget / ((size_t)a->m * sizeof(double)));
    if (chunk < 1) chunk = 1;
    if (chunk > a->n) chunk = a->n;
    Scratch<double> stage;
    int rc = stage.alloc((size_t)a->m * chunk);
    if (rc) return rc;
    const size_t es = (size_t)elem_size(a->storage);
    for (i64 c = 0; c < a->n; c += chunk) {
        const i64 nc = (a->n - c < chunk) ? (a->n - c) : chunk;
        SMK_HIP(hipMemcpy2DAsync(stage, (size_t)a->m * sizeof(double), host + c * ld, (size_t)ld * sizeof(double),
                                 (size_t)a->m * sizeof(double), (size_t)nc, hipMemcpyHostToDevice, ctx().stream));
        rc = launch_convert_f64(stage, a->m, (unsigned char*)a->A + (size_t)c * a->ldA * es, a->storage, a->ldA,
                                a->m, nc, ctx().stream);
        if (rc) return rc;
        SMK_HIP(hipStreamSynchronize(ctx().stream));
    }
    rc = matrix_make_transpose(a);
    if (rc) return rc;
    SMK_HIP(hipStreamSynchronize(ctx().stream));
    return SMK_OK;
}

int smk_matrix_fill_uniform(smk_matrix* a, uint64_t seed)
{
    if (a) { a->ascale = 0.f; a->col_spread_log2 = -1; a->colnorm_max = a->rownorm_max = -1.0; a->kl_negative = -1; }
    if (!a || a->sparse) return SMK_BAD_PARAM;
    int rc = launch_fill_uniform(a->A, a->storage, a->ldA, a->m, a->n, a->ldA, a->colsA, 0, a->c0, a->m, seed,
                                 a->storage == SMK_STORE_BF16 ? 1 : 0, ctx().stream);
    if (rc) return rc;
    rc = matrix_make_transpose(a);
    if (rc) return rc;
    SMK_HIP(hipStreamSynchronize(ctx().stream));
    return SMK_OK;
}

int smk_matrix_fill_planted(smk_matrix* a, uint64_t seed, int kstar, double threshold, double noise)
{
    if (a) { a->ascale = 0.f; a->col_spread_log2 = -1; a->colnorm_max = a->rownorm_max = -1.0; a->kl_negative = -1; }
    if (!a || a->sparse || kstar < 1 || kstar > 4096 || !(threshold >= 0.0 && threshold < 1.0) || !(noise >= 0.0)) return SMK_BAD_PARAM;
    int rc = launch_fill_planted(a->A, a->storage, a->ldA, a->m, a->n, a->ldA, a->colsA, a->c0, a->m, seed, kstar, threshold,
                                 noise, a->storage == SMK_STORE_BF16 ? 1 : 0, ctx().stream);
    if (rc) return rc;
    rc = matrix_make_transpose(a);
    if (rc) return rc;
    SMK_HIP(hipStreamSynchronize(ctx().stream));
    return SMK_OK;
}

int smk_matrix_download_f64(const smk_matrix* a, double* host, int64_t ld)
{
    if (!a || !host || ld < a->m || a->sparse) return SMK_BAD_PARAM;
    const size_t es = (size_t)elem_size(a->storage);
    std::vector<unsigned char> col((size_t)a->m * es);
    SMK_HIP(hipStreamSynchronize(ctx().stream));
    for (i64 c = 0; c < a->n; ++c) {
        SMK_HIP(hipMemcpy(col.data(), (const unsigned char*)a->A + (size_t)c * a->ldA * es, (size_t)a->m * es,
                          hipMemcpyDeviceToHost));
        if (a->storage == SMK_STORE_BF16) {
            const uint16_t* p = (const uint16_t*)col.data();
            for (i64 r = 0; r < a->m; ++r) {
                uint32_t b = ((uint32_t)p[r]) << 16;
                float f;
                memcpy(&f, &b, 4);
                host[c * ld + r] = (double)f;
            }
        } else {
            const float* p = (const float*)col.data();
            for (i64 r = 0; r < a->m; ++r) host[c * ld + r] = (double)p[r];
        }
    }
    return SMK_OK;
}

// ---- device memory -> resident matrix -> device memory ("Device tensors in and out") -----------------------------
// The device twin of smk_matrix_upload_f64: nothing crosses PCIe, and A and the stored transpose come from one read of the
// source (adopt.hip) instead of a conversion pass and a transpose pass that reads A again.
int smk_matrix_adopt_device(smk_matrix* a, const void* src, int dtype, int64_t row_stride, int64_t col_stride, void* stream)
{
    if (a) { a->ascale = 0.f; a->col_spread_log2 = -1; a->colnorm_max = a->rownorm_max = -1.0; a->kl_negative = -1; }     // new contents, as in smk_matrix_upload_f64
    if (!a || a->sparse) return SMK_BAD_PARAM;
    int rc = check_device_view(src, dtype, a->m, a->n, row_stride, col_stride, false, "smk_matrix_adopt_device");
    if (rc) return rc;
    Owned own;
    rc = join_caller_stream(own, ctx().stream, stream);
    if (rc) return rc;
    rc = launch_adopt_dense(src, dtype, row_stride, col_stride, a->A, a->ldA, a->single ? nullptr : a->At, a->ldAt, a->storage, a->m, a->n,
                            ctx().stream);
    if (rc) return rc;
    SMK_HIP(hipStreamSynchronize(ctx().stream));
    return SMK_OK;
}

int smk_matrix_copy_to_device(const smk_matrix* a, void* dst, int dtype, int64_t row_stride, int64_t col_stride, void* stream)
{
    if (!a || a->sparse) return SMK_BAD_PARAM;
    int rc = check_device_view(dst, dtype, a->m, a->n, row_stride, col_stride, true, "smk_matrix_copy_to_device");
    if (rc) return rc;
    Owned own;
    rc = join_caller_stream(own, ctx().stream, stream);      // what the caller's stream still does with dst comes first
    if (rc) return rc;
    rc = launch_strided_convert(a->A, a->storage == SMK_STORE_BF16 ? DT_BF16 : DT_F32, 1, a->ldA, dst, dtype, row_stride, col_stride, a->m,
                                a->n, ctx().stream);
    if (rc) return rc;
    SMK_HIP(hipStreamSynchronize(ctx().stream));
    return SMK_OK;
}

int smk_matrix_create_sparse_device(smk_matrix** out, int64_t height, int64_t width, int64_t nnz, const void* col_offsets, int idx_type,
                                    const void* row_indices, int row_idx_type, const void* values, int dtype, void* stream)
{
    if (!out) return SMK_BAD_PARAM;
    *out = nullptr;
    if (int rc = require_init()) return rc;
    if (height <= 0 || width <= 0 || nnz <= 0 || height > 0xFFFFFFFFll) { set_error("smk_matrix_create_sparse_device: empty or oversized matrix"); return SMK_BAD_PARAM; }
    if ((idx_type != SMK_IDX_I32 && idx_type != SMK_IDX_I64) || (row_idx_type != SMK_IDX_I32 && row_idx_type != SMK_IDX_I64)) {
        set_error("smk_matrix_create_sparse_device: unknown index type");
        return SMK_BAD_PARAM;
    }
    // the three arrays as views of 8- / 4- / 2-byte elements: same pointer and extent checks as a dense view
    const auto idx_dt = [](int t) { return t == SMK_IDX_I64 ? (int)DT_F64 : (int)DT_F32; };
    int rc = check_device_view(col_offsets, idx_dt(idx_type), width + 1, 1, 1, width + 1, false, "smk_matrix_create_sparse_device(col_offsets)");
    if (!rc) rc = check_device_view(row_indices, idx_dt(row_idx_type), nnz, 1, 1, nnz, false, "smk_matrix_create_sparse_device(row_indices)");
    if (!rc) rc = check_device_view(values, dtype, nnz, 1, 1, nnz, false, "smk_matrix_create_sparse_device(values)");
    if (rc) return rc;
    Owned own;
    hipStream_t st = ctx().stream;
    rc = join_caller_stream(own, st, stream);
    if (rc) return rc;
    // the index arrays are checked on the device before the fill, the transpose or any gather reads them
    Scratch<unsigned> flag;
    rc = flag.alloc(1);
    if (rc) return rc;
    unsigned bad = 0;
    rc = launch_csc_validate(col_offsets, idx_type, width, nnz, row_indices, row_idx_type, height, flag, st);
    if (rc) return rc;
    SMK_HIP(hipMemcpyAsync(&bad, flag, sizeof(bad), hipMemcpyDeviceToHost, st));
    SMK_HIP(hipStreamSynchronize(st));
    if (bad) {
        set_error(std::string("smk_matrix_create_sparse_device:") + ((bad & 1) ? " col_offsets not monotone;" : "") +
                  ((bad & 2) ? " col_offsets do not run from 0 to nnz;" : "") + ((bad & 4) ? " row index out of range;" : "") +
                  ((bad & 8) ? " offset outside 32 bits;" : ""));
        return SMK_BAD_PARAM;
    }
    return matrix_create_sparse_device(out, height, width, nnz, [&](i64* colptr, unsigned* rowidx, double* val, hipStream_t fst) -> int {
        int frc = launch_csc_convert(col_offsets, idx_type, width, nnz, row_indices, row_idx_type, colptr, rowidx, fst);
        if (!frc) frc = launch_strided_convert(values, dtype, 1, nnz, val, DT_F64, 1, nnz, nnz, 1, fst);
        return frc;
    });
}

void smk_matrix_destroy(smk_matrix* a)
{
    if (!a) return;
    unregister_matrix(a);
    free_blocked_csc(&a->bA);
    free_blocked_csc(&a->bAt);
    free_seg_plan(&a->segA);
    free_seg_plan(&a->segAt);
    a->own.release();
    delete a;
}

// A copy of a resident matrix in the CALLING thread's context (its current device and stream): the second device of a
// two-device HierNMF2 run holds one (hierclust.cpp).  Device-to-device copies; works across devices and on one.
int smk_matrix_clone(const smk_matrix* src, smk_matrix** out)
{
    if (!src || !out) return SMK_BAD_PARAM;
    *out = nullptr;
    if (int rc = require_init()) return rc;
    smk_matrix* a = new_matrix(src->m, src->n_global, src->c0, src->n, src->storage, src->sparse, src->nnz);
    a->ascale = src->ascale; a->col_spread_log2 = src->col_spread_log2;
    a->colnorm_max = src->colnorm_max; a->rownorm_max = src->rownorm_max;
    a->ldA = src->ldA; a->colsA = src->colsA; a->ldAt = src->ldAt; a->colsAt = src->colsAt;
    a->single = src->single;
    bool ok = true;
    auto dup = [&](void** dst, const void* from, size_t bytes) {
        if (!ok || !from) return;
        if (a->own.dev((unsigned char**)dst, bytes) || hipMemcpy(*dst, from, bytes, hipMemcpyDefault) != hipSuccess) ok = false;
    };
    if (src->sparse) {
        dup((void**)&a->colptr, src->colptr, (size_t)(src->n + 1) * sizeof(i64));
        dup((void**)&a->colptr_t, src->colptr_t, (size_t)(src->m + 1) * sizeof(i64));
        dup((void**)&a->rowidx, src->rowidx, (size_t)src->nnz * sizeof(unsigned));
        dup((void**)&a->rowidx_t, src->rowidx_t, (size_t)src->nnz * sizeof(unsigned));
        dup((void**)&a->val, src->val, (size_t)src->nnz * sizeof(double));
        dup((void**)&a->val_t, src->val_t, (size_t)src->nnz * sizeof(double));
    } else {
        const size_t es = (size_t)elem_size(src->storage);
        dup(&a->A, src->A, (size_t)src->ldA * src->colsA * es);
        dup(&a->At, src->At, (size_t)src->ldAt * src->colsAt * es);
    }
    if (!ok) { set_error("smk_matrix_clone: device allocation or copy failed"); smk_matrix_destroy(a); return SMK_DEVICE_ERROR; }
    *out = a;
    return SMK_OK;
}

// read a resident sparse matrix (or the stored CSC of its transpose) back to the host (tests)
int smk_matrix_download_csc(const smk_matrix* a, int transposed, unsigned* col_offsets, unsigned* row_indices, double* data)
{
    if (!a || !a->sparse || !col_offsets) return SMK_BAD_PARAM;
    const i64 nc = transposed ? a->m : a->n;
    std::vector<i64> cp((size_t)nc + 1);
    SMK_HIP(hipStreamSynchronize(ctx().stream));
    SMK_HIP(hipMemcpy(cp.data(), transposed ? a->colptr_t : a->colptr, cp.size() * sizeof(i64), hipMemcpyDeviceToHost));
    for (i64 c = 0; c <= nc; ++c) col_offsets[c] = (unsigned)cp[(size_t)c];
    if (a->nnz > 0 && row_indices && data) {
        SMK_HIP(hipMemcpy(row_indices, transposed ? a->rowidx_t : a->rowidx, (size_t)a->nnz * sizeof(unsigned), hipMemcpyDeviceToHost));
        SMK_HIP(hipMemcpy(data, transposed ? a->val_t : a->val, (size_t)a->nnz * sizeof(double), hipMemcpyDeviceToHost));
    }
    return SMK_OK;
}

// The sparse Gemm of the reference by itself (common/include/sparse_gemm_ab_impl.hpp / sparse_gemm_ba_impl.hpp in gather
// form): out (k x ncols(B)) = X (k x rows(B)) * B with B = A (transposed == 0: W'A from X = W') or B = A' (transposed != 0:
// (AH')' from X = H), on the kernel the solver would take at rank k.  `reps` launches are timed with HIP events (avg_ms, may be NULL).
int smk_matrix_sparse_product(const smk_matrix* a, int transposed, int k, const double* X, int64_t ldx, double* out,
                              int64_t ldo, int reps, double* avg_ms)
{
    if (!a || !a->sparse || k < 1 || k > MAX_K || !X || !out || ldx < k || ldo < k) return SMK_BAD_PARAM;
    const i64 rows = transposed ? a->n : a->m, ncols = transposed ? a->m : a->n;
    const int KP = kp_of(k);
    const int kpp = (k <= 2) ? 2 : KP;
    const int ldx_dev = (k <= 2) ? 2 : KP;
    hipStream_t st = matrix_stream(a);
    if (k > 2 && !is_wide(k)) ensure_seg_plans(a);
    std::vector<double> xp((size_t)rows * ldx_dev, 0.0), pp((size_t)ncols * kpp);
    for (i64 r = 0; r < rows; ++r)
        for (int c = 0; c < k; ++c) xp[(size_t)r * ldx_dev + c] = X[r * ldx + c];
    Scratch<double> dX, dP;
    int rc = dX.alloc(xp.size());
    if (!rc) rc = dP.alloc(pp.size());
    if (rc) return rc;
    SMK_HIP(hipMemcpyAsync(dX, xp.data(), xp.size() * sizeof(double), hipMemcpyHostToDevice, st));
    const i64* cp = transposed ? a->colptr_t : a->colptr;
    const unsigned* ri = transposed ? a->rowidx_t : a->rowidx;
    const double* va = transposed ? a->val_t : a->val;
    const SegPlan& seg = transposed ? a->segAt : a->segA;
    auto once = [&]() -> int {
        if (k > 2 && !is_wide(k) && seg.rowflag && seg.ncols == ncols && !seg.uniform) return launch_spmm_seg(seg, cp, va, dX, k, dP, kpp, st);
        return launch_spmm_gather(cp, ri, va, ncols, a->nnz, dX, ldx_dev, k, dP, kpp, st);
    };
    rc = once();
    if (rc) return rc;
    if (reps > 0 && avg_ms) {
        Owned timer;                        // the two events of this measurement
        hipEvent_t e0, e1;
        if (timer.event(&e0, hipEventDefault) || timer.event(&e1, hipEventDefault)) return SMK_DEVICE_ERROR;
        SMK_HIP(hipEventRecord(e0, st));
        for (int i = 0; i < reps && !rc; ++i) rc = once();
        SMK_HIP(hipEventRecord(e1, st));
        SMK_HIP(hipEventSynchronize(e1));
        float ms = 0.f;
        (void)hipEventElapsedTime(&ms, e0, e1);
        *avg_ms = (double)ms / reps;
        if (rc) return rc;
    }
    SMK_HIP(hipMemcpyAsync(pp.data(), dP, pp.size() * sizeof(double), hipMemcpyDeviceToHost, st));
    SMK_HIP(hipStreamSynchronize(st));
    for (i64 j = 0; j < ncols; ++j)
        for (int c = 0; c < k; ++c) out[j * ldo + c] = pp[(size_t)j * kpp + c];
    return SMK_OK;
}
int64_t smk_matrix_nnz(const smk_matrix* a) { return a ? a->nnz : 0; }
int64_t smk_matrix_height(const smk_matrix* a) { return a ? a->m : 0; }

// the six arrays of CSC(A) and CSC(A') for a->n columns, a->m rows and a->nnz entries
static int alloc_csc(smk_matrix* a)
{
    return a->own.dev(&a->colptr, (size_t)a->n + 1) || a->own.dev(&a->colptr_t, (size_t)a->m + 1) || a->own.dev(&a->rowidx, (size_t)a->nnz) ||
           a->own.dev(&a->rowidx_t, (size_t)a->nnz) || a->own.dev(&a->val, (size_t)a->nnz) || a->own.dev(&a->val_t, (size_t)a->nnz);
}

// CSC shard (columns [col0, col0+ncols_local) of a height x width_global matrix) -> HBM, plus the
// CSC of its transpose built on the host by a counting sort (SparseMatrix::Transpose,
// sparse_matrix_ops.hpp:37-127).  Duplicate entries are kept (they add up in every product, as in
// the reference's Compress(), sparse_matrix_impl.hpp:184-260).
int smk_matrix_create_sparse(smk_matrix** out, int64_t height, int64_t width_global, int64_t col0,
                             int64_t ncols_local, int64_t nnz, const unsigned* col_offsets,
                             const unsigned* row_indices, const double* data)
{
    if (!out) return SMK_BAD_PARAM;
    *out = nullptr;
    if (int rc = require_init()) return rc;
    if (height <= 0 || width_global <= 0 || ncols_local <= 0 || col0 < 0 || col0 + ncols_local > width_global ||
        nnz < 0 || !col_offsets || (nnz > 0 && (!row_indices || !data)))
        return SMK_BAD_PARAM;
    if ((int64_t)col_offsets[ncols_local] - (int64_t)col_offsets[0] != nnz) { set_error("col_offsets do not span nnz"); return SMK_BAD_PARAM; }
    const unsigned base = col_offsets[0];
    std::vector<i64> cp((size_t)ncols_local + 1);
    for (int64_t c = 0; c <= ncols_local; ++c) {
        if (c > 0 && col_offsets[c] < col_offsets[c - 1]) { set_error("col_offsets not monotone"); return SMK_BAD_PARAM; }
        cp[(size_t)c] = (i64)col_offsets[c] - base;
    }
    for (int64_t p = 0; p < nnz; ++p)
        if ((int64_t)row_indices[base + p] >= height) { set_error("row index out of range"); return SMK_BAD_PARAM; }
    smk_matrix* a = new_matrix(height, width_global, col0, ncols_local, SMK_STORE_F32, true, nnz);
    if (alloc_csc(a)) { smk_matrix_destroy(a); return SMK_DEVICE_ERROR; }
    hipError_t e = hipMemcpy(a->colptr, cp.data(), cp.size() * sizeof(i64), hipMemcpyHostToDevice);
    if (e == hipSuccess && nnz > 0) e = hipMemcpy(a->rowidx, row_indices + base, (size_t)nnz * sizeof(unsigned), hipMemcpyHostToDevice);
    if (e == hipSuccess && nnz > 0) e = hipMemcpy(a->val, data + base, (size_t)nnz * sizeof(double), hipMemcpyHostToDevice);
    // the transpose: a stable radix sort by row on the device (sort.hip) -- the entry order of the host counting sort --
    // or, if that is not available (SMK_TRANSPOSE=host forces it), the host routine and a second upload
    const bool host_tr = sw::transpose_host();
    bool done = false;
    if (e == hipSuccess && !host_tr)
        done = device_csc_transpose(height, ncols_local, nnz, a->colptr, a->rowidx, a->val, a->colptr_t, a->rowidx_t, a->val_t, ctx().stream) == 0;
    if (e == hipSuccess && !done) {
        std::vector<unsigned> rit((size_t)(nnz > 0 ? nnz : 1)), cpt32((size_t)height + 1);
        std::vector<double> vt((size_t)(nnz > 0 ? nnz : 1));
        const int trc = smk_csc_transpose(height, ncols_local, col_offsets, row_indices, data, cpt32.data(), rit.data(), vt.data());
        if (trc != SMK_OK) { smk_matrix_destroy(a); return trc; }
        std::vector<i64> cpt((size_t)height + 1);
        for (int64_t r = 0; r <= height; ++r) cpt[(size_t)r] = cpt32[(size_t)r];
        e = hipMemcpy(a->colptr_t, cpt.data(), cpt.size() * sizeof(i64), hipMemcpyHostToDevice);
        if (e == hipSuccess && nnz > 0) e = hipMemcpy(a->rowidx_t, rit.data(), (size_t)nnz * sizeof(unsigned), hipMemcpyHostToDevice);
        if (e == hipSuccess && nnz > 0) e = hipMemcpy(a->val_t, vt.data(), (size_t)nnz * sizeof(double), hipMemcpyHostToDevice);
    }
    if (e != hipSuccess) {
        set_error(std::string("hipMemcpy(CSC): ") + hipGetErrorString(e));
        smk_matrix_destroy(a);
        return SMK_DEVICE_ERROR;
    }
    *out = a;
    return SMK_OK;
}

// preprocess.cpp: the resident matrix of a preprocessing result, filled on the device by `fill` (CSC with 64-bit offsets, on the
// context stream) and its transpose built as smk_matrix_create_sparse builds it -- the same matrix as one created from the
// downloaded arrays
extern "C++" {
namespace smk {
int matrix_create_sparse_device(smk_matrix** out, i64 height, i64 width, i64 nnz,
                                const std::function<int(i64* colptr, unsigned* rowidx, double* val, hipStream_t st)>& fill)
{
    if (!out) return SMK_BAD_PARAM;
    *out = nullptr;
    if (int rc = require_init()) return rc;
    if (height <= 0 || width <= 0 || nnz < 0) { set_error("empty matrix"); return SMK_BAD_PARAM; }
    smk_matrix* a = new_matrix(height, width, 0, width, SMK_STORE_F32, true, nnz);
    if (alloc_csc(a)) { smk_matrix_destroy(a); return SMK_DEVICE_ERROR; }
    if (fill(a->colptr, a->rowidx, a->val, ctx().stream) != 0 ||
        device_csc_transpose(height, width, nnz, a->colptr, a->rowidx, a->val, a->colptr_t, a->rowidx_t, a->val_t, ctx().stream) != 0) {
        smk_matrix_destroy(a);
        return SMK_DEVICE_ERROR;
    }
    const hipError_t e = hipStreamSynchronize(ctx().stream);
    if (e != hipSuccess) {
        set_error(std::string("resident CSC: ") + hipGetErrorString(e));
        smk_matrix_destroy(a);
        return SMK_DEVICE_ERROR;
    }
    *out = a;
    return SMK_OK;
}
}  // namespace smk
}  // extern "C++"

// host copy of a resident CSC (32-bit offsets), fetched on first use: only column subsets whose list is not strictly
// increasing are cut on the host
extern "C++" {
namespace smk {
int matrix_host_csc(const smk_matrix* a)
{
    if (!a->h_colptr.empty()) return SMK_OK;
    a->h_colptr.resize((size_t)a->n + 1);
    a->h_rowidx.resize((size_t)(a->nnz > 0 ? a->nnz : 1));
    a->h_val.resize((size_t)(a->nnz > 0 ? a->nnz : 1));
    const int rc = smk_matrix_download_csc(a, 0, a->h_colptr.data(), a->h_rowidx.data(), a->h_val.data());
    if (rc != SMK_OK) { a->h_colptr.clear(); return rc; }
    return SMK_OK;
}
}  // namespace smk
}  // extern "C++"

// Column subset of a resident matrix as a new matrix (HierNMF2 node, SubMatrixColsCompact).
// Dense (dense_matrix_impl.hpp:224-281): all rows kept, columns gathered HBM -> HBM, transpose rebuilt
// on the device.  Sparse (sparse_matrix_impl.hpp:479-590): rows without a stored entry in the selected
// columns are dropped; the cut is made on the host copy of the CSC and uploaded.
int smk_matrix_gather_cols(const smk_matrix* src, const unsigned* cols, int64_t ncols, smk_matrix** out,
                           unsigned* new_to_old_rows, int64_t* new_height)
{
    if (!out) return SMK_BAD_PARAM;
    *out = nullptr;
    if (!src || !cols || ncols <= 0) { set_error("SubMatrixColsCompact: empty column set"); return SMK_BAD_PARAM; }
    for (int64_t j = 0; j < ncols; ++j)
        if ((i64)cols[j] >= src->n) { set_error("SubMatrixColsCompact: column index out of range"); return SMK_BAD_PARAM; }
    if (!src->sparse) {
        smk_matrix* a = nullptr;
        int rc = smk_matrix_create(&a, src->m, ncols, 0, ncols, src->storage);
        if (rc) return rc;
        Scratch<unsigned> dcols;
        rc = dcols.alloc((size_t)ncols);
        if (rc) { smk_matrix_destroy(a); return rc; }
        const i64 es = elem_size(src->storage);
        hipError_t e = hipMemcpyAsync(dcols, cols, (size_t)ncols * sizeof(unsigned), hipMemcpyHostToDevice, ctx().stream);
        if (e == hipSuccess) {
            rc = launch_gather_cols(src->A, src->ldA * es, dcols, ncols, a->A, a->ldA * es, src->ldA * es, ctx().stream);
            if (!rc) rc = matrix_make_transpose(a);
            if (!rc) e = hipStreamSynchronize(ctx().stream);
        }
        if (e != hipSuccess) { set_error(std::string("gather_cols: ") + hipGetErrorString(e)); rc = SMK_DEVICE_ERROR; }
        if (rc) { smk_matrix_destroy(a); return rc; }
        if (new_to_old_rows) for (i64 r = 0; r < src->m; ++r) new_to_old_rows[r] = (unsigned)r;
        if (new_height) *new_height = src->m;
        *out = a;
        return SMK_OK;
    }
    // strictly increasing column lists (every HierNMF2 document list): cut on the device, nothing but
    // the row map crosses PCIe (sparse_subset.hip).  SMK_SPARSE_SUBSET=host forces the host cut below.
    bool increasing = true;
    for (int64_t j = 1; j < ncols && increasing; ++j) increasing = cols[j] > cols[j - 1];
    const bool force_host = sw::sparse_subset_host();
    if (increasing && !force_host) {
        SparseDev sd, od;
        sd.m = src->m; sd.n = src->n; sd.nnz = src->nnz;
        sd.colptr = src->colptr; sd.rowidx = src->rowidx; sd.val = src->val;
        sd.colptr_t = src->colptr_t; sd.rowidx_t = src->rowidx_t; sd.val_t = src->val_t;
        std::vector<unsigned> n2o_tmp;
        unsigned* n2o = new_to_old_rows;
        if (!n2o) { n2o_tmp.resize((size_t)src->m); n2o = n2o_tmp.data(); }
        const int rc = device_sparse_subset(sd, cols, ncols, &od, n2o, ctx().stream);
        if (rc) return rc == -3 ? SMK_BAD_PARAM : SMK_DEVICE_ERROR;
        smk_matrix* a = new_matrix(od.m, ncols, 0, ncols, SMK_STORE_F32, true, od.nnz);
        a->colptr = od.colptr; a->rowidx = od.rowidx; a->val = od.val;
        a->colptr_t = od.colptr_t; a->rowidx_t = od.rowidx_t; a->val_t = od.val_t;
        for (void* p : {(void*)od.colptr, (void*)od.rowidx, (void*)od.val, (void*)od.colptr_t, (void*)od.rowidx_t, (void*)od.val_t}) a->own.adopt(p);
        if (new_height) *new_height = od.m;
        *out = a;
        return SMK_OK;
    }
    int64_t nh = 0, nz = 0;
    int rc = matrix_host_csc(src);
    if (rc != SMK_OK) return rc;
    rc = smk_csc_subset_cols_compact(src->m, src->n, src->h_colptr.data(), src->h_rowidx.data(), src->h_val.data(), cols,
                                         ncols, nullptr, nullptr, nullptr, nullptr, nullptr, &nh, &nz);
    if (rc != SMK_OK) return rc;
    std::vector<unsigned> cp((size_t)ncols + 1), ri((size_t)nz);
    std::vector<double> va((size_t)nz);
    rc = smk_csc_subset_cols_compact(src->m, src->n, src->h_colptr.data(), src->h_rowidx.data(), src->h_val.data(), cols,
                                     ncols, cp.data(), ri.data(), va.data(), nullptr, new_to_old_rows, &nh, &nz);
    if (rc != SMK_OK) return rc;
    if (new_height) *new_height = nh;
    return smk_matrix_create_sparse(out, nh, ncols, 0, ncols, nz, cp.data(), ri.data(), va.data());
}

}  // extern "C"
