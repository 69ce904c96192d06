// smallk_amd/csrc/vocabulary.cpp -- a fitted vocabulary (surviving terms, their idf, the old -> new term map) and its
// application to the raw term counts of new documents (include/smallk_amd.h: smk_vocabulary_*).
//
// smk_vocabulary_apply and its device twin share one driver: the convert and row sort of preprocess_tf as they are, then the
// count pass, two scans and the fused fill-and-score pass of vocabulary.hip.  Two words come back to the host in between (the
// kept column and entry counts, which size the result).  The result is an ordinary smk_preprocess_result.
#include <chrono>
#include <mutex>
#include <string>
#include <vector>

#include "preprocess.h"
#include "preprocess_result.h"
#include "entry.h"
#include "vocabulary.h"

struct smk_vocabulary {
    unsigned height_in = 0, height = 0;
    int boolean_mode = 0;
    unsigned *term = nullptr, *old_to_new = nullptr;
    double* idf = nullptr;
    // pinned: the words an apply reads back (a column is unsorted; kept columns and entries).  One apply at a time uses them.
    unsigned* host = nullptr;
    mutable std::mutex host_mu;
    ~smk_vocabulary()
    {
        void* ptrs[] = {term, old_to_new, idf};
        for (void* p : ptrs)
            if (p) (void)smk::dev_free(p);
        if (host) (void)hipHostFree(host);
    }
};

namespace {

using smk::i64;
using smk::set_error;

double now_ms()
{
    using namespace std::chrono;
    return (double)duration_cast<nanoseconds>(steady_clock::now().time_since_epoch()).count() * 1e-6;
}

template <typename T>
int alloc(T** p, size_t count)
{
    *p = nullptr;
    SMK_HIP(smk::dev_malloc((void**)p, (count ? count : 1) * sizeof(T)));
    return 0;
}

#define VOC_TRY(expr)                                 \
    do {                                              \
        const int _rc = (expr);                       \
        if (_rc != 0) return SMK_DEVICE_ERROR;        \
    } while (0)

// the three arrays of a vocabulary from device sources (term, idf: `height` elements readable on st), and the scattered map
int build(smk_vocabulary* v, const unsigned* term, const double* idf, hipMemcpyKind kind, hipStream_t st)
{
    VOC_TRY(alloc(&v->term, v->height));
    VOC_TRY(alloc(&v->idf, v->height));
    VOC_TRY(alloc(&v->old_to_new, v->height_in));
    SMK_HIP(hipHostMalloc((void**)&v->host, 64));
    SMK_HIP(hipMemcpyAsync(v->term, term, (size_t)v->height * 4, kind, st));
    SMK_HIP(hipMemcpyAsync(v->idf, idf, (size_t)v->height * 8, kind, st));
    VOC_TRY(smk::voc_scatter(v->term, v->height, v->height_in, v->old_to_new, st));
    SMK_HIP(hipStreamSynchronize(st));
    return SMK_OK;
}

// the working set of one apply, allocated before the timers start (as a fit allocates its own) and freed with the call
struct Work {
    smk::Owned own;
    smk::PpScan scan;
    uint2* ent = nullptr;
    unsigned *unsorted = nullptr, *flag = nullptr, *len = nullptr, *cpos = nullptr, *dst = nullptr;
    int alloc(unsigned width, unsigned nnz)
    {
        VOC_TRY(own.dev(&ent, nnz));
        VOC_TRY(own.dev(&unsorted, 1));
        VOC_TRY(own.dev(&flag, (size_t)width + 1));
        VOC_TRY(own.dev(&len, (size_t)width + 1));
        VOC_TRY(own.dev(&cpos, (size_t)width + 1));
        VOC_TRY(own.dev(&dst, (size_t)width + 1));
        return 0;
    }
    ~Work() { scan.release(); }
};

// cp (offsets from 0), rows (< height_in) and data are device arrays that st may read; everything the result needs is written
// and complete on return.  t_up: when the input was on the device (the device phase is timed from there).
int apply(const smk_vocabulary& v, Work& w, unsigned min_terms, int boolean_mode, unsigned width, unsigned nnz, const unsigned* cp,
          const unsigned* rows, const double* data, hipStream_t st, double t_up, smk_preprocess_result* res)
{
    std::lock_guard<std::mutex> lock(v.host_mu);
    smk::PpScan& scan = w.scan;
    uint2* const ent = w.ent;
    unsigned *const unsorted = w.unsorted, *const flag = w.flag, *const len = w.len, *const cpos = w.cpos, *const dst = w.dst;
    unsigned* const host = v.host;
    res->height = v.height;
    res->height_in = v.height_in;
    res->boolean_mode = boolean_mode;

    // counts, and the row sort where a column needs it: preprocess_tf's own
    SMK_HIP(hipMemsetAsync(unsorted, 0, 4, st));
    VOC_TRY(smk::pp_convert(cp, rows, data, width, boolean_mode, ent, unsorted, st));
    SMK_HIP(hipMemcpyAsync(host, unsorted, 4, hipMemcpyDeviceToHost, st));
    SMK_HIP(hipStreamSynchronize(st));
    if (host[0]) VOC_TRY(smk::pp_sort_columns(cp, width, nnz, v.height_in, ent, st));

    VOC_TRY(smk::voc_count(cp, ent, width, v.old_to_new, min_terms, flag, len, st));
    VOC_TRY(scan.exclusive(flag, cpos, (i64)width + 1, st));
    VOC_TRY(scan.exclusive(len, dst, (i64)width + 1, st));
    SMK_HIP(hipMemcpyAsync(host, cpos + width, 4, hipMemcpyDeviceToHost, st));
    SMK_HIP(hipMemcpyAsync(host + 1, dst + width, 4, hipMemcpyDeviceToHost, st));
    SMK_HIP(hipStreamSynchronize(st));
    const unsigned new_width = host[0], new_nnz = host[1];
    if (new_width == 0) {
        // like a fit that lost every column: the sizes before the drop (the entries that survive the term filter)
        VOC_TRY(smk::voc_count(cp, ent, width, v.old_to_new, 0u, flag, len, st));
        VOC_TRY(scan.exclusive(len, dst, (i64)width + 1, st));
        SMK_HIP(hipMemcpyAsync(host, dst + width, 4, hipMemcpyDeviceToHost, st));
        SMK_HIP(hipStreamSynchronize(st));
        res->failed = true;
        res->width = width;
        res->nnz = host[0];
        res->device_ms = now_ms() - t_up;
        return SMK_FAILURE;
    }

    VOC_TRY(alloc(&res->cp, (size_t)new_width + 1));
    VOC_TRY(alloc(&res->doc, new_width));
    VOC_TRY(alloc(&res->ent, new_nnz));
    VOC_TRY(alloc(&res->score, new_nnz));
    VOC_TRY(alloc(&res->term, v.height));
    VOC_TRY(smk::voc_fill_score(cp, ent, width, v.old_to_new, v.idf, flag, cpos, dst, res->cp, res->ent, res->score, res->doc, st));
    SMK_HIP(hipMemcpyAsync(res->term, v.term, (size_t)v.height * 4, hipMemcpyDeviceToDevice, st));
    SMK_HIP(hipStreamSynchronize(st));
    res->width = new_width;
    res->nnz = new_nnz;
    res->device_ms = now_ms() - t_up;
    return SMK_OK;
}

// what both apply entries check first; *boolean_mode: the option, or the fit's value for -1
int apply_args(const char* who, const smk_vocabulary* v, const smk_apply_options* opts, unsigned width, smk_preprocess_result** out,
               int* boolean_mode)
{
    const std::string w(who);
    if (!out) { set_error(w + ": null output"); return SMK_BAD_PARAM; }
    *out = nullptr;
    if (int rc = smk::require_init()) return rc;
    if (!v) { set_error(w + ": null vocabulary"); return SMK_BAD_PARAM; }
    if (!opts) { set_error(w + ": null options"); return SMK_BAD_PARAM; }
    if (width == 0) { set_error(w + ": width 0"); return SMK_BAD_PARAM; }
    if (width > 0x7FFFFFFFu) { set_error(w + ": more than 2^31 - 1 columns"); return SMK_SIZE_TOO_LARGE; }
    if (opts->boolean_mode < -1) { set_error(w + ": boolean_mode is -1 (the fit's), 0 or 1"); return SMK_BAD_PARAM; }
    *boolean_mode = opts->boolean_mode == -1 ? v->boolean_mode : (opts->boolean_mode != 0);
    return SMK_OK;
}

int hand_over(int rc, smk_preprocess_result* res, smk_preprocess_result** out)
{
    if (rc == SMK_OK || rc == SMK_FAILURE) *out = res;
    else delete res;
    return rc;
}

}  // namespace

extern "C" {

int smk_preprocess_result_vocabulary(const smk_preprocess_result* r, smk_vocabulary** out)
{
    if (!out) return SMK_BAD_PARAM;
    *out = nullptr;
    if (!r) return SMK_BAD_PARAM;
    if (r->failed) { set_error("preprocess: every column was pruned"); return SMK_FAILURE; }
    if (!r->idf || !r->term || r->height == 0) {
        set_error("smk_preprocess_result_vocabulary: not the result of a fit (an applied result keeps no idf: use the vocabulary that made it)");
        return SMK_FAILURE;
    }
    smk_vocabulary* v = new smk_vocabulary;
    v->height_in = r->height_in;
    v->height = r->height;
    v->boolean_mode = r->boolean_mode;
    const int rc = build(v, r->term, r->idf, hipMemcpyDeviceToDevice, smk::context_stream(nullptr));
    if (rc) { delete v; return rc; }
    *out = v;
    return SMK_OK;
}

int smk_vocabulary_create(unsigned height_in, unsigned height, const unsigned* term_indices, const double* idf, int boolean_mode,
                          smk_vocabulary** out)
{
    if (!out) { set_error("smk_vocabulary_create: null output"); return SMK_BAD_PARAM; }
    *out = nullptr;
    if (int rc = smk::require_init()) return rc;
    if (!term_indices || !idf) { set_error("smk_vocabulary_create: null array"); return SMK_BAD_PARAM; }
    if (height < 1) { set_error("smk_vocabulary_create: height < 1"); return SMK_BAD_PARAM; }
    for (unsigned i = 0; i < height; ++i) {
        if (term_indices[i] >= height_in) { set_error("smk_vocabulary_create: term index not below height_in"); return SMK_BAD_PARAM; }
        if (i > 0 && term_indices[i] <= term_indices[i - 1]) { set_error("smk_vocabulary_create: term_indices not strictly ascending"); return SMK_BAD_PARAM; }
    }
    smk_vocabulary* v = new smk_vocabulary;
    v->height_in = height_in;
    v->height = height;
    v->boolean_mode = boolean_mode != 0;
    const int rc = build(v, term_indices, idf, hipMemcpyHostToDevice, smk::ctx().stream);
    if (rc) { delete v; return rc; }
    *out = v;
    return SMK_OK;
}

void smk_vocabulary_destroy(smk_vocabulary* v) { delete v; }

int smk_vocabulary_sizes(const smk_vocabulary* v, unsigned* height_in, unsigned* height, int* boolean_mode)
{
    if (!v) return SMK_BAD_PARAM;
    if (height_in) *height_in = v->height_in;
    if (height) *height = v->height;
    if (boolean_mode) *boolean_mode = v->boolean_mode;
    return SMK_OK;
}

int smk_vocabulary_download(const smk_vocabulary* v, unsigned* term_indices, double* idf)
{
    if (!v) return SMK_BAD_PARAM;
    const hipStream_t st = smk::context_stream(nullptr);
    if (term_indices) SMK_HIP(hipMemcpyAsync(term_indices, v->term, (size_t)v->height * 4, hipMemcpyDeviceToHost, st));
    if (idf) SMK_HIP(hipMemcpyAsync(idf, v->idf, (size_t)v->height * 8, hipMemcpyDeviceToHost, st));
    SMK_HIP(hipStreamSynchronize(st));
    return SMK_OK;
}

int smk_vocabulary_apply(const smk_vocabulary* v, const smk_apply_options* opts, unsigned width, unsigned nnz, const unsigned* col_offsets,
                         const unsigned* row_indices, const double* data, smk_preprocess_result** out)
{
    int boolean_mode = 0;
    int rc = apply_args("smk_vocabulary_apply", v, opts, width, out, &boolean_mode);
    if (rc) return rc;
    // the input, checked as smk_preprocess checks its own
    if (!col_offsets || (nnz > 0 && (!row_indices || !data))) { set_error("smk_vocabulary_apply: null array"); return SMK_BAD_PARAM; }
    if ((int64_t)col_offsets[width] - (int64_t)col_offsets[0] != (int64_t)nnz) { set_error("col_offsets do not span nnz"); return SMK_BAD_PARAM; }
    if (nnz > 0x7FFFFFFFu) { set_error("smk_vocabulary_apply: more than 2^31 - 1 entries"); return SMK_SIZE_TOO_LARGE; }
    for (unsigned c = 1; c <= width; ++c)                                // width < 2^31 (apply_args): c does not wrap
        if (col_offsets[c] < col_offsets[c - 1]) { set_error("col_offsets not monotone"); return SMK_BAD_PARAM; }
    const unsigned base = col_offsets[0];
    for (unsigned p = 0; p < nnz; ++p)
        if (row_indices[(size_t)base + p] >= v->height_in) { set_error("row index out of range"); return SMK_BAD_PARAM; }
    std::vector<unsigned> cp_host((size_t)width + 1);
    for (size_t c = 0; c <= width; ++c) cp_host[c] = col_offsets[c] - base;

    const hipStream_t st = smk::ctx().stream;
    smk::Scratch<unsigned> d_cp, d_rows;
    smk::Scratch<double> d_data;
    VOC_TRY(d_cp.alloc((size_t)width + 1));
    VOC_TRY(d_rows.alloc(nnz));
    VOC_TRY(d_data.alloc(nnz));
    Work work;
    VOC_TRY(work.alloc(width, nnz));
    smk_preprocess_result* res = new smk_preprocess_result;
    auto upload = [&]() -> int {
        const double t0 = now_ms();
        SMK_HIP(hipMemcpyAsync(d_cp, cp_host.data(), ((size_t)width + 1) * 4, hipMemcpyHostToDevice, st));
        if (nnz > 0) {
            SMK_HIP(hipMemcpyAsync(d_rows, row_indices + base, (size_t)nnz * 4, hipMemcpyHostToDevice, st));
            SMK_HIP(hipMemcpyAsync(d_data, data + base, (size_t)nnz * 8, hipMemcpyHostToDevice, st));
        }
        SMK_HIP(hipStreamSynchronize(st));
        res->upload_ms = now_ms() - t0;
        return 0;
    };
    rc = upload();
    if (!rc) rc = apply(*v, work, opts->min_terms, boolean_mode, width, nnz, d_cp, d_rows, d_data, st, now_ms(), res);
    return hand_over(rc, res, out);
}

int smk_vocabulary_apply_device(const smk_vocabulary* v, const smk_apply_options* opts, unsigned width, unsigned nnz, const void* col_offsets,
                                int idx_type, const void* row_indices, int row_idx_type, const void* values, int dtype, void* stream,
                                smk_preprocess_result** out)
{
    int boolean_mode = 0;
    int rc = apply_args("smk_vocabulary_apply_device", v, opts, width, out, &boolean_mode);
    if (rc) return rc;
    if ((idx_type != SMK_IDX_I32 && idx_type != SMK_IDX_I64) || (row_idx_type != SMK_IDX_I32 && row_idx_type != SMK_IDX_I64)) {
        set_error("smk_vocabulary_apply_device: unknown index type");
        return SMK_BAD_PARAM;
    }
    if (!smk::is_factor_dtype(dtype)) { set_error("smk_vocabulary_apply_device: values are fp64 or fp32"); return SMK_BAD_PARAM; }
    if (nnz > 0x7FFFFFFFu) { set_error("smk_vocabulary_apply_device: more than 2^31 - 1 entries"); return SMK_SIZE_TOO_LARGE; }
    // the three arrays as views of 8- / 4-byte elements: same pointer and extent checks as a dense view
    const auto idx_dt = [](int t) { return t == SMK_IDX_I64 ? (int)smk::DT_F64 : (int)smk::DT_F32; };
    rc = smk::check_device_view(col_offsets, idx_dt(idx_type), (i64)width + 1, 1, 1, (i64)width + 1, false, "smk_vocabulary_apply_device(col_offsets)");
    if (!rc && nnz > 0) rc = smk::check_device_view(row_indices, idx_dt(row_idx_type), nnz, 1, 1, nnz, false, "smk_vocabulary_apply_device(row_indices)");
    if (!rc && nnz > 0) rc = smk::check_device_view(values, dtype, nnz, 1, 1, nnz, false, "smk_vocabulary_apply_device(values)");
    if (rc) return rc;
    // everything the call allocates comes first, then the caller's stream is joined and the clock starts
    smk::Scratch<unsigned> flag, d_cp, d_rows;
    smk::Scratch<double> d_data;
    Work work;
    VOC_TRY(flag.alloc(1));
    VOC_TRY(work.alloc(width, nnz));
    if (idx_type == SMK_IDX_I64) VOC_TRY(d_cp.alloc((size_t)width + 1));
    if (row_idx_type == SMK_IDX_I64 && nnz > 0) VOC_TRY(d_rows.alloc(nnz));
    if (dtype != SMK_DT_F64 && nnz > 0) VOC_TRY(d_data.alloc(nnz));
    smk::Owned own;
    const hipStream_t st = smk::ctx().stream;
    rc = smk::join_caller_stream(own, st, stream);
    if (rc) return rc;
    const double t0 = now_ms();
    // the index arrays are checked on the device before the convert or any gather reads through them
    unsigned bad = 0;
    VOC_TRY(smk::launch_csc_validate(col_offsets, idx_type, width, nnz, row_indices, row_idx_type, v->height_in, flag, st));
    SMK_HIP(hipMemcpyAsync(&bad, flag, sizeof(bad), hipMemcpyDeviceToHost, st));
    SMK_HIP(hipStreamSynchronize(st));
    if (bad) {
        set_error(std::string("smk_vocabulary_apply_device:") + ((bad & 1) ? " col_offsets not monotone;" : "") +
                  ((bad & 2) ? " col_offsets do not run from 0 to nnz;" : "") + ((bad & 4) ? " row index out of range;" : "") +
                  ((bad & 8) ? " offset outside 32 bits;" : ""));
        return SMK_BAD_PARAM;
    }
    // checked 32-bit indices and fp64 values are read where they are; the other types through a copy in the working types
    const unsigned* cp = (const unsigned*)col_offsets;
    const unsigned* rows = (const unsigned*)row_indices;
    const double* data = (const double*)values;
    if (idx_type == SMK_IDX_I64) {
        VOC_TRY(smk::voc_narrow_i64((const long long*)col_offsets, (i64)width + 1, d_cp, st));
        cp = d_cp;
    }
    if (row_idx_type == SMK_IDX_I64 && nnz > 0) {
        VOC_TRY(smk::voc_narrow_i64((const long long*)row_indices, nnz, d_rows, st));
        rows = d_rows;
    }
    if (dtype != SMK_DT_F64 && nnz > 0) {
        VOC_TRY(smk::launch_strided_convert(values, dtype, 1, nnz, d_data, smk::DT_F64, 1, nnz, nnz, 1, st));
        data = d_data;
    }
    smk_preprocess_result* res = new smk_preprocess_result;
    rc = apply(*v, work, opts->min_terms, boolean_mode, width, nnz, cp, rows, data, st, t0, res);
    return hand_over(rc, res, out);
}

}  // extern "C"
