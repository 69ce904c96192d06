// smallk_amd/csrc/preprocess.cpp -- preprocess_tf (preprocessor/src/preprocess.cpp:81-232) on the device: the host loop
// over the passes of preprocess.hip, the C ABI of include/smallk_amd.h and the reduced_matrix.mtx writer.
//
// Per iteration only the scalars the loop branches on come back to the host (new height, new width after the length
// test, new width after the duplicate check, the entry count for the log line).  smk_preprocess waits for its last pass, so
// a result's arrays are complete when it returns; the accessors work on the calling thread's current context stream.
#include <sched.h>

#include <chrono>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <thread>
#include <vector>

#include "../../include/smallk_amd.h"
#include "common.h"
#include "entry.h"
#include "owned.h"
#include "preprocess.h"
#include "preprocess_result.h"

namespace {

using smk::i64;

double now_ms()
{
    using namespace std::chrono;
    return (double)duration_cast<nanoseconds>(steady_clock::now().time_since_epoch()).count() * 1e-6;
}

struct Work {
    hipStream_t st = nullptr;
    unsigned *cp[2] = {}, *term[2] = {}, *doc[2] = {};
    unsigned long long* stat[2] = {};                // tot << 32 | df per row
    uint2* ent[2] = {};
    unsigned *rflag = nullptr, *rpos = nullptr, *cflag = nullptr, *cpos = nullptr, *len = nullptr, *dst = nullptr;
    unsigned long long *hash = nullptr, *hash_sorted = nullptr;
    unsigned *idx = nullptr, *idx_sorted = nullptr, *differ = nullptr;
    unsigned* host = nullptr;                        // pinned: the scalars the loop reads
    smk::PpScan scan;
    int a = 0;                                       // which half of each ping-pong pair is current
    ~Work()
    {
        for (int h = 0; h < 2; ++h) {
            void* ptrs[] = {cp[h], stat[h], term[h], doc[h], ent[h]};
            for (void* p : ptrs)
                if (p) (void)smk::dev_free(p);
        }
        void* ptrs[] = {rflag, rpos, cflag, cpos, len, dst, hash, hash_sorted, idx, idx_sorted, differ};
        for (void* p : ptrs)
            if (p) (void)smk::dev_free(p);
        if (host) (void)hipHostFree(host);
        scan.release();
    }
};

#define PP_TRY(expr)                                  \
    do {                                              \
        const int _rc = (expr);                       \
        if (_rc != 0) return SMK_DEVICE_ERROR;        \
    } while (0)
#define PP_HIP(expr)                                                                         \
    do {                                                                                     \
        hipError_t _e = (expr);                                                              \
        if (_e != hipSuccess) {                                                              \
            smk::set_error(std::string("preprocess: ") + #expr + ": " + hipGetErrorString(_e)); \
            return SMK_DEVICE_ERROR;                                                         \
        }                                                                                    \
    } while (0)

template <typename T>
int alloc(T** p, size_t count)
{
    *p = nullptr;
    PP_HIP(smk::dev_malloc((void**)p, (count ? count : 1) * sizeof(T)));
    return 0;
}

// read `count` words of device memory into w.host[slot..] and wait
int fetch(Work& w, int slot, const unsigned* dev, int count)
{
    PP_HIP(hipMemcpyAsync(w.host + slot, dev, (size_t)count * 4, hipMemcpyDeviceToHost, w.st));
    PP_HIP(hipStreamSynchronize(w.st));
    return 0;
}

// drop the columns with cflag[c] == 0 (cpos = exclusive scan of cflag, new_width = cpos[width]); returns the new entry count
int drop_columns(Work& w, unsigned width, unsigned new_width, unsigned* nnz)
{
    const int a = w.a, b = 1 - w.a;
    PP_TRY(smk::pp_col_kept_len(w.cp[a], width, w.cflag, w.len, w.st));
    PP_TRY(w.scan.exclusive(w.len, w.dst, (i64)width + 1, w.st));
    PP_TRY(smk::pp_col_drop_stats(w.cp[a], w.ent[a], width, w.cflag, w.stat[a], w.st));
    PP_TRY(smk::pp_col_copy(w.cp[a], w.ent[a], width, w.cflag, w.cpos, w.dst, w.doc[a], w.cp[b], w.ent[b], w.doc[b], w.st));
    // the new offsets, entries and doc indices take the current half; statistics and term indices stay where they are
    std::swap(w.cp[a], w.cp[b]);
    std::swap(w.ent[a], w.ent[b]);
    std::swap(w.doc[a], w.doc[b]);
    PP_TRY(fetch(w, 0, w.cp[a] + new_width, 1));
    *nnz = w.host[0];
    return 0;
}

// UniqueCols (preprocess.cpp:631-724): cflag = 1 for the columns that survive, cpos its scan; returns the surviving count
int unique_columns(Work& w, unsigned width, unsigned* new_width)
{
    const int a = w.a;
    PP_TRY(smk::pp_hash(w.cp[a], w.ent[a], width, w.hash, w.idx, w.st));
    PP_TRY(w.scan.sort_pairs(w.hash, w.hash_sorted, w.idx, w.idx_sorted, width, w.st));
    PP_TRY(smk::pp_dup_resolve(w.cp[a], w.ent[a], w.hash_sorted, w.idx_sorted, width, w.cflag, w.differ, w.st));
    PP_TRY(w.scan.exclusive(w.cflag, w.cpos, (i64)width + 1, w.st));
    PP_TRY(fetch(w, 0, w.cpos + width, 1));
    *new_width = w.host[0];
    return 0;
}

int run(const smk_preprocess_options& o, unsigned height, unsigned width, unsigned nnz, const unsigned* col_offsets,
        const unsigned* row_indices, const double* data, hipStream_t st, smk_preprocess_result* res)
{
    Work w;
    w.st = st;
    res->height_in = height;
    res->boolean_mode = o.boolean_mode;
    const unsigned base = col_offsets[0];
    std::vector<unsigned> cp_host((size_t)width + 1);
    for (size_t c = 0; c <= width; ++c) cp_host[c] = col_offsets[c] - base;

    smk::Scratch<unsigned> d_rows, d_unsorted;          // the input as uploaded: gone when this function returns
    smk::Scratch<double> d_data;
    for (int h = 0; h < 2; ++h) {
        PP_TRY(alloc(&w.cp[h], (size_t)width + 1));
        PP_TRY(alloc(&w.ent[h], nnz));
        PP_TRY(alloc(&w.stat[h], (size_t)height + 1));
        PP_TRY(alloc(&w.term[h], (size_t)height + 1));
        PP_TRY(alloc(&w.doc[h], (size_t)width + 1));
    }
    PP_TRY(alloc(&w.rflag, (size_t)height + 1));
    PP_TRY(alloc(&w.rpos, (size_t)height + 1));
    PP_TRY(alloc(&w.cflag, (size_t)width + 1));
    PP_TRY(alloc(&w.cpos, (size_t)width + 1));
    PP_TRY(alloc(&w.len, (size_t)width + 1));
    PP_TRY(alloc(&w.dst, (size_t)width + 1));
    PP_TRY(alloc(&w.hash, width));
    PP_TRY(alloc(&w.hash_sorted, width));
    PP_TRY(alloc(&w.idx, width));
    PP_TRY(alloc(&w.idx_sorted, width));
    PP_TRY(alloc(&w.differ, (size_t)width + 1));
    PP_TRY(alloc(d_rows.put(), nnz));
    PP_TRY(alloc(d_data.put(), nnz));
    PP_TRY(alloc(d_unsorted.put(), 1));
    PP_HIP(hipHostMalloc((void**)&w.host, 64));

    // the input upload: the copies alone (the working set above is allocated before the timer starts)
    const double t0 = now_ms();
    PP_HIP(hipMemcpyAsync(w.cp[0], cp_host.data(), ((size_t)width + 1) * 4, hipMemcpyHostToDevice, w.st));
    if (nnz > 0) {
        PP_HIP(hipMemcpyAsync(d_rows, row_indices + base, (size_t)nnz * 4, hipMemcpyHostToDevice, w.st));
        PP_HIP(hipMemcpyAsync(d_data, data + base, (size_t)nnz * 8, hipMemcpyHostToDevice, w.st));
    }
    PP_HIP(hipStreamSynchronize(w.st));
    const double t1 = now_ms();
    res->upload_ms = t1 - t0;

    // counts, the row sort where a column needs it, identity index sets, the row statistics
    PP_HIP(hipMemsetAsync(d_unsorted, 0, 4, w.st));
    PP_TRY(smk::pp_convert(w.cp[0], d_rows, d_data, width, o.boolean_mode, w.ent[0], d_unsorted, w.st));
    PP_TRY(fetch(w, 0, d_unsorted, 1));
    if (w.host[0]) PP_TRY(smk::pp_sort_columns(w.cp[0], width, nnz, height, w.ent[0], w.st));
    PP_TRY(smk::pp_iota(w.term[0], height, w.st));
    PP_TRY(smk::pp_iota(w.doc[0], width, w.st));
    PP_HIP(hipMemsetAsync(w.stat[0], 0, ((size_t)height + 1) * 8, w.st));
    PP_TRY(smk::pp_row_stats(w.ent[0], nnz, w.stat[0], w.st));

    unsigned iter = 0;
    while (iter < o.max_iter) {
        // PruneRows
        {
            const int a = w.a, b = 1 - w.a;
            PP_TRY(smk::pp_row_keep(w.stat[a], height, o.docs_per_term, width, w.rflag, w.st));
            PP_TRY(w.scan.exclusive(w.rflag, w.rpos, (i64)height + 1, w.st));
            PP_TRY(fetch(w, 0, w.rpos + height, 1));
            const unsigned new_height = w.host[0];
            if (new_height != height) {
                PP_TRY(smk::pp_row_gather(w.rflag, w.rpos, height, w.stat[a], w.term[a], w.stat[b], w.term[b], w.st));
                PP_TRY(smk::pp_col_count_rows(w.cp[a], w.ent[a], width, w.rflag, w.len, w.st));
                PP_TRY(w.scan.exclusive(w.len, w.cp[b], (i64)width + 1, w.st));
                PP_TRY(smk::pp_col_fill_rows(w.cp[a], w.ent[a], width, w.rflag, w.rpos, w.cp[b], w.ent[b], w.st));
                // the doc indices do not move
                std::swap(w.doc[a], w.doc[b]);
                w.a = b;
                height = new_height;
            }
        }
        // PrunableCols
        PP_TRY(smk::pp_col_keep_len(w.cp[w.a], width, o.terms_per_doc, w.cflag, w.st));
        PP_TRY(w.scan.exclusive(w.cflag, w.cpos, (i64)width + 1, w.st));
        PP_TRY(fetch(w, 0, w.cpos + width, 1));
        unsigned new_width = w.host[0];
        if (new_width == width) {
            PP_TRY(unique_columns(w, width, &new_width));
            if (new_width == width) break;
        } else {
            if (new_width == 0) {
                PP_TRY(fetch(w, 0, w.cp[w.a] + width, 1));
                res->failed = true;
                res->height = height; res->width = width; res->nnz = w.host[0]; res->iterations = iter;
                res->device_ms = now_ms() - t1;
                return SMK_FAILURE;
            }
            PP_TRY(drop_columns(w, width, new_width, &nnz));
            width = new_width;
            PP_TRY(unique_columns(w, width, &new_width));
        }
        if (new_width != width) {
            PP_TRY(drop_columns(w, width, new_width, &nnz));
            width = new_width;
        }
        PP_TRY(fetch(w, 0, w.cp[w.a] + width, 1));
        nnz = w.host[0];
        res->log.push_back(height);
        res->log.push_back(width);
        res->log.push_back(nnz);
        ++iter;
    }
    PP_TRY(fetch(w, 0, w.cp[w.a] + width, 1));
    nnz = w.host[0];

    // scores on the final matrix; the result takes the current halves and keeps the idf (smk_preprocess_result_vocabulary)
    PP_TRY(alloc(&res->idf, (size_t)height + 1));
    PP_TRY(alloc(&res->score, nnz));
    const int rc_sc = smk::pp_scores(w.cp[w.a], w.ent[w.a], width, w.stat[w.a], height, res->idf, res->score, w.st);
    const hipError_t e = hipStreamSynchronize(w.st);
    if (rc_sc) return SMK_DEVICE_ERROR;
    if (e != hipSuccess) { smk::set_error(std::string("preprocess scores: ") + hipGetErrorString(e)); return SMK_DEVICE_ERROR; }
    res->device_ms = now_ms() - t1;

    const int a = w.a;
    res->cp = w.cp[a]; w.cp[a] = nullptr;
    res->ent = w.ent[a]; w.ent[a] = nullptr;
    res->term = w.term[a]; w.term[a] = nullptr;
    res->doc = w.doc[a]; w.doc[a] = nullptr;
    res->height = height; res->width = width; res->nnz = nnz; res->iterations = iter;
    return SMK_OK;
}

// threads of the .mtx writer: the hardware threads this process may run on (its CPU affinity), at most OMP_NUM_THREADS when
// that is set
int writer_threads()
{
    int n = (int)std::thread::hardware_concurrency();
    cpu_set_t set;
    if (sched_getaffinity(0, sizeof set, &set) == 0 && CPU_COUNT(&set) > 0) n = n > 0 ? std::min(n, CPU_COUNT(&set)) : CPU_COUNT(&set);
    if (const char* e = getenv("OMP_NUM_THREADS"))
        if (atoi(e) > 0) n = n > 0 ? std::min(n, atoi(e)) : atoi(e);
    return n > 0 ? n : 2;
}

}  // namespace

extern "C" {

int smk_preprocess(const smk_preprocess_options* opts, unsigned height, unsigned width, unsigned nnz, const unsigned* col_offsets,
                   const unsigned* row_indices, const double* data, smk_preprocess_result** out)
{
    if (!out) return SMK_BAD_PARAM;
    *out = nullptr;
    if (int rc = smk::require_init()) return rc;
    hipStream_t st = smk::context_stream(nullptr);
    if (!opts || height == 0 || width == 0 || !col_offsets || (nnz > 0 && (!row_indices || !data))) return SMK_BAD_PARAM;
    if ((int64_t)col_offsets[width] - (int64_t)col_offsets[0] != (int64_t)nnz) { smk::set_error("col_offsets do not span nnz"); return SMK_BAD_PARAM; }
    if (nnz > 0x7FFFFFFFu) { smk::set_error("preprocess: more than 2^31 - 1 entries"); return SMK_SIZE_TOO_LARGE; }
    for (unsigned c = 1; c <= width; ++c)
        if (col_offsets[c] < col_offsets[c - 1]) { smk::set_error("col_offsets not monotone"); return SMK_BAD_PARAM; }
    const unsigned base = col_offsets[0];
    for (unsigned p = 0; p < nnz; ++p)
        if (row_indices[base + p] >= height) { smk::set_error("row index out of range"); return SMK_BAD_PARAM; }
    smk_preprocess_result* res = new smk_preprocess_result;
    const int rc = run(*opts, height, width, nnz, col_offsets, row_indices, data, st, res);
    if (rc == SMK_OK || rc == SMK_FAILURE) {
        *out = res;
        return rc;
    }
    delete res;
    return rc;
}

void smk_preprocess_result_destroy(smk_preprocess_result* r) { delete r; }

int smk_preprocess_result_sizes(const smk_preprocess_result* r, unsigned* height, unsigned* width, unsigned* nnz, unsigned* iterations)
{
    if (!r) return SMK_BAD_PARAM;
    if (height) *height = r->height;
    if (width) *width = r->width;
    if (nnz) *nnz = r->nnz;
    if (iterations) *iterations = r->iterations;
    return SMK_OK;
}

int smk_preprocess_result_log(const smk_preprocess_result* r, unsigned* out)
{
    if (!r || !out) return SMK_BAD_PARAM;
    std::copy(r->log.begin(), r->log.end(), out);
    return SMK_OK;
}

int smk_preprocess_result_timing(const smk_preprocess_result* r, double* upload_ms, double* device_ms)
{
    if (!r) return SMK_BAD_PARAM;
    if (upload_ms) *upload_ms = r->upload_ms;
    if (device_ms) *device_ms = r->device_ms;
    return SMK_OK;
}

int smk_preprocess_result_download(const smk_preprocess_result* r, unsigned* term_indices, unsigned* doc_indices, unsigned* col_offsets,
                                   unsigned* row_indices, double* scores)
{
    if (!r) return SMK_BAD_PARAM;
    if (r->failed) { smk::set_error("preprocess: every column was pruned"); return SMK_FAILURE; }
    const hipStream_t st = smk::context_stream(nullptr);
    smk::Scratch<unsigned> rows;
    if (row_indices && r->nnz > 0) {
        if (smk::dev_malloc(rows.put(), (size_t)r->nnz * 4) != hipSuccess) { smk::set_error("preprocess: hipMalloc"); return SMK_DEVICE_ERROR; }
        if (smk::pp_export(r->cp, r->width, r->ent, r->nnz, nullptr, rows, st)) return SMK_DEVICE_ERROR;
    }
    hipError_t e = hipSuccess;
    auto D2H = [&](void* dst, const void* src, size_t bytes) {
        if (e == hipSuccess && dst && bytes) e = hipMemcpyAsync(dst, src, bytes, hipMemcpyDeviceToHost, st);
    };
    D2H(term_indices, r->term, (size_t)r->height * 4);
    D2H(doc_indices, r->doc, (size_t)r->width * 4);
    D2H(col_offsets, r->cp, ((size_t)r->width + 1) * 4);
    D2H(row_indices, rows, (size_t)r->nnz * 4);
    D2H(scores, r->score, (size_t)r->nnz * 8);
    if (e == hipSuccess) e = hipStreamSynchronize(st);
    if (e != hipSuccess) { smk::set_error(std::string("preprocess download: ") + hipGetErrorString(e)); return SMK_DEVICE_ERROR; }
    return SMK_OK;
}

int smk_preprocess_result_matrix(const smk_preprocess_result* r, smk_matrix** out)
{
    if (!out) return SMK_BAD_PARAM;
    *out = nullptr;
    if (!r) return SMK_BAD_PARAM;
    if (r->failed) { smk::set_error("preprocess: every column was pruned"); return SMK_FAILURE; }
    // the offsets and row indices are written straight into the new matrix, the scores copied beside them; all on the stream
    // of the matrix's context, which also builds the transpose
    auto fill = [r](smk::i64* colptr, unsigned* rowidx, double* val, hipStream_t st) {
        if (smk::pp_export(r->cp, r->width, r->ent, r->nnz, colptr, rowidx, st)) return -1;
        if (r->nnz > 0 && hipMemcpyAsync(val, r->score, (size_t)r->nnz * 8, hipMemcpyDeviceToDevice, st) != hipSuccess) {
            smk::set_error("preprocess: scores to the resident matrix");
            return -1;
        }
        return 0;
    };
    return smk::matrix_create_sparse_device(out, r->height, r->width, r->nnz, fill);
}

int smk_preprocess_write_mtx(const smk_preprocess_result* r, const char* path, unsigned precision)
{
    if (!r || !path) return SMK_BAD_PARAM;
    if (r->failed) { smk::set_error("preprocess: every column was pruned"); return SMK_FAILURE; }
    std::vector<unsigned> cp((size_t)r->width + 1), rows(r->nnz);
    std::vector<double> scores(r->nnz);
    int rc = smk_preprocess_result_download(r, nullptr, nullptr, cp.data(), rows.data(), scores.data());
    if (rc != SMK_OK) return rc;
    FILE* f = fopen(path, "wb");
    if (!f) { smk::set_error(std::string("could not open ") + path); return SMK_FAILURE; }
    std::string head = "%%MatrixMarket matrix coordinate real general\n" + std::to_string(r->height) + " " + std::to_string(r->width) +
                       " " + std::to_string(r->nnz) + "\n";
    bool ok = fwrite(head.data(), 1, head.size(), f) == head.size();
    // rounds of `threads` chunks of whole columns; each thread formats its chunk, the chunks go out in order.  About 2^22
    // lines (~100 MB of text) are in flight per round, whatever the thread count.
    const int threads = writer_threads();
    const size_t chunk_entries = std::max<size_t>(1u << 14, (1u << 22) / (size_t)threads);
    std::vector<std::string> buf((size_t)threads);
    unsigned c = 0;
    const int prec = (int)precision;
    while (ok && c < r->width) {
        std::vector<std::pair<unsigned, unsigned>> ranges;
        while (c < r->width && (int)ranges.size() < threads) {
            const unsigned c0 = c;
            while (c < r->width && cp[c] - cp[c0] < chunk_entries) ++c;
            ranges.emplace_back(c0, c);
        }
        auto format = [&](size_t t) {
            std::string& s = buf[t];
            s.clear();
            char line[512];
            for (unsigned j = ranges[t].first; j < ranges[t].second; ++j)
                for (unsigned p = cp[j]; p < cp[j + 1]; ++p) {
                    const int n = snprintf(line, sizeof line, "%u %u %.*f\n", rows[p] + 1, j + 1, prec, scores[p]);
                    s.append(line, n > 0 ? (size_t)std::min(n, (int)sizeof line - 1) : 0);
                }
        };
        std::vector<std::thread> pool;
        for (size_t t = 1; t < ranges.size(); ++t) pool.emplace_back(format, t);
        format(0);
        for (auto& th : pool) th.join();
        for (size_t t = 0; t < ranges.size() && ok; ++t) ok = fwrite(buf[t].data(), 1, buf[t].size(), f) == buf[t].size();
    }
    if (fclose(f) != 0) ok = false;
    if (!ok) { smk::set_error(std::string("could not write ") + path); return SMK_FAILURE; }
    return SMK_OK;
}

}  // extern "C"
