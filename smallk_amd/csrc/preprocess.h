// smallk_amd/csrc/preprocess.h -- launchers of the preprocess_tf passes (preprocess.hip), driven by preprocess.cpp.
// Device pointers everywhere, all asynchronous on `st` unless noted; 0 on success, -100 (SMK_DEVICE_ERROR) otherwise.
#pragma once
#include "common.h"

namespace smk {

// hipcub workspace kept across the calls of one preprocessing run
struct PpScan {
    void* temp = nullptr;
    size_t cap = 0;
    int exclusive(const unsigned* in, unsigned* out, i64 count, hipStream_t st);
    int sort_pairs(const unsigned long long* kin, unsigned long long* kout, const unsigned* vin, unsigned* vout, i64 n, hipStream_t st);
    void release();
};

// counts from the stored values; *unsorted != 0 afterwards if some column's rows are not in increasing order
int pp_convert(const unsigned* cp, const unsigned* rows, const double* data, unsigned width, int boolean_mode, uint2* ent,
               unsigned* unsorted, hipStream_t st);
// stable sort by row inside every column (synchronous)
int pp_sort_columns(const unsigned* cp, unsigned width, i64 nnz, unsigned height, uint2* ent, hipStream_t st);
// row statistics: stat[r] = tot << 32 | df (tot = the wrapping 32-bit sum of the counts, df = the number of entries)
// stat[r] += count << 32 | 1 for every entry (stat zeroed by the caller)
int pp_row_stats(const uint2* ent, i64 nnz, unsigned long long* stat, hipStream_t st);
// flag[r] = tot[r] >= docs_per_term && df[r] < width, flag[height] = 0
int pp_row_keep(const unsigned long long* stat, unsigned height, unsigned docs_per_term, unsigned width, unsigned* flag, hipStream_t st);
// kept rows to their new index pos[r]: statistics and term indices
int pp_row_gather(const unsigned* flag, const unsigned* pos, unsigned height, const unsigned long long* stat, const unsigned* term,
                  unsigned long long* stat2, unsigned* term2, hipStream_t st);
// len[c] = entries of column c in kept rows, len[width] = 0
int pp_col_count_rows(const unsigned* cp, const uint2* ent, unsigned width, const unsigned* rflag, unsigned* len, hipStream_t st);
// entries in kept rows to ent2 at the offsets cp2, rows renumbered by rpos
int pp_col_fill_rows(const unsigned* cp, const uint2* ent, unsigned width, const unsigned* rflag, const unsigned* rpos,
                     const unsigned* cp2, uint2* ent2, hipStream_t st);
// flag[c] = length of c >= terms_per_doc, flag[width] = 0
int pp_col_keep_len(const unsigned* cp, unsigned width, unsigned terms_per_doc, unsigned* flag, hipStream_t st);
// len[c] = flag[c] ? length of c : 0, len[width] = 0
int pp_col_kept_len(const unsigned* cp, unsigned width, const unsigned* flag, unsigned* len, hipStream_t st);
// the entries of every column with flag[c] == 0 leave their rows' statistics
int pp_col_drop_stats(const unsigned* cp, const uint2* ent, unsigned width, const unsigned* flag, unsigned long long* stat, hipStream_t st);
// kept columns (flag) to column cpos[c] at entry offset dst[c]; doc indices follow; cp2[cpos[width]] = dst[width]
int pp_col_copy(const unsigned* cp, const uint2* ent, unsigned width, const unsigned* flag, const unsigned* cpos, const unsigned* dst,
                const unsigned* doc, unsigned* cp2, uint2* ent2, unsigned* doc2, hipStream_t st);
// hash[c], idx[c] = c
int pp_hash(const unsigned* cp, const uint2* ent, unsigned width, unsigned long long* hash, unsigned* idx, hipStream_t st);
// keep[0..n) = 1, keep[n] = 0, then 0 for every column that has an identical column of larger index.  hs / idx: the hashes
// sorted (stably) with their column indices; differ: n + 1 words of scratch
int pp_dup_resolve(const unsigned* cp, const uint2* ent, const unsigned long long* hs, const unsigned* idx, unsigned n,
                   unsigned* keep, unsigned* differ, hipStream_t st);
// idf (height doubles of scratch) and the tf-idf scores of every entry
int pp_scores(const unsigned* cp, const uint2* ent, unsigned width, const unsigned long long* stat, unsigned height, double* idf,
              double* score, hipStream_t st);
int pp_iota(unsigned* out, unsigned n, hipStream_t st);
// colptr[0..width] = cp (64-bit; skipped when colptr is null), rows[p] = ent[p].x
int pp_export(const unsigned* cp, unsigned width, const uint2* ent, i64 nnz, i64* colptr, unsigned* rows, hipStream_t st);

}  // namespace smk
