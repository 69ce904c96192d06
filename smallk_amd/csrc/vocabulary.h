// smallk_amd/csrc/vocabulary.h -- launchers of the passes that score new documents against a fitted term set and idf
// (vocabulary.hip), driven by vocabulary.cpp.  Device pointers everywhere, all asynchronous on `st`; 0 on success, -100
// (SMK_DEVICE_ERROR) otherwise.
#pragma once
#include "common.h"

namespace smk {

constexpr unsigned VOC_PRUNED = 0xFFFFFFFFu;          // old_to_new of a term that did not survive the fit

// old_to_new[0 .. height_in) = VOC_PRUNED, then old_to_new[term[i]] = i for i < height
int voc_scatter(const unsigned* term, unsigned height, unsigned height_in, unsigned* old_to_new, hipStream_t st);
// count pass: n = entries of column c whose term survived; flag[c] = n >= min_terms, len[c] = flag[c] ? n : 0;
// flag[width] = len[width] = 0 close the scans
int voc_count(const unsigned* cp, const uint2* ent, unsigned width, const unsigned* old_to_new, unsigned min_terms, unsigned* flag,
              unsigned* len, hipStream_t st);
// fill-and-score pass: kept column c (flag) becomes column cpos[c] at entry offset dst[c]: the surviving entries in order with
// their new rows, their tf-idf scores with the column normalised, doc2[cpos[c]] = c, cp2[cpos[c]] = dst[c];
// cp2[cpos[width]] = dst[width]
int voc_fill_score(const unsigned* cp, const uint2* ent, unsigned width, const unsigned* old_to_new, const double* idf,
                   const unsigned* flag, const unsigned* cpos, const unsigned* dst, unsigned* cp2, uint2* ent2, double* score,
                   unsigned* doc2, hipStream_t st);
// index arrays of a caller (checked already) to 32 bits: out[i] = in[i]
int voc_narrow_i64(const long long* in, i64 n, unsigned* out, hipStream_t st);

}  // namespace smk
