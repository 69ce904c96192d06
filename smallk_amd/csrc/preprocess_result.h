// smallk_amd/csrc/preprocess_result.h -- the result object of smk_preprocess and smk_vocabulary_apply (preprocess.cpp and
// vocabulary.cpp fill it, the accessors of preprocess.cpp read it).  Host code only.
#pragma once
#include <vector>

#include "../../include/smallk_amd.h"
#include "common.h"

struct smk_preprocess_result {
    unsigned height = 0, width = 0, nnz = 0, iterations = 0;
    unsigned height_in = 0;                          // the term count of the input (a fit's, or the applied vocabulary's)
    int boolean_mode = 0;
    bool failed = false;
    std::vector<unsigned> log;                       // height, width, nonzeros per iteration
    unsigned *cp = nullptr, *term = nullptr, *doc = nullptr;
    uint2* ent = nullptr;
    double* score = nullptr;
    double* idf = nullptr;                           // idf[height] of the final matrix: what a vocabulary takes over
    double upload_ms = 0.0, device_ms = 0.0;
    ~smk_preprocess_result()
    {
        void* ptrs[] = {cp, term, doc, ent, score, idf};
        for (void* p : ptrs)
            if (p) (void)smk::dev_free(p);
    }
};
