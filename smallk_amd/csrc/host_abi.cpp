// smallk_amd/csrc/host_abi.cpp -- the part of the C ABI (include/smallk_amd.h) that never touches the HIP runtime:
// the error string, option validation, the host generator, the CSC bookkeeping and the one-call drivers, which are
// compositions of public smk_* calls.  tests/asan compiles this file as it is, with the host compiler.
#include "common.h"
#include "../../include/smallk_amd.h"

#include <algorithm>
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

namespace smk {

static thread_local std::string g_err;

void set_error(const std::string& msg) { g_err = msg; }

}  // namespace smk

using namespace smk;

extern "C" {

const char* smk_last_error(void) { return g_err.c_str(); }

// IsValid, common/src/nmf_options.cpp:23-112 (same checks, same messages)
int smk_is_valid(const smk_options* o, int validate_matrix)
{
    if (!o) return 0;
    if (o->k <= 0) { fprintf(stderr, "nmflib error: k-value must be a positive integer\n"); return 0; }
    if (validate_matrix) {
        if (o->height <= 0) { fprintf(stderr, "nmflib error: matrix height must be a positive integer\n"); return 0; }
        if (o->width <= 0) { fprintf(stderr, "nmflib error: matrix width must be a positive integer\n"); return 0; }
        if (o->k > o->width) { fprintf(stderr, "nmflib error: k value cannot exceed the number of columns\n"); return 0; }
    }
    if (o->tol <= 0.0 || o->tol >= 1.0) { fprintf(stderr, "nmflib error: tolerance must be in the interval (0.0, 1.0)\n"); return 0; }
    if (o->min_iter <= 0) { fprintf(stderr, "nmflib error: miniter must be a positive integer\n"); return 0; }
    if (o->max_iter <= 0) { fprintf(stderr, "nmflib error: maxiter must be a positive integer\n"); return 0; }
    if (o->tolcount <= 0) { fprintf(stderr, "nmflib error: tolcount must be a positive integer\n"); return 0; }
    if (o->algorithm != SMK_ALG_MU && o->algorithm != SMK_ALG_HALS && o->algorithm != SMK_ALG_RANK2 &&
        o->algorithm != SMK_ALG_BPP) {
        fprintf(stderr, "nmflib error: unknown NMF algorithm specified\n");
        return 0;
    }
    if (o->algorithm == SMK_ALG_RANK2 && o->k != 2) { fprintf(stderr, "nmflib error: RANK2 algorithm requires k == 2\n"); return 0; }
    if (o->prog_est_algorithm != SMK_PROG_PG_RATIO && o->prog_est_algorithm != SMK_PROG_DELTA_FNORM) {
        fprintf(stderr, "nmflib error: unknown stopping criterion specified\n");
        return 0;
    }
    return 1;
}

// same generator as the device fill (kernels.hip) and the oracle, on the host
static inline uint64_t h_mix64(uint64_t z)
{
    z += 0x9E3779B97F4A7C15ull;
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    return z ^ (z >> 31);
}

void smk_uniform_fill_host(double* buf, int64_t ld, int64_t rows, int64_t cols, int64_t r0, int64_t c0,
                           int64_t gheight, uint64_t seed, int quant)
{
    for (int64_t c = 0; c < cols; ++c)
        for (int64_t r = 0; r < rows; ++r) {
            uint64_t h = h_mix64(seed * 0xD1342543DE82EF95ull + (uint64_t)((c0 + c) * gheight + (r0 + r)));
            float f = (float)(h >> 40) * (1.0f / 16777216.0f);
            if (quant == 1) {
                uint32_t b;
                memcpy(&b, &f, 4);
                b += 0x7FFFu + ((b >> 16) & 1u);
                b &= 0xFFFF0000u;
                memcpy(&f, &b, 4);
            }
            buf[c * ld + r] = (double)f;
        }
}

// ---- host-side CSC bookkeeping (no device involved; pinned against the reference's own SparseMatrix code
// compiled in place, oracle/_ref/libref_sparse.so, by tests/test_ref_sparse.py) -------------------------
// Transpose(SparseMatrix), common/include/sparse_matrix_ops.hpp:36-127: counting sort by row; inside a
// row of the result the entries keep the source's column order.
int smk_csc_transpose(int64_t height, int64_t width, const unsigned* col_offsets, const unsigned* row_indices,
                      const double* data, unsigned* out_col_offsets /* height+1 */, unsigned* out_row_indices,
                      double* out_data)
{
    if (height < 0 || width < 0 || !col_offsets || !out_col_offsets) return SMK_BAD_PARAM;
    const unsigned base = col_offsets[0];
    const int64_t nnz = (int64_t)col_offsets[width] - base;
    if (nnz > 0 && (!row_indices || !data || !out_row_indices || !out_data)) return SMK_BAD_PARAM;
    std::vector<i64> cnt((size_t)height + 1, 0);
    for (int64_t p = 0; p < nnz; ++p) {
        if ((int64_t)row_indices[base + p] >= height) { set_error("row index out of range"); return SMK_BAD_PARAM; }
        cnt[(size_t)row_indices[base + p] + 1] += 1;
    }
    for (int64_t r = 0; r < height; ++r) cnt[(size_t)r + 1] += cnt[(size_t)r];
    for (int64_t r = 0; r <= height; ++r) out_col_offsets[r] = (unsigned)cnt[(size_t)r];
    std::vector<i64> fill(cnt.begin(), cnt.end() - 1);
    for (int64_t c = 0; c < width; ++c)
        for (i64 p = (i64)col_offsets[c] - base; p < (i64)col_offsets[c + 1] - base; ++p) {
            const i64 q = fill[row_indices[base + p]]++;
            out_row_indices[q] = (unsigned)c;
            out_data[q] = data[base + p];
        }
    return SMK_OK;
}

// SparseMatrix::SubMatrixColsCompact, common/include/sparse_matrix_impl.hpp:478-592: the listed columns in
// the listed order, rows without a stored entry dropped and the rest renumbered in increasing order.
// Call once with out_* NULL for the sizes (*out_nnz, *new_height), then with arrays of that capacity.
// old_to_new (height entries, 0xFFFFFFFF = dropped) and new_to_old may be NULL.
int smk_csc_subset_cols_compact(int64_t height, int64_t width, const unsigned* col_offsets, const unsigned* row_indices,
                                const double* data, const unsigned* cols, int64_t ncols, unsigned* out_col_offsets,
                                unsigned* out_row_indices, double* out_data, unsigned* old_to_new, unsigned* new_to_old,
                                int64_t* new_height, int64_t* out_nnz)
{
    if (height <= 0 || width <= 0 || !col_offsets || !cols || ncols <= 0) { set_error("SubMatrixColsCompact: empty column set"); return SMK_BAD_PARAM; }
    const unsigned UNUSED = 0xFFFFFFFFu;
    std::vector<unsigned> o2n((size_t)height, UNUSED);
    int64_t total = 0;
    for (int64_t j = 0; j < ncols; ++j) {
        if ((int64_t)cols[j] >= width) { set_error("SubMatrixColsCompact: column index out of range"); return SMK_BAD_PARAM; }
        for (unsigned p = col_offsets[cols[j]]; p < col_offsets[cols[j] + 1]; ++p) o2n[row_indices[p]] = 0;
        total += col_offsets[cols[j] + 1] - col_offsets[cols[j]];
    }
    if (total == 0) { set_error("SparseMatrix::SubMatrixColsCompact: submatrix is the zero matrix"); return SMK_BAD_PARAM; }
    int64_t nh = 0;
    for (int64_t r = 0; r < height; ++r)
        if (o2n[(size_t)r] != UNUSED) {
            o2n[(size_t)r] = (unsigned)nh;
            if (new_to_old) new_to_old[nh] = (unsigned)r;
            ++nh;
        }
    if (old_to_new) std::copy(o2n.begin(), o2n.end(), old_to_new);
    if (new_height) *new_height = nh;
    if (out_nnz) *out_nnz = total;
    if (!out_col_offsets) return SMK_OK;
    if (!out_row_indices || !out_data) return SMK_BAD_PARAM;
    unsigned q = 0;
    for (int64_t j = 0; j < ncols; ++j) {
        out_col_offsets[j] = q;
        for (unsigned p = col_offsets[cols[j]]; p < col_offsets[cols[j] + 1]; ++p, ++q) {
            out_row_indices[q] = o2n[row_indices[p]];
            out_data[q] = data[p];
        }
    }
    out_col_offsets[ncols] = q;
    return SMK_OK;
}

// Result Nmf(...), common/src/nmf.cpp:173-229
int smk_nmf_dense(const smk_options* opts, const double* A, int64_t ldA, double* W, int64_t ldW, double* H,
                  int64_t ldH, smk_stats* stats, int storage)
{
    if (smk_is_initialized() != SMK_INITIALIZED) {
        fprintf(stderr, "nmflib error: nmf_initialize() must be called prior to any factorization routine\n\n");
        return SMK_NOTINITIALIZED;
    }
    if (!opts || !smk_is_valid(opts, 1)) return SMK_BAD_PARAM;
    if (!A || !W || !H) return SMK_BAD_PARAM;
    if (opts->k > MAX_K || (opts->algorithm == SMK_ALG_BPP && opts->k > MAX_K_BPP)) { set_error("device path supports k <= 2048"); return SMK_UNSUPPORTED; }     // before anything is uploaded
    const int64_t m = opts->height, n = opts->width;
    if (ldA < m || ldW < m || ldH < opts->k) { set_error("leading dimension too small"); return SMK_BAD_PARAM; }
    smk_matrix* a = nullptr;
    smk_solver* s = nullptr;
    int rc = smk_matrix_create(&a, m, n, 0, n, storage);
    if (rc == SMK_OK) rc = smk_matrix_upload_f64(a, A, ldA);
    if (rc == SMK_OK) rc = smk_solver_create(&s, opts, a);
    if (rc == SMK_OK) rc = smk_solver_set_factors(s, W, ldW, H, ldH);
    int run_rc = SMK_OK;
    if (rc == SMK_OK) {
        run_rc = smk_solver_run(s, stats);
        // like the reference, W/H hold the last iterate even when the solver reports failure
        if (run_rc == SMK_OK || run_rc == SMK_FAILURE) (void)smk_solver_get_factors(s, 0, W, ldW, H, ldH);
        rc = run_rc;
    }
    smk_solver_destroy(s);
    smk_matrix_destroy(a);
    return rc;
}

// Result NmfSparse(...), common/src/nmf.cpp:232-300 (CSC input, 32-bit indices as in the reference)
int smk_nmf_sparse(const smk_options* opts, unsigned height, unsigned width, unsigned nz, const unsigned* col_offsets,
                   const unsigned* row_indices, const double* data, double* W, int64_t ldW, double* H, int64_t ldH,
                   smk_stats* stats)
{
    if (smk_is_initialized() != SMK_INITIALIZED) {
        fprintf(stderr, "nmflib error: nmf_initialize() must be called prior to any factorization routine\n\n");
        return SMK_NOTINITIALIZED;
    }
    if (!opts || !smk_is_valid(opts, 1)) return SMK_BAD_PARAM;
    if (!col_offsets || !row_indices || !data || !W || !H) return SMK_BAD_PARAM;
    if (opts->k > MAX_K || (opts->algorithm == SMK_ALG_BPP && opts->k > MAX_K_BPP)) { set_error("device path supports k <= 2048"); return SMK_UNSUPPORTED; }
    if ((int64_t)height != opts->height || (int64_t)width != opts->width) return SMK_BAD_PARAM;
    if (ldW < opts->height || ldH < opts->k) { set_error("leading dimension too small"); return SMK_BAD_PARAM; }
    smk_matrix* a = nullptr;
    smk_solver* s = nullptr;
    int rc = smk_matrix_create_sparse(&a, height, width, 0, width, nz, col_offsets, row_indices, data);
    if (rc == SMK_OK) rc = smk_solver_create(&s, opts, a);
    if (rc == SMK_OK) rc = smk_solver_set_factors(s, W, ldW, H, ldH);
    if (rc == SMK_OK) {
        rc = smk_solver_run(s, stats);
        if (rc == SMK_OK || rc == SMK_FAILURE) (void)smk_solver_get_factors(s, 0, W, ldW, H, ldH);
    }
    smk_solver_destroy(s);
    smk_matrix_destroy(a);
    return rc;
}

}  // extern "C"
