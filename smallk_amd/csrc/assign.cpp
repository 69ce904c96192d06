// smallk_amd/csrc/assign.cpp -- labels, memberships and top terms of factors that are in device memory (include/smallk_amd.h:
// smk_labels_device, smk_top_terms_device).  The kernels (assign.hip) read a factor in its k-contiguous layout; a
// view in any other layout is converted into a workspace first.  Every workspace belongs to the smk::Entry local of the entry
// (entry.h: synchronised before it releases them).  The solver's entries (factors.cpp: smk_solver_labels, smk_solver_top_terms)
// come through the same two functions with the resident H and Wt, which are k-contiguous as they stand: no copy.
#include "entry.h"

#include <string>

namespace smk {

int labels_from_view(const void* H, int dtype, i64 rs, i64 cs, int k, i64 n, hipStream_t st, Owned& own, void* labels, void* memberships)
{
    const void* src = H;
    i64 ldc = cs;
    int dt = dtype;
    if (rs != 1 && k > 1) {                  // rows of H are not consecutive in memory: a compact fp64 copy, column c at c * k
        double* ws = nullptr;
        if (own.dev(&ws, (size_t)k * (size_t)n)) { set_error("labels: no memory for the workspace copy of H"); return SMK_DEVICE_ERROR; }
        const int rc = convert_view(DeviceView::in(H, dtype, rs, cs), DeviceView::cols(ws, k), k, n, st);
        if (rc) return rc;
        src = ws; ldc = k; dt = DT_F64;
    }
    const int rc = launch_labels(src, dt, ldc, k, n, (unsigned*)labels, (float*)memberships, st);
    if (rc) return rc;
    SMK_HIP(hipStreamSynchronize(st));       // the workspace is freed on return, the caller's stream may read the results
    return SMK_OK;
}

int top_terms_from_view(const void* W, int dtype, i64 rs, i64 cs, i64 m, int k, int maxterms, hipStream_t st, Owned& own, void* term_indices)
{
    const void* src = W;
    i64 ld = rs;
    int dt = dtype;
    if (cs != 1 && k > 1) {                  // columns of W are not consecutive in memory: a compact fp64 copy, row i at i * k
        double* ws = nullptr;
        if (own.dev(&ws, (size_t)m * (size_t)k)) { set_error("top terms: no memory for the workspace copy of W"); return SMK_DEVICE_ERROR; }
        const int rc = convert_view(DeviceView::in(W, dtype, rs, cs), DeviceView::rows(ws, k), m, k, st);
        if (rc) return rc;
        src = ws; ld = k; dt = DT_F64;
    }
    int rc;
    if (maxterms <= TOPTERMS_CAP) {
        unsigned char* scratch = nullptr;
        const size_t bytes = topterms_scratch_bytes(m, k, maxterms, ctx().cus);
        if (bytes && own.dev(&scratch, bytes)) { set_error("top terms: no memory for the candidates"); return SMK_DEVICE_ERROR; }
        rc = launch_top_terms(src, dt, ld, m, k, maxterms, scratch, (int*)term_indices, ctx().cus, st);
    } else {
        rc = launch_top_terms_sorted(src, dt, ld, m, k, maxterms, (int*)term_indices, st);
    }
    if (rc) return rc;
    SMK_HIP(hipStreamSynchronize(st));
    return SMK_OK;
}

// what both entries check first
static int assign_args(const char* who, const void* factor, int dtype, int k, i64 extent, const char* extent_name)
{
    const std::string w(who);
    if (int rc = require_init()) return rc;
    if (!factor) { set_error(w + ": null factor"); return SMK_BAD_PARAM; }
    if (k < 1) { set_error(w + ": k < 1"); return SMK_BAD_PARAM; }
    if (extent < 1) { set_error(w + ": " + extent_name + " < 1"); return SMK_BAD_PARAM; }
    if (!is_factor_dtype(dtype)) { set_error(w + ": factors are fp64 or fp32"); return SMK_BAD_PARAM; }
    if (k > MAX_K) { set_error(w + ": device path supports k <= 2048"); return SMK_UNSUPPORTED; }
    return SMK_OK;
}

}  // namespace smk

extern "C" {

int smk_labels_device(const void* H, int dtype, int64_t rsH, int64_t csH, int k, int64_t n, void* stream, void* labels, void* memberships)
{
    int rc = assign_args("smk_labels_device", H, dtype, k, n, "n");
    if (rc) return rc;
    if (!labels) { set_error("smk_labels_device: null output"); return SMK_BAD_PARAM; }
    rc = check_device_view(H, dtype, k, n, rsH, csH, false, "smk_labels_device(H)");
    // (labels are 32-bit integers: the extent of as many 4-byte elements)
    if (!rc) rc = check_device_view(labels, DT_F32, n, 1, 1, n, true, "smk_labels_device(labels)");
    if (!rc && memberships) rc = check_device_view(memberships, DT_F32, k, n, 1, k, true, "smk_labels_device(memberships)");
    if (rc) return rc;
    Entry e(ctx().stream);
    rc = e.join(stream);
    if (rc) return rc;
    return e.synced(labels_from_view(H, dtype, rsH, csH, k, n, e.st, e.own, labels, memberships));
}

int smk_top_terms_device(const void* W, int dtype, int64_t rsW, int64_t csW, int64_t m, int k, int maxterms, void* stream, void* term_indices)
{
    int rc = assign_args("smk_top_terms_device", W, dtype, k, m, "m");
    if (rc) return rc;
    if (maxterms < 1) { set_error("smk_top_terms_device: maxterms < 1"); return SMK_BAD_PARAM; }
    if (!term_indices) { set_error("smk_top_terms_device: null output"); return SMK_BAD_PARAM; }
    if (m > 0x7FFFFFFFll) { set_error("smk_top_terms_device: term indices are 32-bit"); return SMK_UNSUPPORTED; }
    rc = check_device_view(W, dtype, m, k, rsW, csW, false, "smk_top_terms_device(W)");
    if (!rc) rc = check_device_view(term_indices, DT_F32, maxterms, k, 1, maxterms, true, "smk_top_terms_device(term_indices)");
    if (rc) return rc;
    Entry e(ctx().stream);
    rc = e.join(stream);
    if (rc) return rc;
    return e.synced(top_terms_from_view(W, dtype, rsW, csW, m, k, maxterms, e.st, e.own, term_indices));
}

}  // extern "C"
