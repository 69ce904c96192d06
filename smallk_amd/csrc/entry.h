// smallk_amd/csrc/entry.h -- what the entries of the C ABI share around their own work: the initialisation check,
// the element types and the stream of a factor view, the two layouts of a resident factor, the lifecycle of a factor pair, the
// penalties of the regularised solvers, the segment plan of a sparse matrix, the timing loop -- and, through Entry, one rule: an
// entry synchronises its stream before its workspaces are released.  Host code only: no .hip file and no header of one reads it.
#pragma once
#include "state.h"

#include <string>

namespace smk {

inline int require_init()
{
    if (ctx().init) return SMK_OK;
    set_error("smk_initialize() has not been called");
    return SMK_NOTINITIALIZED;
}

inline bool is_factor_dtype(int dt) { return dt == SMK_DT_F64 || dt == SMK_DT_F32; }
// "<who>: <what> are fp64 or fp32" unless both element types are
inline int check_factor_dtypes(const std::string& who, const char* what, int dtA, int dtB)
{
    if (is_factor_dtype(dtA) && is_factor_dtype(dtB)) return SMK_OK;
    set_error(who + ": " + what + " are fp64 or fp32");
    return SMK_BAD_PARAM;
}
// the stream of the context that created the matrix (the calling thread's once that context is gone)
inline hipStream_t matrix_stream(const smk_matrix* a) { return a->st ? a->st : ctx().stream; }

// What an entry holds for the length of a call: its stream, the owner of its workspaces and events, the segment plans built for
// this call alone.  The destructor waits for the stream before anything is released, so a return after a failed launch frees
// nothing under launches still in flight.  A path that has synchronised says so (sync / synced) and is not synchronised twice.
class Entry {
    bool armed_ = true;

public:
    const hipStream_t st;
    Owned own;                      // (not copyable, hence neither is an Entry)
    SegPlan planA, planAt;
    explicit Entry(hipStream_t s) : st(s) {}
    ~Entry() { if (armed_) (void)hipStreamSynchronize(st); free_seg_plan(&planA); free_seg_plan(&planAt); }     // then own releases
    int join(void* caller_stream) { return join_caller_stream(own, st, caller_stream); }
    int sync() { armed_ = false; SMK_HIP(hipStreamSynchronize(st)); return SMK_OK; }      // the one synchronise of a path that succeeded
    int synced(int rc) { if (!rc) armed_ = false; return rc; }                              // rc of work that synchronises st when it succeeds
};

// the segments of CSC(A) (transposed: of CSC(A')), read-only: the matrix's own plan, or (SMK_SPMM_SEG=0) one built into `local` on `st`
inline int seg_plan_or_local(const smk_matrix* a, bool transposed, hipStream_t st, SegPlan* local, const SegPlan** out)
{
    ensure_seg_plans(a);
    *out = transposed ? &a->segAt : &a->segA;
    const i64 ncols = transposed ? a->m : a->n;
    if ((*out)->rowflag && (*out)->ncols == ncols) return 0;
    *out = local;
    return build_seg_plan(ncols, a->nnz, transposed ? a->colptr_t : a->colptr, transposed ? a->rowidx_t : a->rowidx, local, st);
}

// A strided view in device memory: element (r, c) at p + r rs + c cs, in elements of dtype.  in(): a view that is only read.
struct DeviceView {
    void* p; int dtype; i64 rs, cs;
    static DeviceView in(const void* p, int dtype, i64 rs, i64 cs) { return {const_cast<void*>(p), dtype, rs, cs}; }
    // the two layouts of a resident factor, ld doubles per row of W / column of H (ld = KP in a workspace: pad rows zero)
    static DeviceView rows(double* ws, i64 ld) { return {ws, DT_F64, ld, 1}; }      // an N x k view: element (i, t) at i ld + t
    static DeviceView cols(double* ws, i64 ld) { return {ws, DT_F64, 1, ld}; }      // a k x N view: element (t, j) at j ld + t
};

inline int convert_view(const DeviceView& src, const DeviceView& dst, i64 rows, i64 cols, hipStream_t st)
{
    return launch_strided_convert(src.p, src.dtype, src.rs, src.cs, dst.p, dst.dtype, dst.rs, dst.cs, rows, cols, st);
}

// W (m x k) and H (k x n) as the resident pair Wt (KP x m) and H (KP x n).  The buffers are the pair's own (alloc_zeroed) or
// somebody else's (a solver's, a finished SVD's).  second_rows: the second view is n x k (the V of an SVD), not k x n.
struct FactorPair {
    i64 m = 0, n = 0;
    int k = 0, KP = 0;
    hipStream_t st = nullptr;
    double *Wt = nullptr, *H = nullptr;
    bool second_rows = false;
    DeviceView first() const { return DeviceView::rows(Wt, KP); }
    DeviceView second() const { return second_rows ? DeviceView::rows(H, KP) : DeviceView::cols(H, KP); }
    i64 rows2() const { return second_rows ? n : k; }
    i64 cols2() const { return second_rows ? k : n; }
    int check(const std::string& who, const DeviceView& W, const DeviceView& Hv, bool writeW, bool writeH, const char* nameW = "W", const char* nameH = "H") const
    {
        const int rc = check_device_view(W.p, W.dtype, m, k, W.rs, W.cs, writeW, (who + "(" + nameW + ")").c_str());
        return rc ? rc : check_device_view(Hv.p, Hv.dtype, rows2(), cols2(), Hv.rs, Hv.cs, writeH, (who + "(" + nameH + ")").c_str());
    }
    int zero() const             // pad rows of the resident layout must be (and stay) zero
    {
        SMK_HIP(hipMemsetAsync(Wt, 0, (size_t)KP * m * sizeof(double), st));
        SMK_HIP(hipMemsetAsync(H, 0, (size_t)KP * n * sizeof(double), st));
        return 0;
    }
    int alloc_zeroed(Owned& own, const std::string& who)
    {
        if (own.dev(&Wt, (size_t)KP * m) || own.dev(&H, (size_t)KP * n)) { set_error(who + ": no memory for the factor workspace"); return SMK_DEVICE_ERROR; }
        return zero();
    }
    int load(const DeviceView& W, const DeviceView& Hv) const
    {
        const int rc = convert_view(W, first(), m, k, st);
        return rc ? rc : convert_view(Hv, second(), rows2(), cols2(), st);
    }
    int store(const DeviceView* W, const DeviceView* Hv) const          // null: that factor stays with the caller as it is
    {
        const int rc = W ? convert_view(first(), *W, m, k, st) : 0;
        return rc || !Hv ? rc : convert_view(second(), *Hv, rows2(), cols2(), st);
    }
};

// the option ranges smk_cd_options and smk_kl_options share ...
inline int check_penalties(const std::string& w, double alpha_w, double alpha_h, double l1_ratio, double tol, int max_iter)
{
    if (!(alpha_w >= 0.0) || !(alpha_h >= 0.0)) { set_error(w + ": alpha_w and alpha_h must be >= 0"); return SMK_BAD_PARAM; }
    if (!(l1_ratio >= 0.0 && l1_ratio <= 1.0)) { set_error(w + ": l1_ratio must lie in [0, 1]"); return SMK_BAD_PARAM; }
    if (!(tol >= 0.0)) { set_error(w + ": tol must be >= 0"); return SMK_BAD_PARAM; }
    if (max_iter < 1) { set_error(w + ": max_iter < 1"); return SMK_BAD_PARAM; }
    return SMK_OK;
}

// what every entry of the two KL-divergence drivers (kl.cpp, kl_dense.cpp) checks first
inline int kl_args(const std::string& w, const smk_matrix* a, int k, const void* W, int dtW, const void* H, int dtH)
{
    if (int rc = require_init()) return rc;
    if (!a || !W || !H) { set_error(w + ": null argument"); return SMK_BAD_PARAM; }
    if (k < 1) { set_error(w + ": k < 1"); return SMK_BAD_PARAM; }
    if (k > a->m || k > a->n_global) { set_error(w + ": k exceeds min(m, n)"); return SMK_BAD_PARAM; }
    return check_factor_dtypes(w, "W and H", dtW, dtH);
}

// kl_dense.cpp: refuses a dense matrix that stores a negative value (SMK_BAD_PARAM); fills a->kl_negative and a->kl_zero once per contents
int kl_dense_sign_check(const smk_matrix* a, const std::string& w);

// ... and what they weigh: the l1 and l2 terms of H scale with m, those of W with n (scikit-learn's convention on X = A')
struct Penalties {
    double l1h, l2h, l1w, l2w;
    Penalties(i64 m, i64 n, double alpha_w, double alpha_h, double l1_ratio)
        : l1h((double)m * alpha_h * l1_ratio), l2h((double)m * alpha_h * (1.0 - l1_ratio)),
          l1w((double)n * alpha_w * l1_ratio), l2w((double)n * alpha_w * (1.0 - l1_ratio)) {}
};

// the average time of `reps` calls of once() on st after three to warm up; waits for the last.  who: the entry, for the error text
template <class Once>
int time_launches(const std::string& who, Owned& own, hipStream_t st, int reps, Once once, double* ms)
{
    hipEvent_t e0 = nullptr, e1 = nullptr;
    if (own.event(&e0, hipEventDefault) || own.event(&e1, hipEventDefault)) { set_error(who + ": no device memory"); return SMK_DEVICE_ERROR; }
    int rc = 0;
    for (int i = 0; i < 3 && !rc; ++i) rc = once();
    if (rc) return rc;
    SMK_HIP(hipEventRecord(e0, st));
    for (int i = 0; i < reps && !rc; ++i) rc = once();
    if (rc) return rc;
    SMK_HIP(hipEventRecord(e1, st));
    SMK_HIP(hipEventSynchronize(e1));
    float t = 0.f;
    SMK_HIP(hipEventElapsedTime(&t, e0, e1));
    *ms = (double)t / reps;
    return SMK_OK;
}

}  // namespace smk
