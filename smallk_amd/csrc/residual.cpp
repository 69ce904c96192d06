// smallk_amd/csrc/residual.cpp -- the reconstruction error of a factorisation (include/smallk_amd.h: smk_matrix_residual,
// smk_matrix_residual_device, smk_solver_residual).  The three entries differ in where the factors come from;
// each brings them into a workspace of its own (Wt: m rows of KP doubles, H: n columns of KP doubles, pad rows zero) and runs
// residual_run on it.  Every workspace belongs to an smk::Owned local of the entry and is released on every path; nothing is
// written into a matrix or solver handle except the once-per-matrix duplicate record of a sparse matrix.
#include "state.h"

#include <algorithm>
#include <mutex>
#include <string>
#include <utility>
#include <vector>

namespace smk {

// Does the CSC store an entry twice?  Then sum a_e^2 over the stored entries is not ||A||^2 (the other two terms of the sparse
// formula are linear in the stored values and right as they are), and the sum of squares per column is taken from the merged
// entries, once, on the host copy of the CSC (off the hot path), and kept on the device.
int ensure_dup_record(const smk_matrix* a)
{
    static std::mutex mu;             // lazily built part of a shared, nominally const matrix (as ensure_seg_plans)
    std::lock_guard<std::mutex> lk(mu);
    if (a->dup_state >= 0) return 0;
    int rc = matrix_host_csc(a);
    if (rc) return rc;
    std::vector<double> colsq((size_t)a->n, 0.0);
    std::vector<std::pair<unsigned, double>> col;
    bool any = false;
    for (i64 j = 0; j < a->n; ++j) {
        const size_t p0 = a->h_colptr[(size_t)j], p1 = a->h_colptr[(size_t)j + 1];
        col.clear();
        for (size_t p = p0; p < p1; ++p) col.emplace_back(a->h_rowidx[p], a->h_val[p]);
        std::stable_sort(col.begin(), col.end(), [](const auto& x, const auto& y) { return x.first < y.first; });
        double s = 0.0;
        for (size_t q = 0; q < col.size();) {
            double v = col[q].second;
            size_t e = q + 1;
            for (; e < col.size() && col[e].first == col[q].first; ++e) { v += col[e].second; any = true; }
            s += v * v;
            q = e;
        }
        colsq[(size_t)j] = s;
    }
    if (any) {
        if (a->own.dev(&a->dup_colsq, (size_t)a->n)) { set_error("residual: no memory for the merged column sums"); return SMK_DEVICE_ERROR; }
        SMK_HIP(hipMemcpy(a->dup_colsq, colsq.data(), colsq.size() * sizeof(double), hipMemcpyHostToDevice));
    }
    a->dup_state = any ? 1 : 0;
    return 0;
}

// Wt / H: the workspace copies (ldf = KP doubles per row of W / column of H), complete on `st` in stream order.
// col_dev (optional): n contiguous doubles in device memory; col_host (optional): the same on the host.  Synchronises `st`.
static int residual_run(const smk_matrix* a, int k, const double* Wt, const double* H, int ldf, hipStream_t st, Owned& own,
                        double* resid_sq, double* a_sq, double* col_dev, double* col_host)
{
    double *col_r = nullptr, *col_a = nullptr, *out2 = nullptr, *scratch = nullptr;
    int rc = own.dev(&col_r, (size_t)a->n);
    if (!rc) rc = own.dev(&col_a, (size_t)a->n);
    if (!rc) rc = own.dev(&out2, 2);
    if (rc) return rc;
    if (!a->sparse) {
        rc = own.dev(&scratch, residual_dense_scratch_elems(a->m, a->n, ctx().cus));
        if (!rc) rc = launch_residual_dense(a->A, a->storage, a->ldA, a->m, a->n, Wt, H, ldf, k, scratch, col_r, col_a, out2, ctx().cus, st);
        if (rc) return rc;
    } else {
        rc = ensure_dup_record(a);
        if (rc) return rc;
        // the entry-balanced segments of CSC(A), read-only; a matrix without a plan (SMK_SPMM_SEG=0) gets one for this call
        ensure_seg_plans(a);
        SegPlan local;
        struct FreeLocal { SegPlan* p; ~FreeLocal() { free_seg_plan(p); } } free_local{&local};
        const SegPlan* sp = &a->segA;
        if (!sp->rowflag || sp->ncols != a->n) {
            rc = build_seg_plan(a->n, a->nnz, a->colptr, a->rowidx, &local, st);
            if (rc) return rc;
            sp = &local;
        }
        // W'W into scratch of this call (never into a solver's Gram matrices)
        const int KP = ldf;
        double *G = nullptr, *gscratch = nullptr;
        rc = own.dev(&G, (size_t)KP * KP);
        if (!rc) rc = own.dev(&gscratch, gram_scratch_elems(k, GRAM_BLOCKS));
        if (!rc) rc = own.dev(&scratch, residual_sparse_scratch_elems(*sp, a->n));
        if (!rc) rc = launch_gram(Wt, k, a->m, G, gscratch, GRAM_BLOCKS, st);
        if (!rc) rc = launch_residual_sparse(*sp, a->colptr, a->val, a->n, Wt, H, ldf, k, G, KP, a->dup_state == 1 ? a->dup_colsq : nullptr, scratch,
                                             col_r, col_a, out2, st);
        if (!rc) SMK_HIP(hipStreamSynchronize(st));        // the local plan is freed on return
        if (rc) return rc;
    }
    double h2[2] = {0.0, 0.0};
    SMK_HIP(hipMemcpyAsync(h2, out2, sizeof(h2), hipMemcpyDeviceToHost, st));
    if (col_dev) SMK_HIP(hipMemcpyAsync(col_dev, col_r, (size_t)a->n * sizeof(double), hipMemcpyDeviceToDevice, st));
    if (col_host) SMK_HIP(hipMemcpyAsync(col_host, col_r, (size_t)a->n * sizeof(double), hipMemcpyDeviceToHost, st));
    SMK_HIP(hipStreamSynchronize(st));
    *resid_sq = h2[0];
    *a_sq = h2[1];
    return SMK_OK;
}

// what every entry checks first
static int residual_args(const char* who, const smk_matrix* a, int k, const void* W, const void* H, const double* resid_sq, const double* a_sq)
{
    const std::string w(who);
    if (!ctx().init) { set_error("smk_initialize() has not been called"); return SMK_NOTINITIALIZED; }
    if (!a || !W || !H) { set_error(w + ": null matrix or factor"); return SMK_BAD_PARAM; }
    if (!resid_sq || !a_sq) { set_error(w + ": null output"); return SMK_BAD_PARAM; }
    if (k < 1) { set_error(w + ": k < 1"); return SMK_BAD_PARAM; }
    if (k > MAX_K) { set_error(w + ": device path supports k <= 2048"); return SMK_UNSUPPORTED; }
    return SMK_OK;
}

// the zeroed workspace copies of the factors
static int residual_workspace(const smk_matrix* a, int KP, hipStream_t st, Owned& own, double** Wt, double** H)
{
    int rc = own.dev(Wt, (size_t)KP * a->m);
    if (!rc) rc = own.dev(H, (size_t)KP * a->n);
    if (rc) { set_error("residual: no memory for the factor workspace"); return SMK_DEVICE_ERROR; }
    SMK_HIP(hipMemsetAsync(*Wt, 0, (size_t)KP * a->m * sizeof(double), st));
    SMK_HIP(hipMemsetAsync(*H, 0, (size_t)KP * a->n * sizeof(double), st));
    return 0;
}

// factors in device memory as strided views (W m x k, H k x n) -> workspace -> residual_run
static int residual_from_views(const smk_matrix* a, int k, const void* W, int dtypeW, i64 rsW, i64 csW, const void* H, int dtypeH, i64 rsH,
                               i64 csH, hipStream_t st, Owned& own, double* resid_sq, double* a_sq, double* col_dev, double* col_host)
{
    const int KP = kp_of(k);
    double *Wt = nullptr, *Hc = nullptr;
    int rc = residual_workspace(a, KP, st, own, &Wt, &Hc);
    if (!rc) rc = launch_strided_convert(W, dtypeW, rsW, csW, Wt, DT_F64, KP, 1, a->m, k, st);
    if (!rc) rc = launch_strided_convert(H, dtypeH, rsH, csH, Hc, DT_F64, 1, KP, k, a->n, st);
    if (rc) return rc;
    return residual_run(a, k, Wt, Hc, KP, st, own, resid_sq, a_sq, col_dev, col_host);
}

}  // namespace smk

extern "C" {

int smk_matrix_residual(const smk_matrix* a, int k, const double* W, int64_t ldW, const double* H, int64_t ldH, double* resid_sq,
                        double* a_sq, double* col_resid_sq)
{
    int rc = residual_args("smk_matrix_residual", a, k, W, H, resid_sq, a_sq);
    if (rc) return rc;
    if (ldW < a->m || ldH < k) { set_error("smk_matrix_residual: leading dimension too small"); return SMK_BAD_PARAM; }
    Owned own;
    hipStream_t st = a->st ? a->st : ctx().stream;
    // W (m x k, host, column-major) -> a contiguous device copy, then as a view; H (k x n) likewise
    double *dW = nullptr, *dH = nullptr;
    rc = own.dev(&dW, (size_t)a->m * k);
    if (!rc) rc = own.dev(&dH, (size_t)a->n * k);
    if (rc) { set_error("smk_matrix_residual: no memory for the factors"); return SMK_DEVICE_ERROR; }
    SMK_HIP(hipMemcpy2DAsync(dW, (size_t)a->m * sizeof(double), W, (size_t)ldW * sizeof(double), (size_t)a->m * sizeof(double), (size_t)k,
                             hipMemcpyHostToDevice, st));
    SMK_HIP(hipMemcpy2DAsync(dH, (size_t)k * sizeof(double), H, (size_t)ldH * sizeof(double), (size_t)k * sizeof(double), (size_t)a->n,
                             hipMemcpyHostToDevice, st));
    return residual_from_views(a, k, dW, DT_F64, 1, a->m, dH, DT_F64, 1, k, st, own, resid_sq, a_sq, nullptr, col_resid_sq);
}

int smk_matrix_residual_device(const smk_matrix* a, int k, const void* W, int dtypeW, int64_t rsW, int64_t csW, const void* H, int dtypeH,
                               int64_t rsH, int64_t csH, void* stream, double* resid_sq, double* a_sq, void* col_resid_sq)
{
    int rc = residual_args("smk_matrix_residual_device", a, k, W, H, resid_sq, a_sq);
    if (rc) return rc;
    if ((dtypeW != SMK_DT_F64 && dtypeW != SMK_DT_F32) || (dtypeH != SMK_DT_F64 && dtypeH != SMK_DT_F32)) {
        set_error("smk_matrix_residual_device: factors are fp64 or fp32");
        return SMK_BAD_PARAM;
    }
    rc = check_device_view(W, dtypeW, a->m, k, rsW, csW, false, "smk_matrix_residual_device(W)");
    if (!rc) rc = check_device_view(H, dtypeH, k, a->n, rsH, csH, false, "smk_matrix_residual_device(H)");
    if (!rc && col_resid_sq) rc = check_device_view(col_resid_sq, DT_F64, a->n, 1, 1, a->n, true, "smk_matrix_residual_device(col_resid_sq)");
    if (rc) return rc;
    Owned own;
    hipStream_t st = a->st ? a->st : ctx().stream;
    rc = join_caller_stream(own, st, stream);
    if (rc) return rc;
    return residual_from_views(a, k, W, dtypeW, rsW, csW, H, dtypeH, rsH, csH, st, own, resid_sq, a_sq, (double*)col_resid_sq, nullptr);
}

// The solver's current fp64 factors, copied as smk_solver_get_factors_device(normalize = 0) would see them (Wt and H hold them on
// every route, RANK2's compact copies and the resident kernel included: both write Wt / H as well), on the solver's stream.  The
// solver is only read: no field of it is written, nothing is launched that writes its buffers.
int smk_solver_residual(smk_solver* s, double* resid_sq, double* a_sq, double* col_resid_sq)
{
    if (!s) { set_error("smk_solver_residual: null solver"); return SMK_BAD_PARAM; }
    int rc = residual_args("smk_solver_residual", s->a, s->k, s->Wt, s->H, resid_sq, a_sq);
    if (rc) return rc;
    if (s->ar || s->comm) { set_error("smk_solver_residual: not available on a solver with a communicator"); return SMK_UNSUPPORTED; }
    if (!s->have_factors) { set_error("smk_solver_residual: the solver has no factors yet"); return SMK_BAD_PARAM; }
    Owned own;
    return residual_from_views(s->a, s->k, s->Wt, DT_F64, s->KP, 1, s->H, DT_F64, 1, s->KP, s->st, own, resid_sq, a_sq, nullptr, col_resid_sq);
}

}  // extern "C"
