// smallk_amd/csrc/residual.cpp -- the reconstruction error of a factorisation (include/smallk_amd.h: smk_matrix_residual,
// smk_matrix_residual_device, smk_solver_residual).  The three entries differ in where the factors come from;
// each hands them to residual_from_views, which brings them into a workspace FactorPair (entry.h).  Every workspace belongs to
// the smk::Entry local of the entry, which synchronises the stream before it releases them, on every path; nothing is written
// into a matrix or solver handle except the once-per-matrix duplicate record of a sparse matrix.
#include "entry.h"

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

// The factors in device memory as strided views (W m x k, H k x n) -> a zeroed workspace pair (Wt / H, ldf = KP doubles per row of
// W / column of H) -> the sums.  col_dev (optional): n contiguous doubles in device memory; col_host (optional): the same on
// the host.  Synchronises e.st.
static int residual_from_views(Entry& e, const smk_matrix* a, int k, const DeviceView& vW, const DeviceView& vH, double* resid_sq, double* a_sq,
                               double* col_dev, double* col_host)
{
    Owned& own = e.own;
    const hipStream_t st = e.st;
    FactorPair f{a->m, a->n, k, kp_of(k), st};
    int rc = f.alloc_zeroed(own, "residual");
    if (!rc) rc = f.load(vW, vH);
    if (rc) return rc;
    const double *Wt = f.Wt, *H = f.H;
    const int ldf = f.KP;
    double *col_r = nullptr, *col_a = nullptr, *out2 = nullptr, *scratch = nullptr;
    rc = own.dev(&col_r, (size_t)a->n);
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
        const SegPlan* sp = nullptr;
        rc = seg_plan_or_local(a, false, st, &e.planA, &sp);
        if (rc) return rc;
        // W'W into scratch of this call (never into a solver's Gram matrices)
        const int KP = ldf;
        double *G = nullptr, *gscratch = nullptr;
        rc = own.dev(&G, (size_t)KP * KP);
        if (!rc) rc = own.dev(&gscratch, gram_scratch_elems(k, GRAM_BLOCKS));
        if (!rc) rc = own.dev(&scratch, residual_sparse_scratch_elems(*sp, a->n));
        if (!rc) rc = launch_gram(Wt, k, a->m, G, gscratch, GRAM_BLOCKS, st);
        if (!rc) rc = launch_residual_sparse(*sp, a->colptr, a->val, a->n, Wt, H, ldf, k, G, KP, a->dup_state == 1 ? a->dup_colsq : nullptr, scratch,
                                             col_r, col_a, out2, st);
        if (!rc) SMK_HIP(hipStreamSynchronize(st));        // the sparse route waits here as well, as it always has
        if (rc) return rc;
    }
    double h2[2] = {0.0, 0.0};
    SMK_HIP(hipMemcpyAsync(h2, out2, sizeof(h2), hipMemcpyDeviceToHost, st));
    if (col_dev) SMK_HIP(hipMemcpyAsync(col_dev, col_r, (size_t)a->n * sizeof(double), hipMemcpyDeviceToDevice, st));
    if (col_host) SMK_HIP(hipMemcpyAsync(col_host, col_r, (size_t)a->n * sizeof(double), hipMemcpyDeviceToHost, st));
    rc = e.sync();
    if (rc) return rc;
    *resid_sq = h2[0];
    *a_sq = h2[1];
    return SMK_OK;
}

// what every entry checks first
static int residual_args(const char* who, const smk_matrix* a, int k, const void* W, const void* H, const double* resid_sq, const double* a_sq)
{
    const std::string w(who);
    if (int rc = require_init()) return rc;
    if (!a || !W || !H) { set_error(w + ": null matrix or factor"); return SMK_BAD_PARAM; }
    if (!resid_sq || !a_sq) { set_error(w + ": null output"); return SMK_BAD_PARAM; }
    if (k < 1) { set_error(w + ": k < 1"); return SMK_BAD_PARAM; }
    if (k > MAX_K) { set_error(w + ": device path supports k <= 2048"); return SMK_UNSUPPORTED; }
    return SMK_OK;
}

}  // namespace smk

extern "C" {

int smk_matrix_residual(const smk_matrix* a, int k, const double* W, int64_t ldW, const double* H, int64_t ldH, double* resid_sq,
                        double* a_sq, double* col_resid_sq)
{
    int rc = residual_args("smk_matrix_residual", a, k, W, H, resid_sq, a_sq);
    if (rc) return rc;
    if (ldW < a->m || ldH < k) { set_error("smk_matrix_residual: leading dimension too small"); return SMK_BAD_PARAM; }
    Entry e(matrix_stream(a));
    // W (m x k, host, column-major) -> a contiguous device copy, then as a view; H (k x n) likewise
    double *dW = nullptr, *dH = nullptr;
    rc = e.own.dev(&dW, (size_t)a->m * k);
    if (!rc) rc = e.own.dev(&dH, (size_t)a->n * k);
    if (rc) { set_error("smk_matrix_residual: no memory for the factors"); return SMK_DEVICE_ERROR; }
    SMK_HIP(hipMemcpy2DAsync(dW, (size_t)a->m * sizeof(double), W, (size_t)ldW * sizeof(double), (size_t)a->m * sizeof(double), (size_t)k,
                             hipMemcpyHostToDevice, e.st));
    SMK_HIP(hipMemcpy2DAsync(dH, (size_t)k * sizeof(double), H, (size_t)ldH * sizeof(double), (size_t)k * sizeof(double), (size_t)a->n,
                             hipMemcpyHostToDevice, e.st));
    return residual_from_views(e, a, k, DeviceView::cols(dW, a->m), DeviceView::cols(dH, k), resid_sq, a_sq, nullptr, col_resid_sq);
}

int smk_matrix_residual_device(const smk_matrix* a, int k, const void* W, int dtypeW, int64_t rsW, int64_t csW, const void* H, int dtypeH,
                               int64_t rsH, int64_t csH, void* stream, double* resid_sq, double* a_sq, void* col_resid_sq)
{
    const char* who = "smk_matrix_residual_device";
    int rc = residual_args(who, a, k, W, H, resid_sq, a_sq);
    if (!rc) rc = check_factor_dtypes(who, "factors", dtypeW, dtypeH);
    if (rc) return rc;
    const DeviceView vW = DeviceView::in(W, dtypeW, rsW, csW), vH = DeviceView::in(H, dtypeH, rsH, csH);
    rc = FactorPair{a->m, a->n, k}.check(who, vW, vH, false, false);
    if (!rc && col_resid_sq) rc = check_device_view(col_resid_sq, DT_F64, a->n, 1, 1, a->n, true, "smk_matrix_residual_device(col_resid_sq)");
    if (rc) return rc;
    Entry e(matrix_stream(a));
    rc = e.join(stream);
    if (rc) return rc;
    return residual_from_views(e, a, k, vW, vH, resid_sq, a_sq, (double*)col_resid_sq, nullptr);
}

// The solver's current fp64 factors, copied as smk_solver_get_factors_device(normalize = 0) would see them (Wt and H hold them on
// every route, RANK2's compact copies and the resident kernel included: both write Wt / H as well), on the solver's stream.  The
// solver is only read: no field of it is written, nothing is launched that writes its buffers.
int smk_solver_residual(smk_solver* s, double* resid_sq, double* a_sq, double* col_resid_sq)
{
    if (!s) { set_error("smk_solver_residual: null solver"); return SMK_BAD_PARAM; }
    int rc = residual_args("smk_solver_residual", s->a, s->k, s->Wt, s->H, resid_sq, a_sq);
    if (rc) return rc;
    if (s->ex.ar || s->ex.comm) { set_error("smk_solver_residual: not available on a solver with a communicator"); return SMK_UNSUPPORTED; }
    if (!s->have_factors) { set_error("smk_solver_residual: the solver has no factors yet"); return SMK_BAD_PARAM; }
    Entry e(s->st);
    return residual_from_views(e, s->a, s->k, DeviceView::rows(s->Wt, s->KP), DeviceView::cols(s->H, s->KP), resid_sq, a_sq, nullptr, col_resid_sq);
}

}  // extern "C"
