// smallk_amd/csrc/factors.cpp -- the factors on their way into and out of a solver: every smk_solver_set_factors* (host arrays,
// views in device memory, the uniform fill on the device), every smk_solver_get_factors*, and the labels and top terms read
// straight from the resident factors.  What the ways in share is factors_begin / factors_end, what the ways out share is
// factors_ready; solver.cpp lends gather_w, normalize_device and sync_and_check.
#include "solver_internal.h"
#include "entry.h"

#include <algorithm>
#include <climits>
#include <vector>

namespace smk {

// What every way of setting the factors shares.  Before the factors are written: a matrix refilled after this solver was created
// has its fp16 product scale and its norms measured again.  After: the failure flag, the copies of the start, this rank's blocks
// of a row-sharded W, the state of a fresh run.
static int factors_begin(smk_solver* s)
{
    if (s->nsplit == NSPLIT_F16X2 && (s->a->ascale == 0.f || s->a->ascale != s->pg1[0].ascale)) {
        // the matrix was refilled after this solver was created: its fp16 product scale follows the new contents
        if (s->a->ascale == 0.f) { const int rc0 = matrix_measure_scale(s->a, s->st); if (rc0) return rc0; }
        for (int g = 0; g < s->ng; ++g) s->pg1[g].ascale = s->pg2[g].ascale = s->a->ascale;
        s->pl1.ascale = s->pl2.ascale = s->a->ascale;
    }
    if (s->pack_in_solve && (s->a->colnorm_max < 0.0 || s->a->rownorm_max < 0.0)) {      // ... and so do the norms behind the packing NNLS launch
        const int rc0 = matrix_measure_norms(s->a, s->st);
        if (rc0) return rc0;
    }
    return 0;
}

static int factors_end(smk_solver* s)
{
    const int big = INT_MAX;
    SMK_HIP(hipMemcpyAsync(s->fail_flag, &big, sizeof(int), hipMemcpyHostToDevice, s->st));
    if (s->W0c) {
        SMK_HIP(hipMemcpyAsync(s->W0c, s->Wt, (size_t)s->KP * s->m * sizeof(double), hipMemcpyDeviceToDevice, s->st));
        SMK_HIP(hipMemcpyAsync(s->H0c, s->H, (size_t)s->KP * s->n * sizeof(double), hipMemcpyDeviceToDevice, s->st));
    }
    if (s->ex.w_sharded) { const int rc = scatter_own(s); if (rc) return rc; }
    SMK_HIP(hipStreamSynchronize(s->st));
    s->ex.w_full = true;
    s->wc_valid = false;
    s->have_factors = true;
    s->inited = false;
    s->normalized = false;
    s->iter = 0;
    s->pc.reset_estimator();
    return SMK_OK;
}

// the solver's resident factors as the pair the view entries convert into and out of (entry.h): buffers the pair does not own
static FactorPair resident_pair(const smk_solver* s) { return {s->m, s->n, s->k, s->KP, s->st, s->Wt, s->H}; }

// what every way of reading the factors does first
static int factors_ready(smk_solver* s, int normalize)
{
    int rc = gather_w(s);                 // a collective when W is row-sharded and stale: every rank must be here
    if (rc) return rc;
    if (normalize) { rc = normalize_device(s); if (rc) return rc; }
    return 0;
}

}  // namespace smk

extern "C" {

int smk_solver_set_factors(smk_solver* s, const double* W0, int64_t ldW, const double* H0, int64_t ldH)
{
    if (!s || !W0 || !H0) return SMK_BAD_PARAM;
    if (ldW < s->m || ldH < s->k) { set_error("leading dimension too small"); return SMK_BAD_PARAM; }
    int rc = factors_begin(s);
    if (!rc) rc = resident_pair(s).zero();
    if (rc) return rc;
    // W0 (m x k, host) -> tmpW (m x k, ld m) -> Wt (KP x m)
    SMK_HIP(hipMemcpy2DAsync(s->tmpW, (size_t)s->m * sizeof(double), W0, (size_t)ldW * sizeof(double),
                             (size_t)s->m * sizeof(double), (size_t)s->k, hipMemcpyHostToDevice, s->st));
    rc = launch_transpose_f64(s->tmpW, s->m, s->Wt, s->KP, s->m, s->k, s->st);
    if (rc) return rc;
    SMK_HIP(hipMemcpy2DAsync(s->H, (size_t)s->KP * sizeof(double), H0, (size_t)ldH * sizeof(double),
                             (size_t)s->k * sizeof(double), (size_t)s->n, hipMemcpyHostToDevice, s->st));
    return factors_end(s);
}

// The same start from views in device memory (a torch tensor's data_ptr and strides): W0 is m x k, H0 is k x n.  The strided
// convert kernel writes Wt (KP x m) and H (KP x n) directly -- a row-major W0 already has the layout of Wt with pitch k instead
// of KP, so it is a straight copy, with no pass through tmpW.
int smk_solver_set_factors_device(smk_solver* s, const void* W0, int dtypeW, int64_t rsW, int64_t csW, const void* H0, int dtypeH,
                                  int64_t rsH, int64_t csH, void* stream)
{
    const char* who = "smk_solver_set_factors_device";
    if (!s) return SMK_BAD_PARAM;
    const FactorPair f = resident_pair(s);
    const DeviceView vW = DeviceView::in(W0, dtypeW, rsW, csW), vH = DeviceView::in(H0, dtypeH, rsH, csH);
    int rc = check_factor_dtypes(who, "factors", dtypeW, dtypeH);
    if (!rc) rc = f.check(who, vW, vH, false, false, "W0", "H0");
    if (rc) return rc;
    Entry e(s->st);
    rc = e.join(stream);
    if (!rc) rc = factors_begin(s);
    if (!rc) rc = f.zero();
    if (!rc) rc = f.load(vW, vH);
    if (rc) return rc;
    return e.synced(factors_end(s));
}

// The same start as smk_solver_set_factors(W0, H0) with W0 = smk_uniform_fill_host(m x k, seed_w), H0 = smk_uniform_fill_host
// (k x n, seed_h) -- the RandomMatrix stand-in of every caller in this library -- generated on the device: no host fill, no
// upload.  (HierNMF2 draws two such matrices per node.)  Unsharded solvers only.
int smk_solver_set_factors_uniform(smk_solver* s, uint64_t seed_w, uint64_t seed_h)
{
    if (!s) return SMK_BAD_PARAM;
    if (is_dist(s) || s->ex.comm) { set_error("set_factors_uniform: not for sharded solvers"); return SMK_UNSUPPORTED; }
    int rc = factors_begin(s);
    if (!rc) rc = launch_fill_factor_uniform(s->Wt, s->k, s->m, seed_w, 1, s->st);
    if (!rc) rc = launch_fill_factor_uniform(s->H, s->k, s->n, seed_h, 0, s->st);
    if (rc) return rc;
    return factors_end(s);       // never row-sharded here
}

// ... into views in device memory: W (m x k) from Wt, H (k x n) from the first k rows of the resident H, converted in flight
int smk_solver_get_factors_device(smk_solver* s, int normalize, void* W, int dtypeW, int64_t rsW, int64_t csW, void* H, int dtypeH,
                                  int64_t rsH, int64_t csH, void* stream)
{
    const char* who = "smk_solver_get_factors_device";
    if (!s) return SMK_BAD_PARAM;
    const DeviceView vW{W, dtypeW, rsW, csW}, vH{H, dtypeH, rsH, csH};
    int rc = check_factor_dtypes(who, "factors", dtypeW, dtypeH);
    if (!rc) rc = resident_pair(s).check(who, vW, vH, true, true);
    if (rc) return rc;
    Entry e(s->st);
    rc = e.join(stream);
    if (!rc) rc = factors_ready(s, normalize);
    if (!rc) rc = resident_pair(s).store(&vW, &vH);
    if (rc) return rc;
    return e.synced(sync_and_check(s, nullptr));
}

// Labels / memberships of the local columns and the top terms of the topics, straight from the resident factors (H at H + c KP,
// W as Wt + i KP: the k-contiguous layout the kernels of assign.hip read; the pad rows are never candidates).  normalize as in
// smk_solver_get_factors; the solver is otherwise left exactly as it was.
int smk_solver_labels(smk_solver* s, int normalize, void* stream, void* labels, void* memberships)
{
    if (!s) { set_error("smk_solver_labels: null solver"); return SMK_BAD_PARAM; }
    if (!s->have_factors) { set_error("smk_solver_labels: the solver has no factors yet"); return SMK_BAD_PARAM; }
    if (!labels) { set_error("smk_solver_labels: null output"); return SMK_BAD_PARAM; }
    int rc = check_device_view(labels, DT_F32, s->n, 1, 1, s->n, true, "smk_solver_labels(labels)");       // 32-bit integers
    if (!rc && memberships) rc = check_device_view(memberships, DT_F32, s->k, s->n, 1, s->k, true, "smk_solver_labels(memberships)");
    if (rc) return rc;
    Owned own;
    rc = join_caller_stream(own, s->st, stream);
    if (!rc) rc = factors_ready(s, normalize);
    if (rc) return rc;
    return labels_from_view(s->H, DT_F64, 1, s->KP, s->k, s->n, s->st, own, labels, memberships);
}

int smk_solver_top_terms(smk_solver* s, int normalize, int maxterms, void* stream, void* term_indices)
{
    if (!s) { set_error("smk_solver_top_terms: null solver"); return SMK_BAD_PARAM; }
    if (!s->have_factors) { set_error("smk_solver_top_terms: the solver has no factors yet"); return SMK_BAD_PARAM; }
    if (maxterms < 1) { set_error("smk_solver_top_terms: maxterms < 1"); return SMK_BAD_PARAM; }
    if (!term_indices) { set_error("smk_solver_top_terms: null output"); return SMK_BAD_PARAM; }
    int rc = check_device_view(term_indices, DT_F32, maxterms, s->k, 1, maxterms, true, "smk_solver_top_terms(term_indices)");
    if (rc) return rc;
    Owned own;
    rc = join_caller_stream(own, s->st, stream);
    if (!rc) rc = factors_ready(s, normalize);       // a row-sharded W is gathered here
    if (rc) return rc;
    return top_terms_from_view(s->Wt, DT_F64, s->KP, 1, s->m, s->k, maxterms, s->st, own, term_indices);
}

int smk_solver_get_factors(smk_solver* s, int normalize, double* W, int64_t ldW, double* H, int64_t ldH)
{
    if (!s || !W || !H) return SMK_BAD_PARAM;
    if (ldW < s->m || ldH < s->k) { set_error("leading dimension too small"); return SMK_BAD_PARAM; }
    int rc = factors_ready(s, normalize);
    if (rc) return rc;
    rc = launch_transpose_f64(s->Wt, s->KP, s->tmpW, s->m, s->k, s->m, s->st);
    if (rc) return rc;
    // Device-to-host copies are kept contiguous: a strided hipMemcpy2DAsync into pageable memory leaves
    // ~190 KiB of runtime staging behind per call on this ROCm (1200 one-shot sparse runs: 230 MiB).
    if (ldW == s->m) {
        SMK_HIP(hipMemcpyAsync(W, s->tmpW, (size_t)s->m * s->k * sizeof(double), hipMemcpyDeviceToHost, s->st));
    } else {
        for (int c = 0; c < s->k; ++c)
            SMK_HIP(hipMemcpyAsync(W + (size_t)c * ldW, s->tmpW + (size_t)c * s->m, (size_t)s->m * sizeof(double),
                                   hipMemcpyDeviceToHost, s->st));
    }
    if (s->k == s->KP && ldH == s->k) {
        SMK_HIP(hipMemcpyAsync(H, s->H, (size_t)s->k * s->n * sizeof(double), hipMemcpyDeviceToHost, s->st));
    } else {
        if (!s->tmpH) { rc = s->own.dev(&s->tmpH, (size_t)s->k * s->n); if (rc) return rc; }
        rc = launch_compact_rows(s->H, s->KP, s->tmpH, s->k, s->n, s->st);
        if (rc) return rc;
        if (ldH == s->k) {
            SMK_HIP(hipMemcpyAsync(H, s->tmpH, (size_t)s->k * s->n * sizeof(double), hipMemcpyDeviceToHost, s->st));
        } else {      // caller's leading dimension exceeds k: compact on the device, scatter on the host
            std::vector<double> tmp((size_t)s->k * s->n);
            SMK_HIP(hipMemcpyAsync(tmp.data(), s->tmpH, tmp.size() * sizeof(double), hipMemcpyDeviceToHost, s->st));
            SMK_HIP(hipStreamSynchronize(s->st));
            for (i64 c = 0; c < s->n; ++c)
                std::copy(tmp.begin() + c * s->k, tmp.begin() + (c + 1) * s->k, H + c * ldH);
        }
    }
    return sync_and_check(s, nullptr);
}

}  // extern "C"
