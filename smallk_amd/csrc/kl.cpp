// smallk_amd/csrc/kl.cpp -- NMF of a resident sparse matrix under the generalised Kullback-Leibler divergence by multiplicative
// updates (include/smallk_amd.h: smk_nmf_kl_device, smk_matrix_kl_divergence_device): scikit-learn's solver="mu",
// beta_loss="kullback-leibler".  A driver by itself, beside the solver's schedules and beside cd.cpp: each half-iteration is one
// sweep of kl.hip over the stored entries (CSC(A) for H, CSC(A') for W), the denominators are the row sums of the other factor.
// The entries are synchronous; every workspace belongs to an smk::Owned local of the entry and is released on every path; of the
// matrix handle only the once-per-matrix records are written (segment plans, duplicate record, sign record).  W and H are written
// once, at the end: on any error they are untouched.
#include "state.h"

#include <cmath>
#include <mutex>
#include <string>

namespace smk {

struct KlRun {
    const smk_matrix* a = nullptr;
    int k = 0, KP = 0;
    hipStream_t st = nullptr;
    const SegPlan *spA = nullptr, *spAt = nullptr;
    SegPlan localA, localAt;                      // a matrix without plans (SMK_SPMM_SEG=0) gets them for this call
    double *Wt = nullptr, *H = nullptr;           // the factors: KP x m and KP x n
    double *sumsW = nullptr, *sumsH = nullptr, *part = nullptr, *piecesA = nullptr, *piecesAt = nullptr, *divpart = nullptr, *out4 = nullptr;
    double* pin = nullptr;                        // the pinned slot the host reads the divergence from (4 doubles)
    int entry_passes = 0, divergence_passes = 0;
    ~KlRun() { free_seg_plan(&localA); free_seg_plan(&localAt); }
};

// the last run of the calling thread (smk_kl_last_profile)
static thread_local int g_kl_entry_passes = 0, g_kl_divergence_passes = 0;

// What the divergence asks of the stored values, looked up once per matrix: no entry stored twice (KL is not linear in a: the
// duplicates of an entry cannot be treated one by one) and no negative value.
static int kl_matrix_checks(const smk_matrix* a, const std::string& w)
{
    int rc = ensure_dup_record(a);
    if (rc) return rc;
    if (a->dup_state == 1) { set_error(w + ": the matrix stores an entry twice; merge duplicates first"); return SMK_UNSUPPORTED; }
    {
        static std::mutex mu;             // lazily built part of a shared, nominally const matrix (as ensure_dup_record)
        std::lock_guard<std::mutex> lk(mu);
        if (a->kl_negative < 0) {
            int neg = 0;
            for (double v : a->h_val) if (v < 0.0) { neg = 1; break; }      // (the host copy: ensure_dup_record fetched it)
            a->kl_negative = neg;
        }
    }
    if (a->kl_negative == 1) { set_error(w + ": the matrix stores a negative value"); return SMK_BAD_PARAM; }
    return 0;
}

static int kl_plans(KlRun& r)
{
    const smk_matrix* a = r.a;
    ensure_seg_plans(a);
    r.spA = &a->segA;
    r.spAt = &a->segAt;
    if (!r.spA->rowflag || r.spA->ncols != a->n) {
        const int rc = build_seg_plan(a->n, a->nnz, a->colptr, a->rowidx, &r.localA, r.st);
        if (rc) return rc;
        r.spA = &r.localA;
    }
    if (!r.spAt->rowflag || r.spAt->ncols != a->m) {
        const int rc = build_seg_plan(a->m, a->nnz, a->colptr_t, a->rowidx_t, &r.localAt, r.st);
        if (rc) return rc;
        r.spAt = &r.localAt;
    }
    return 0;
}

// the zeroed factor workspaces (pad rows of the resident layout are zeros), the views converted in, the sums' and the sweeps' scratch
static int kl_setup(KlRun& r, Owned& own, bool sweeps, const void* W, int dtW, i64 rsW, i64 csW, const void* H, int dtH, i64 rsH, i64 csH,
                    const char* who)
{
    const smk_matrix* a = r.a;
    const i64 nmax = a->m > a->n ? a->m : a->n;
    int rc = kl_plans(r);
    if (rc) return rc;
    rc = own.dev(&r.Wt, (size_t)r.KP * a->m);
    if (!rc) rc = own.dev(&r.H, (size_t)r.KP * a->n);
    if (!rc) rc = own.dev(&r.sumsW, (size_t)r.KP);
    if (!rc) rc = own.dev(&r.sumsH, (size_t)r.KP);
    if (!rc) rc = own.dev(&r.part, (size_t)kl_sums_blocks(nmax) * r.KP);
    if (!rc) rc = own.dev(&r.divpart, (size_t)2 * (r.spA->nseg > 0 ? r.spA->nseg : 1));
    if (!rc) rc = own.dev(&r.out4, 4);
    if (!rc) rc = own.pinned((void**)&r.pin, 4 * sizeof(double));
    if (!rc && sweeps && r.spA->npieces > 0) rc = own.dev(&r.piecesA, (size_t)r.spA->npieces * r.KP);
    if (!rc && sweeps && r.spAt->npieces > 0) rc = own.dev(&r.piecesAt, (size_t)r.spAt->npieces * r.KP);
    if (rc) { set_error(std::string(who) + ": no memory for the factor workspace"); return SMK_DEVICE_ERROR; }
    SMK_HIP(hipMemsetAsync(r.Wt, 0, (size_t)r.KP * a->m * sizeof(double), r.st));
    SMK_HIP(hipMemsetAsync(r.H, 0, (size_t)r.KP * a->n * sizeof(double), r.st));
    rc = launch_strided_convert(W, dtW, rsW, csW, r.Wt, DT_F64, r.KP, 1, a->m, r.k, r.st);
    if (!rc) rc = launch_strided_convert(H, dtH, rsH, csH, r.H, DT_F64, 1, r.KP, r.k, a->n, r.st);
    return rc;
}

static int kl_sums_w(KlRun& r) { return launch_kl_factor_sums(r.Wt, r.k, r.a->m, r.part, r.sumsW, r.st); }
static int kl_sums_h(KlRun& r) { return launch_kl_factor_sums(r.H, r.k, r.a->n, r.part, r.sumsH, r.st); }

// out[0 .. 3] = D, sum a log(a / d), sum WH, sum a of the current factors (their row sums in place), through the pinned slot: one
// synchronisation
static int kl_divergence(KlRun& r, double* out)
{
    ++r.divergence_passes;
    const int rc = launch_kl_divergence(*r.spA, r.a->colptr, r.a->val, r.Wt, r.H, r.k, r.sumsW, r.sumsH, r.divpart, r.out4, r.pin, r.st);
    if (rc) return rc;
    SMK_HIP(hipStreamSynchronize(r.st));
    for (int i = 0; i < 4; ++i) out[i] = r.pin[i];
    return 0;
}

static int kl_error(KlRun& r, double* err)
{
    double d[4];
    const int rc = kl_divergence(r, d);
    if (rc) return rc;
    *err = std::sqrt(2.0 * (d[0] > 0.0 ? d[0] : 0.0));
    return 0;
}

static int kl_loop(KlRun& r, const smk_kl_options& o, smk_kl_stats* stats)
{
    const smk_matrix* a = r.a;
    const double m = (double)a->m, n = (double)a->n;
    const double l1h = m * o.alpha_h * o.l1_ratio, l2h = m * o.alpha_h * (1.0 - o.l1_ratio);
    const double l1w = n * o.alpha_w * o.l1_ratio, l2w = n * o.alpha_w * (1.0 - o.l1_ratio);
    int rc = kl_sums_w(r);                      // update_w = 0: formed once
    if (!rc) rc = kl_sums_h(r);
    double error_init = 0.0;
    if (!rc) rc = kl_error(r, &error_init);
    if (rc) return rc;
    double previous = error_init, error = error_init;
    int checked = 0, it = 0, converged = 0;
    for (it = 1; it <= o.max_iter; ++it) {
        ++r.entry_passes;
        rc = launch_kl_step(*r.spA, a->colptr, a->val, r.Wt, r.H, r.k, r.sumsW, 0, l1h, l2h, 0, r.piecesA, r.st);
        if (!rc && o.update_w) {
            rc = kl_sums_h(r);
            ++r.entry_passes;
            if (!rc) rc = launch_kl_step(*r.spAt, a->colptr_t, a->val_t, r.H, r.Wt, r.k, r.sumsH, 1, l1w, l2w, 1, r.piecesAt, r.st);
            if (!rc) rc = kl_sums_w(r);
        }
        if (rc) return rc;
        if (o.tol > 0.0 && it % 10 == 0) {
            if (!o.update_w) rc = kl_sums_h(r);
            if (!rc) rc = kl_error(r, &error);
            if (rc) return rc;
            checked = it;
            if ((previous - error) / error_init < o.tol) { converged = 1; break; }
            previous = error;
        }
    }
    if (it > o.max_iter) it = o.max_iter;
    if (checked != it) {                        // the error of the factors that go back
        if (!o.update_w) rc = kl_sums_h(r);
        if (!rc) rc = kl_error(r, &error);
        if (rc) return rc;
    }
    stats->iterations = it;
    stats->converged = converged;
    stats->error_init = error_init;
    stats->error = error;
    return 0;
}

static bool kl_dtype(int dt) { return dt == SMK_DT_F64 || dt == SMK_DT_F32; }

// what both entries check first
static int kl_args(const std::string& w, const smk_matrix* a, int k, const void* W, int dtW, const void* H, int dtH)
{
    if (!ctx().init) { set_error("smk_initialize() has not been called"); return SMK_NOTINITIALIZED; }
    if (!a || !W || !H) { set_error(w + ": null argument"); return SMK_BAD_PARAM; }
    if (k < 1) { set_error(w + ": k < 1"); return SMK_BAD_PARAM; }
    if (k > a->m || k > a->n_global) { set_error(w + ": k exceeds min(m, n)"); return SMK_BAD_PARAM; }
    if (!kl_dtype(dtW) || !kl_dtype(dtH)) { set_error(w + ": W and H are fp64 or fp32"); return SMK_BAD_PARAM; }
    return 0;
}

static int kl_supported(const std::string& w, const smk_matrix* a, int k)
{
    if (k > 128) { set_error(w + ": k > 128 is not supported yet"); return SMK_UNSUPPORTED; }
    if (a->n != a->n_global) { set_error(w + ": not available on a column shard"); return SMK_UNSUPPORTED; }
    if (!a->sparse) { set_error(w + ": the Kullback-Leibler path takes a sparse matrix"); return SMK_UNSUPPORTED; }
    return kl_matrix_checks(a, w);
}

}  // namespace smk

extern "C" {

int smk_nmf_kl_device(const smk_matrix* a, int k, const smk_kl_options* o, void* W, int dtW, int64_t rsW, int64_t csW, void* H, int dtH,
                      int64_t rsH, int64_t csH, void* stream, smk_kl_stats* stats)
{
    const std::string w("smk_nmf_kl_device");
    int rc = kl_args(w, a, k, W, dtW, H, dtH);
    if (rc) return rc;
    if (!o || !stats) { set_error(w + ": null argument"); return SMK_BAD_PARAM; }
    if (!(o->alpha_w >= 0.0) || !(o->alpha_h >= 0.0)) { set_error(w + ": alpha_w and alpha_h must be >= 0"); return SMK_BAD_PARAM; }
    if (!(o->l1_ratio >= 0.0 && o->l1_ratio <= 1.0)) { set_error(w + ": l1_ratio must lie in [0, 1]"); return SMK_BAD_PARAM; }
    if (!(o->tol >= 0.0)) { set_error(w + ": tol must be >= 0"); return SMK_BAD_PARAM; }
    if (o->max_iter < 1) { set_error(w + ": max_iter < 1"); return SMK_BAD_PARAM; }
    rc = kl_supported(w, a, k);
    if (rc) return rc;
    rc = check_device_view(W, dtW, a->m, k, rsW, csW, o->update_w != 0, "smk_nmf_kl_device(W)");
    if (!rc) rc = check_device_view(H, dtH, k, a->n, rsH, csH, true, "smk_nmf_kl_device(H)");
    if (rc) return rc;
    Owned own;
    KlRun r;
    r.a = a;
    r.k = k;
    r.KP = kp_of(k);
    r.st = a->st ? a->st : ctx().stream;
    rc = join_caller_stream(own, r.st, stream);
    if (!rc) rc = kl_setup(r, own, true, W, dtW, rsW, csW, H, dtH, rsH, csH, "smk_nmf_kl_device");
    smk_kl_stats st{};
    if (!rc) rc = kl_loop(r, *o, &st);
    g_kl_entry_passes = r.entry_passes;
    g_kl_divergence_passes = r.divergence_passes;
    if (!rc && o->update_w) rc = launch_strided_convert(r.Wt, DT_F64, r.KP, 1, W, dtW, rsW, csW, a->m, k, r.st);
    if (!rc) rc = launch_strided_convert(r.H, DT_F64, 1, r.KP, H, dtH, rsH, csH, k, a->n, r.st);
    if (rc) { (void)hipStreamSynchronize(r.st); return rc; }        // the local plans are freed on return
    SMK_HIP(hipStreamSynchronize(r.st));
    *stats = st;
    return SMK_OK;
}

int smk_matrix_kl_divergence_device(const smk_matrix* a, int k, const void* W, int dtW, int64_t rsW, int64_t csW, const void* H, int dtH,
                                    int64_t rsH, int64_t csH, void* stream, double* out)
{
    const std::string w("smk_matrix_kl_divergence_device");
    int rc = kl_args(w, a, k, W, dtW, H, dtH);
    if (rc) return rc;
    if (!out) { set_error(w + ": null output"); return SMK_BAD_PARAM; }
    rc = kl_supported(w, a, k);
    if (rc) return rc;
    rc = check_device_view(W, dtW, a->m, k, rsW, csW, false, "smk_matrix_kl_divergence_device(W)");
    if (!rc) rc = check_device_view(H, dtH, k, a->n, rsH, csH, false, "smk_matrix_kl_divergence_device(H)");
    if (rc) return rc;
    Owned own;
    KlRun r;
    r.a = a;
    r.k = k;
    r.KP = kp_of(k);
    r.st = a->st ? a->st : ctx().stream;
    rc = join_caller_stream(own, r.st, stream);
    if (!rc) rc = kl_setup(r, own, false, W, dtW, rsW, csW, H, dtH, rsH, csH, "smk_matrix_kl_divergence_device");
    if (!rc) rc = kl_sums_w(r);
    if (!rc) rc = kl_sums_h(r);
    double d[4] = {0.0, 0.0, 0.0, 0.0};
    if (!rc) rc = kl_divergence(r, d);
    if (rc) { (void)hipStreamSynchronize(r.st); return rc; }
    out[0] = d[0];
    out[1] = d[1];
    out[2] = d[2];
    return SMK_OK;
}

int smk_kl_step_time(const smk_matrix* a, int which, int k, int reps, double* ms)
{
    const std::string w("smk_kl_step_time");
    if (!ctx().init) { set_error("smk_initialize() has not been called"); return SMK_NOTINITIALIZED; }
    if (!a || !ms || which < 0 || which > 3 || k < 1 || reps < 1) { set_error(w + ": bad argument"); return SMK_BAD_PARAM; }
    int rc = kl_supported(w, a, k);
    if (rc) return rc;
    Owned own;
    KlRun r;
    r.a = a;
    r.k = k;
    r.KP = kp_of(k);
    r.st = a->st ? a->st : ctx().stream;
    rc = kl_plans(r);
    if (rc) return rc;
    const bool over_rows = which == 1 || which == 3;          // the W side: CSC(A'), H gathered
    const SegPlan& sp = over_rows ? *r.spAt : *r.spA;
    const i64 ng = over_rows ? a->n : a->m, nx = over_rows ? a->m : a->n;
    const i64* colptr = over_rows ? a->colptr_t : a->colptr;
    const double* val = over_rows ? a->val_t : a->val;
    double *G = nullptr, *X = nullptr, *sums = nullptr, *part = nullptr, *pieces = nullptr;
    hipEvent_t e0 = nullptr, e1 = nullptr;
    rc = own.dev(&G, (size_t)r.KP * ng);
    if (!rc) rc = own.dev(&X, (size_t)r.KP * nx);
    if (!rc) rc = own.dev(&sums, (size_t)r.KP);
    if (!rc) rc = own.dev(&part, (size_t)kl_sums_blocks(ng) * r.KP);
    if (!rc) rc = own.dev(&pieces, (size_t)(sp.npieces > 0 ? sp.npieces : 1) * 128);
    if (!rc) rc = own.event(&e0, hipEventDefault);
    if (!rc) rc = own.event(&e1, hipEventDefault);
    if (rc) { set_error(w + ": no device memory"); return SMK_DEVICE_ERROR; }
    rc = launch_fill_factor_uniform(G, k, ng, 11, 0, r.st);
    if (!rc) rc = launch_fill_factor_uniform(X, k, nx, 12, 0, r.st);
    if (!rc) rc = launch_kl_factor_sums(G, k, ng, part, sums, r.st);
    auto once = [&]() -> int {
        if (which <= 1) return launch_kl_step(sp, colptr, val, G, X, k, sums, which, 0.0, 0.0, which, pieces, r.st);
        const int prc = launch_spmm_seg(sp, colptr, val, G, k, X, r.KP, r.st, pieces);
        return prc < 0 ? prc : 0;
    };
    for (int i = 0; i < 3 && !rc; ++i) rc = once();         // warm-up: the code object
    if (!rc && hipEventRecord(e0, r.st) != hipSuccess) rc = SMK_DEVICE_ERROR;
    for (int i = 0; i < reps && !rc; ++i) rc = once();
    if (!rc && hipEventRecord(e1, r.st) != hipSuccess) rc = SMK_DEVICE_ERROR;
    (void)hipStreamSynchronize(r.st);                       // the local plans are freed on return
    if (rc) return rc;
    float t = 0.f;
    SMK_HIP(hipEventElapsedTime(&t, e0, e1));
    *ms = (double)t / reps;
    return SMK_OK;
}

int smk_kl_last_profile(int* entry_passes, int* divergence_passes)
{
    if (entry_passes) *entry_passes = g_kl_entry_passes;
    if (divergence_passes) *divergence_passes = g_kl_divergence_passes;
    return SMK_OK;
}

}  // extern "C"
