// smallk_amd/csrc/kl.cpp -- NMF of a resident sparse matrix under the generalised Kullback-Leibler divergence by multiplicative
// updates (include/smallk_amd.h: smk_nmf_kl_device, smk_matrix_kl_divergence_device): scikit-learn's solver="mu",
// beta_loss="kullback-leibler".  A driver by itself, beside the solver's schedules and beside cd.cpp: each half-iteration is one
// sweep of kl.hip over the stored entries (CSC(A) for H, CSC(A') for W), the denominators are the row sums of the other factor.
// The entries are synchronous; every workspace and local segment plan belongs to the smk::Entry local of the entry (entry.h:
// synchronised before it releases them, on every path); of the matrix handle only the once-per-matrix records are written
// (segment plans, duplicate record, sign record).  W and H are written once, at the end: on any error they are untouched.
#include "entry.h"

#include <cmath>
#include <mutex>
#include <string>

namespace smk {

struct KlRun {
    const smk_matrix* a = nullptr;
    FactorPair f;                                 // the factors: Wt KP x m and H KP x n, k, KP, the stream
    const SegPlan *spA = nullptr, *spAt = nullptr;
    double *sumsW = nullptr, *sumsH = nullptr, *part = nullptr, *piecesA = nullptr, *piecesAt = nullptr, *divpart = nullptr, *out4 = nullptr;
    double* pin = nullptr;                        // the pinned slot the host reads the divergence from (4 doubles)
    int entry_passes = 0, divergence_passes = 0;
    KlRun(const smk_matrix* a_, int k) : a(a_), f{a_->m, a_->n, k, kp_of(k), matrix_stream(a_)} {}
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

static int kl_plans(KlRun& r, Entry& e)
{
    const int rc = seg_plan_or_local(r.a, false, e.st, &e.planA, &r.spA);
    return rc ? rc : seg_plan_or_local(r.a, true, e.st, &e.planAt, &r.spAt);
}

// the plans, the sums' and the sweeps' scratch, the zeroed factor workspaces and the views converted in
static int kl_setup(KlRun& r, Entry& e, bool sweeps, const DeviceView& W, const DeviceView& H, const std::string& who)
{
    Owned& own = e.own;
    const int KP = r.f.KP;
    const i64 nmax = r.a->m > r.a->n ? r.a->m : r.a->n;
    int rc = kl_plans(r, e);
    if (rc) return rc;
    rc = own.dev(&r.sumsW, (size_t)KP);
    if (!rc) rc = own.dev(&r.sumsH, (size_t)KP);
    if (!rc) rc = own.dev(&r.part, (size_t)kl_sums_blocks(nmax) * KP);
    if (!rc) rc = own.dev(&r.divpart, (size_t)2 * (r.spA->nseg > 0 ? r.spA->nseg : 1));
    if (!rc) rc = own.dev(&r.out4, 4);
    if (!rc) rc = own.pinned((void**)&r.pin, 4 * sizeof(double));
    if (!rc && sweeps && r.spA->npieces > 0) rc = own.dev(&r.piecesA, (size_t)r.spA->npieces * KP);
    if (!rc && sweeps && r.spAt->npieces > 0) rc = own.dev(&r.piecesAt, (size_t)r.spAt->npieces * KP);
    if (rc) { set_error(who + ": no memory for the factor workspace"); return SMK_DEVICE_ERROR; }
    rc = r.f.alloc_zeroed(own, who);
    return rc ? rc : r.f.load(W, H);
}

static int kl_sums_w(KlRun& r) { return launch_kl_factor_sums(r.f.Wt, r.f.k, r.a->m, r.part, r.sumsW, r.f.st); }
static int kl_sums_h(KlRun& r) { return launch_kl_factor_sums(r.f.H, r.f.k, r.a->n, r.part, r.sumsH, r.f.st); }

// out[0 .. 3] = D, sum a log(a / d), sum WH, sum a of the current factors (their row sums in place), through the pinned slot: one
// synchronisation
static int kl_divergence(KlRun& r, double* out)
{
    ++r.divergence_passes;
    const int rc = launch_kl_divergence(*r.spA, r.a->colptr, r.a->val, r.f.Wt, r.f.H, r.f.k, r.sumsW, r.sumsH, r.divpart, r.out4, r.pin, r.f.st);
    if (rc) return rc;
    SMK_HIP(hipStreamSynchronize(r.f.st));
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
    const FactorPair& f = r.f;
    const Penalties p(a->m, a->n, o.alpha_w, o.alpha_h, o.l1_ratio);
    int rc = kl_sums_w(r);                      // update_w = 0: formed once
    if (!rc) rc = kl_sums_h(r);
    double error_init = 0.0;
    if (!rc) rc = kl_error(r, &error_init);
    if (rc) return rc;
    double previous = error_init, error = error_init;
    int checked = 0, it = 0, converged = 0;
    for (it = 1; it <= o.max_iter; ++it) {
        ++r.entry_passes;
        rc = launch_kl_step(*r.spA, a->colptr, a->val, f.Wt, f.H, f.k, r.sumsW, 0, p.l1h, p.l2h, 0, r.piecesA, f.st);
        if (!rc && o.update_w) {
            rc = kl_sums_h(r);
            ++r.entry_passes;
            if (!rc) rc = launch_kl_step(*r.spAt, a->colptr_t, a->val_t, f.H, f.Wt, f.k, r.sumsH, 1, p.l1w, p.l2w, 1, r.piecesAt, f.st);
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

// (what both entries check first: entry.h's kl_args, shared with kl_dense.cpp)
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
    rc = check_penalties(w, o->alpha_w, o->alpha_h, o->l1_ratio, o->tol, o->max_iter);
    if (!rc) rc = kl_supported(w, a, k);
    if (rc) return rc;
    KlRun r(a, k);
    const DeviceView vW{W, dtW, rsW, csW}, vH{H, dtH, rsH, csH};
    rc = r.f.check(w, vW, vH, o->update_w != 0, true);
    if (rc) return rc;
    Entry e(r.f.st);
    rc = e.join(stream);
    if (!rc) rc = kl_setup(r, e, true, vW, vH, w);
    smk_kl_stats st{};
    if (!rc) rc = kl_loop(r, *o, &st);
    g_kl_entry_passes = r.entry_passes;
    g_kl_divergence_passes = r.divergence_passes;
    if (!rc) rc = r.f.store(o->update_w ? &vW : nullptr, &vH);
    if (!rc) rc = e.sync();
    if (rc) return rc;
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
    KlRun r(a, k);
    const DeviceView vW = DeviceView::in(W, dtW, rsW, csW), vH = DeviceView::in(H, dtH, rsH, csH);
    rc = r.f.check(w, vW, vH, false, false);
    if (rc) return rc;
    Entry e(r.f.st);
    rc = e.join(stream);
    if (!rc) rc = kl_setup(r, e, false, vW, vH, w);
    if (!rc) rc = kl_sums_w(r);
    if (!rc) rc = kl_sums_h(r);
    double d[4] = {0.0, 0.0, 0.0, 0.0};
    if (!rc) rc = e.synced(kl_divergence(r, d));
    if (rc) return rc;
    out[0] = d[0];
    out[1] = d[1];
    out[2] = d[2];
    return SMK_OK;
}

int smk_kl_step_time(const smk_matrix* a, int which, int k, int reps, double* ms)
{
    const std::string w("smk_kl_step_time");
    if (int rc = require_init()) return rc;
    if (!a || !ms || which < 0 || which > 3 || k < 1 || reps < 1) { set_error(w + ": bad argument"); return SMK_BAD_PARAM; }
    int rc = kl_supported(w, a, k);
    if (rc) return rc;
    KlRun r(a, k);
    Entry e(r.f.st);
    Owned& own = e.own;
    const hipStream_t st = e.st;
    const int KP = r.f.KP;
    rc = kl_plans(r, e);
    if (rc) return rc;
    const bool over_rows = which == 1 || which == 3;          // the W side: CSC(A'), H gathered
    const SegPlan& sp = over_rows ? *r.spAt : *r.spA;
    const i64 ng = over_rows ? a->n : a->m, nx = over_rows ? a->m : a->n;
    const i64* colptr = over_rows ? a->colptr_t : a->colptr;
    const double* val = over_rows ? a->val_t : a->val;
    double *G = nullptr, *X = nullptr, *sums = nullptr, *part = nullptr, *pieces = nullptr;
    rc = own.dev(&G, (size_t)KP * ng);
    if (!rc) rc = own.dev(&X, (size_t)KP * nx);
    if (!rc) rc = own.dev(&sums, (size_t)KP);
    if (!rc) rc = own.dev(&part, (size_t)kl_sums_blocks(ng) * KP);
    if (!rc) rc = own.dev(&pieces, (size_t)(sp.npieces > 0 ? sp.npieces : 1) * 128);
    if (rc) { set_error(w + ": no device memory"); return SMK_DEVICE_ERROR; }
    rc = launch_fill_factor_uniform(G, k, ng, 11, 0, st);
    if (!rc) rc = launch_fill_factor_uniform(X, k, nx, 12, 0, st);
    if (!rc) rc = launch_kl_factor_sums(G, k, ng, part, sums, st);
    if (rc) return rc;
    return e.synced(time_launches(w, own, st, reps, [&]() -> int {
        if (which <= 1) return launch_kl_step(sp, colptr, val, G, X, k, sums, which, 0.0, 0.0, which, pieces, st);
        const int prc = launch_spmm_seg(sp, colptr, val, G, k, X, KP, st, pieces);
        return prc < 0 ? prc : 0;
    }, ms));
}

int smk_kl_last_profile(int* entry_passes, int* divergence_passes)
{
    if (entry_passes) *entry_passes = g_kl_entry_passes;
    if (divergence_passes) *divergence_passes = g_kl_divergence_passes;
    return SMK_OK;
}

}  // extern "C"
