// smallk_amd/csrc/masked_cd.cpp -- NMF fitted to the stored entries of a resident sparse matrix only, by cyclic coordinate descent
// (include/smallk_amd.h: smk_nmf_masked_device, smk_matrix_masked_residual_device): an entry that is not stored is
// "not measured", not 0 -- ratings, missing wells, entries held out on purpose.  A driver by itself, beside cd.cpp and kl.cpp: each
// half-iteration is one sweep of masked_cd.hip over the stored entries (CSC(A) for H, CSC(A') for W), the violation leaves it as
// cd.cpp's does.  The entries are synchronous; every workspace and local segment plan belongs to the smk::Entry local of the entry
// (entry.h: synchronised before it releases them, on every path); of the matrix handle only the once-per-matrix records are written
// (segment plans, duplicate record).  W and H are written once, at the end: on any error they are untouched.
#include "entry.h"

#include <cmath>
#include <string>

namespace smk {

struct MaskedRun {
    const smk_matrix* a = nullptr;
    FactorPair f;                                 // the factors: Wt KP x m and H KP x n, k, KP, the stream
    const SegPlan *spA = nullptr, *spAt = nullptr;
    double *res = nullptr, *part = nullptr, *vdev = nullptr, *scratch = nullptr, *out3 = nullptr;
    double* pin = nullptr;                        // the pinned slots the host reads: [0] the violation, [1 .. 3] the residual's three numbers
    int entry_sweeps = 0, residual_sweeps = 0;
    MaskedRun(const smk_matrix* a_, int k) : a(a_), f{a_->m, a_->n, k, kp_of(k), matrix_stream(a_)} {}
};

// the last run of the calling thread (smk_masked_last_profile)
static thread_local int g_masked_entry_sweeps = 0, g_masked_residual_sweeps = 0;

// what both entries check after their arguments: a sparse matrix, whole, k <= 128, whose stored entries are a set
static int masked_supported(const std::string& w, const smk_matrix* a, int k)
{
    if (k > 128) { set_error(w + ": k > 128 is not supported yet"); return SMK_UNSUPPORTED; }
    if (a->n != a->n_global) { set_error(w + ": not available on a column shard"); return SMK_UNSUPPORTED; }
    if (!a->sparse) { set_error(w + ": the mask is the set of stored entries of a sparse matrix; a dense matrix has none"); return SMK_UNSUPPORTED; }
    if (spmm_seg_len() > masked_seg_len_max()) {          // a lane of the sweep holds four entries of a column: before any plan is built
        set_error(w + ": serves segments of at most " + std::to_string(masked_seg_len_max()) + " entries (SMK_SPMM_SEG_LEN)");
        return SMK_UNSUPPORTED;
    }
    const int rc = ensure_dup_record(a);
    if (rc) return rc;
    if (a->dup_state == 1) { set_error(w + ": the matrix stores an entry twice; merge duplicates first"); return SMK_UNSUPPORTED; }
    return SMK_OK;
}

// the plans of both copies
static int masked_plans(MaskedRun& r, Entry& e, bool both)
{
    const int rc = seg_plan_or_local(r.a, false, e.st, &e.planA, &r.spA);
    return rc || !both ? rc : seg_plan_or_local(r.a, true, e.st, &e.planAt, &r.spAt);
}

static int masked_setup(MaskedRun& r, Entry& e, bool sweeps, const DeviceView& W, const DeviceView& H, const std::string& who)
{
    Owned& own = e.own;
    int rc = masked_plans(r, e, sweeps);
    if (rc) return rc;
    rc = own.dev(&r.scratch, masked_residual_scratch_elems(*r.spA));
    if (!rc) rc = own.dev(&r.out3, 3);
    if (!rc) rc = own.pinned((void**)&r.pin, 4 * sizeof(double));
    if (!rc && sweeps) {
        rc = own.dev(&r.part, (size_t)masked_sweep_partials(*r.spA) + (size_t)masked_sweep_partials(*r.spAt) + 1);
        if (!rc) rc = own.dev(&r.vdev, 1);
        if (!rc && (r.spA->nlong > 0 || r.spAt->nlong > 0)) rc = own.dev(&r.res, (size_t)r.a->nnz);
    }
    if (rc) { set_error(who + ": no memory for the factor workspace"); return SMK_DEVICE_ERROR; }
    rc = r.f.alloc_zeroed(own, who);
    return rc ? rc : r.f.load(W, H);
}

// out[0 .. 2] = sum over the stored entries of (a - w_i . h_j)^2, of a^2, and their number, through the pinned slots: one synchronisation
static int masked_residual(MaskedRun& r, double* col_r, double* col_a, double* out)
{
    ++r.residual_sweeps;
    const int rc = launch_masked_residual(*r.spA, r.a->colptr, r.a->val, r.f.Wt, r.f.H, r.f.k, r.scratch, col_r, col_a, r.out3, r.pin + 1, r.f.st);
    if (rc) return rc;
    SMK_HIP(hipStreamSynchronize(r.f.st));
    for (int i = 0; i < 3; ++i) out[i] = r.pin[1 + i];
    return 0;
}

static int masked_loop(MaskedRun& r, const smk_cd_options& o, smk_masked_stats* stats)
{
    const smk_matrix* a = r.a;
    const FactorPair& f = r.f;
    const Penalties p(a->m, a->n, o.alpha_w, o.alpha_h, o.l1_ratio);
    const int nh = masked_sweep_partials(*r.spA), nw = masked_sweep_partials(*r.spAt);
    stats->iterations = 0;
    stats->converged = 0;
    stats->violation_init = stats->violation = stats->error = 0.0;
    for (int it = 1; it <= o.max_iter; ++it) {
        ++r.entry_sweeps;
        int rc = launch_masked_sweep(*r.spA, a->colptr, a->val, f.Wt, f.H, f.k, p.l1h, p.l2h, r.res, r.part, f.st);
        if (!rc && o.update_w) {
            ++r.entry_sweeps;
            rc = launch_masked_sweep(*r.spAt, a->colptr_t, a->val_t, f.H, f.Wt, f.k, p.l1w, p.l2w, r.res, r.part + nh, f.st);
        }
        if (!rc) rc = launch_cd_violation(r.part, o.update_w ? nh + nw : nh, r.vdev, r.pin, f.st);
        if (rc) return rc;
        SMK_HIP(hipStreamSynchronize(f.st));
        const double v = r.pin[0];
        stats->iterations = it;
        stats->violation = v;
        if (it == 1) stats->violation_init = v;
        if (stats->violation_init == 0.0 || v / stats->violation_init <= o.tol) { stats->converged = 1; break; }
    }
    double d[3];
    const int rc = masked_residual(r, nullptr, nullptr, d);      // the error of the factors that go back
    if (rc) return rc;
    stats->error = std::sqrt(d[0] > 0.0 ? d[0] : 0.0);
    return 0;
}

}  // namespace smk

extern "C" {

int smk_nmf_masked_device(const smk_matrix* a, int k, const smk_cd_options* o, void* W, int dtW, int64_t rsW, int64_t csW, void* H, int dtH,
                          int64_t rsH, int64_t csH, void* stream, smk_masked_stats* stats)
{
    const std::string w("smk_nmf_masked_device");
    int rc = kl_args(w, a, k, W, dtW, H, dtH);
    if (rc) return rc;
    if (!o || !stats) { set_error(w + ": null argument"); return SMK_BAD_PARAM; }
    rc = check_penalties(w, o->alpha_w, o->alpha_h, o->l1_ratio, o->tol, o->max_iter);
    if (!rc) rc = masked_supported(w, a, k);
    if (rc) return rc;
    MaskedRun r(a, k);
    const DeviceView vW{W, dtW, rsW, csW}, vH{H, dtH, rsH, csH};
    rc = r.f.check(w, vW, vH, o->update_w != 0, true);
    if (rc) return rc;
    Entry e(r.f.st);
    rc = e.join(stream);
    if (!rc) rc = masked_setup(r, e, true, vW, vH, w);
    smk_masked_stats st{};
    if (!rc) rc = masked_loop(r, *o, &st);
    g_masked_entry_sweeps = r.entry_sweeps;
    g_masked_residual_sweeps = r.residual_sweeps;
    if (!rc) rc = r.f.store(o->update_w ? &vW : nullptr, &vH);
    if (!rc) rc = e.sync();
    if (rc) return rc;
    *stats = st;
    return SMK_OK;
}

int smk_matrix_masked_residual_device(const smk_matrix* a, int k, const void* W, int dtW, int64_t rsW, int64_t csW, const void* H, int dtH,
                                      int64_t rsH, int64_t csH, double* col_r, double* col_a, void* stream, double* out3)
{
    const std::string w("smk_matrix_masked_residual_device");
    int rc = kl_args(w, a, k, W, dtW, H, dtH);
    if (rc) return rc;
    if (!out3) { set_error(w + ": null output"); return SMK_BAD_PARAM; }
    if ((col_r == nullptr) != (col_a == nullptr)) { set_error(w + ": both per-column outputs or neither"); return SMK_BAD_PARAM; }
    rc = masked_supported(w, a, k);
    if (rc) return rc;
    MaskedRun r(a, k);
    const DeviceView vW = DeviceView::in(W, dtW, rsW, csW), vH = DeviceView::in(H, dtH, rsH, csH);
    rc = r.f.check(w, vW, vH, false, false);
    if (!rc && col_r) rc = check_device_view(col_r, DT_F64, a->n, 1, 1, a->n, true, (w + "(col_r)").c_str());
    if (!rc && col_a) rc = check_device_view(col_a, DT_F64, a->n, 1, 1, a->n, true, (w + "(col_a)").c_str());
    if (rc) return rc;
    Entry e(r.f.st);
    rc = e.join(stream);
    if (!rc) rc = masked_setup(r, e, false, vW, vH, w);
    double d[3] = {0.0, 0.0, 0.0};
    if (!rc) rc = e.synced(masked_residual(r, col_r, col_a, d));
    if (rc) return rc;
    for (int i = 0; i < 3; ++i) out3[i] = d[i];
    return SMK_OK;
}

int smk_masked_step_time(const smk_matrix* a, int which, int k, int reps, double* ms)
{
    const std::string w("smk_masked_step_time");
    if (int rc = require_init()) return rc;
    if (!a || !ms || which < 0 || which > 3 || k < 1 || reps < 1) { set_error(w + ": bad argument"); return SMK_BAD_PARAM; }
    if (k > a->m || k > a->n_global) { set_error(w + ": k exceeds min(m, n)"); return SMK_BAD_PARAM; }
    int rc = masked_supported(w, a, k);
    if (rc) return rc;
    MaskedRun r(a, k);
    Entry e(r.f.st);
    Owned& own = e.own;
    const hipStream_t st = e.st;
    const int KP = r.f.KP;
    rc = masked_plans(r, e, true);
    if (rc) return rc;
    const bool over_rows = which == 1;                        // the W side: CSC(A'), H gathered; 2 and 3 run on the H side
    const SegPlan& sp = over_rows ? *r.spAt : *r.spA;
    const i64 ng = over_rows ? a->n : a->m, nx = over_rows ? a->m : a->n;
    const i64* colptr = over_rows ? a->colptr_t : a->colptr;
    const double* val = over_rows ? a->val_t : a->val;
    double *G = nullptr, *X = nullptr, *sums = nullptr, *spart = nullptr, *pieces = nullptr, *res = nullptr, *part = nullptr;
    rc = own.dev(&G, (size_t)KP * ng);
    if (!rc) rc = own.dev(&X, (size_t)KP * nx);
    if (!rc) rc = own.dev(&sums, (size_t)KP);
    if (!rc) rc = own.dev(&spart, (size_t)kl_sums_blocks(ng) * KP);
    if (!rc) rc = own.dev(&pieces, (size_t)(sp.npieces > 0 ? sp.npieces : 1) * 128);
    if (!rc) rc = own.dev(&res, (size_t)(a->nnz > 0 ? a->nnz : 1));
    if (!rc) rc = own.dev(&part, (size_t)masked_sweep_partials(sp) + 1);
    if (rc) { set_error(w + ": no device memory"); return SMK_DEVICE_ERROR; }
    rc = launch_fill_factor_uniform(G, k, ng, 11, 0, st);
    if (!rc) rc = launch_fill_factor_uniform(X, k, nx, 12, 0, st);
    if (!rc) rc = launch_kl_factor_sums(G, k, ng, spart, sums, st);
    if (rc) return rc;
    return e.synced(time_launches(w, own, st, reps, [&]() -> int {
        if (which <= 1) return launch_masked_sweep(sp, colptr, val, G, X, k, 0.0, 0.0, res, part, st);
        if (which == 2) return launch_kl_step(sp, colptr, val, G, X, k, sums, 0, 0.0, 0.0, 0, pieces, st);
        const int prc = launch_spmm_seg(sp, colptr, val, G, k, X, KP, st, pieces);
        return prc < 0 ? prc : 0;
    }, ms));
}

int smk_masked_last_profile(int* entry_sweeps, int* residual_sweeps)
{
    if (entry_sweeps) *entry_sweeps = g_masked_entry_sweeps;
    if (residual_sweeps) *residual_sweeps = g_masked_residual_sweeps;
    return SMK_OK;
}

}  // extern "C"
