// smallk_amd/csrc/masked_dense.cpp -- NMF of a resident DENSE matrix fitted to its MEASURED entries only, under the beta-divergence
// for beta = 2, 1 or 0, by multiplicative updates (include/smallk_amd.h: smk_nmf_masked_dense_device,
// smk_matrix_masked_divergence_dense_device).  A stored NaN is "not measured"; every other stored value is a
// measurement, 0 included.  The shape is beta_dense.cpp's: each half-iteration is one streaming read of one stored copy by
// masked_dense.hip -- A for the H step, the stored transpose for the W step --, both sums of the update come out of that pass, and
// the mask travels inside the copies.  The entries are synchronous; every workspace belongs to the smk::Entry local of the entry;
// nothing of the matrix handle is written: the look at the stored values (a measured negative value, a measured zero, any measured
// entry at all) is one more read of A per call, because the handle's sign record counts a NaN as a zero.  W and H are written
// once, at the end: on any error they are untouched.  The pinned slot is read on check iterations only.
#include "entry.h"

#include <cmath>
#include <string>

namespace smk {

struct MaskedDenseRun {
    const smk_matrix* a = nullptr;
    int beta = 0;
    FactorPair f;                                 // the factors: Wt KP x m and H KP x n, k, KP, the stream
    double *scratch = nullptr, *out5 = nullptr;
    double* pin = nullptr;                        // the pinned slot the host reads the divergence from (5 doubles)
    int matrix_passes = 0, divergence_passes = 0;
    MaskedDenseRun(const smk_matrix* a_, int k, int beta_) : a(a_), beta(beta_), f{a_->m, a_->n, k, kp_of(k), matrix_stream(a_)} {}
};

// the last run of the calling thread (smk_masked_dense_last_profile)
static thread_local int g_md_matrix_passes = 0, g_md_divergence_passes = 0;

// beta itself: 0, 1 or 2 (SMK_UNSUPPORTED otherwise; a NaN compares unequal to all three)
int masked_dense_beta(const std::string& w, double beta, int* out)
{
    if (beta != 0.0 && beta != 1.0 && beta != 2.0) { set_error(w + ": beta must be 0, 1 or 2"); return SMK_UNSUPPORTED; }
    *out = (int)beta;
    return SMK_OK;
}

// kl_dense.cpp's conditions on the matrix, then the measured data: some, none negative, and no zero at beta = 0
int masked_dense_supported(const std::string& w, const smk_matrix* a, int k, int beta, bool needs_transpose)
{
    if (a->sparse) { set_error(w + ": takes a dense matrix, NaN where nothing was measured (smk_nmf_masked_device takes a sparse one)"); return SMK_UNSUPPORTED; }
    if (k > 128) { set_error(w + ": k > 128 is not supported yet"); return SMK_UNSUPPORTED; }
    if (a->n != a->n_global) { set_error(w + ": not available on a column shard"); return SMK_UNSUPPORTED; }
    if (needs_transpose && (a->single || !a->At)) {
        set_error(w + ": the W step needs the stored transpose; a single-copy matrix serves update_w = 0 only");
        return SMK_UNSUPPORTED;
    }
    Entry e(matrix_stream(a));
    int* flag = nullptr;
    if (e.own.dev(&flag, 1)) { set_error(w + ": no device memory"); return SMK_DEVICE_ERROR; }
    int found = 0;
    SMK_HIP(hipMemsetAsync(flag, 0, sizeof(int), e.st));
    int rc = launch_masked_dense_look(a->A, a->storage, a->ldA, a->m, a->n, flag, e.st);
    if (rc) return rc;
    SMK_HIP(hipMemcpyAsync(&found, flag, sizeof(int), hipMemcpyDeviceToHost, e.st));
    rc = e.sync();
    if (rc) return rc;
    if (!(found & 4)) { set_error(w + ": the matrix has no measured entry (every stored value is NaN)"); return SMK_BAD_PARAM; }
    if (found & 1) { set_error(w + ": the matrix stores a negative value"); return SMK_BAD_PARAM; }
    if (beta == 0 && (found & 2)) {
        set_error(w + ": beta <= 0 and the matrix stores a zero: the iteration may diverge; add a small value to the matrix or use a positive beta");
        return SMK_BAD_PARAM;
    }
    return SMK_OK;
}

static int masked_dense_setup(MaskedDenseRun& r, Entry& e, bool both, const DeviceView& W, const DeviceView& H, const std::string& who)
{
    Owned& own = e.own;
    const size_t sa = masked_dense_scratch_elems(r.a->m, r.a->n, r.f.k, ctx().cus);
    const size_t sat = both ? masked_dense_scratch_elems(r.a->n, r.a->m, r.f.k, ctx().cus) : 0;
    int rc = own.dev(&r.scratch, sa > sat ? sa : sat);
    if (!rc) rc = own.dev(&r.out5, 5);
    if (!rc) rc = own.pinned((void**)&r.pin, 5 * sizeof(double));
    if (rc) { set_error(who + ": no memory for the factor workspace"); return SMK_DEVICE_ERROR; }
    rc = r.f.alloc_zeroed(own, who);
    return rc ? rc : r.f.load(W, H);
}

// the flushes: scikit-learn's W (our H) below 2^-52 becomes 0 when beta < 1, its H (our W) when beta <= 1; none at beta = 2
static int md_step_h(MaskedDenseRun& r, double l1, double l2)
{
    const smk_matrix* a = r.a;
    ++r.matrix_passes;
    return launch_masked_dense_step(a->A, a->storage, a->ldA, a->m, a->n, r.f.Wt, r.f.H, r.f.k, r.beta, l1, l2, r.beta < 1, r.scratch, ctx().cus, r.f.st);
}

static int md_step_w(MaskedDenseRun& r, double l1, double l2)
{
    const smk_matrix* a = r.a;
    ++r.matrix_passes;
    return launch_masked_dense_step(a->At, a->storage, a->ldAt, a->n, a->m, r.f.H, r.f.Wt, r.f.k, r.beta, l1, l2, r.beta <= 1, r.scratch, ctx().cus,
                                    r.f.st);
}

// out[0 .. 4] = D over the measured entries, the three sums it is formed from and their number, through the pinned slot: one
// synchronisation
static int md_divergence(MaskedDenseRun& r, double* out)
{
    const smk_matrix* a = r.a;
    ++r.divergence_passes;
    const int rc = launch_masked_dense_divergence(a->A, a->storage, a->ldA, a->m, a->n, r.f.Wt, r.f.H, r.f.k, r.beta, r.scratch, r.out5, r.pin,
                                                  ctx().cus, r.f.st);
    if (rc) return rc;
    SMK_HIP(hipStreamSynchronize(r.f.st));
    for (int i = 0; i < 5; ++i) out[i] = r.pin[i];
    return 0;
}

static int md_error(MaskedDenseRun& r, double* err)
{
    double d[5];
    const int rc = md_divergence(r, d);
    if (rc) return rc;
    *err = std::sqrt(2.0 * (d[0] > 0.0 ? d[0] : 0.0));
    return 0;
}

// beta_dense.cpp's loop: the same schedule of steps and checks
static int masked_dense_loop(MaskedDenseRun& r, const smk_kl_options& o, smk_kl_stats* stats)
{
    const Penalties p(r.a->m, r.a->n, o.alpha_w, o.alpha_h, o.l1_ratio);
    double error_init = 0.0;
    int rc = md_error(r, &error_init);
    if (rc) return rc;
    double previous = error_init, error = error_init;
    int checked = 0, it = 0, converged = 0;
    for (it = 1; it <= o.max_iter; ++it) {
        rc = md_step_h(r, p.l1h, p.l2h);
        if (!rc && o.update_w) rc = md_step_w(r, p.l1w, p.l2w);
        if (rc) return rc;
        if (o.tol > 0.0 && it % 10 == 0) {
            rc = md_error(r, &error);
            if (rc) return rc;
            checked = it;
            if ((previous - error) / error_init < o.tol) { converged = 1; break; }
            previous = error;
        }
    }
    if (it > o.max_iter) it = o.max_iter;
    if (checked != it) {                        // the error of the factors that go back
        rc = md_error(r, &error);
        if (rc) return rc;
    }
    stats->iterations = it;
    stats->converged = converged;
    stats->error_init = error_init;
    stats->error = error;
    return 0;
}

}  // namespace smk

extern "C" {

int smk_nmf_masked_dense_device(const smk_matrix* a, int k, double beta, const smk_kl_options* o, void* W, int dtW, int64_t rsW, int64_t csW, void* H,
                                int dtH, int64_t rsH, int64_t csH, void* stream, smk_kl_stats* stats)
{
    const std::string w("smk_nmf_masked_dense_device");
    int rc = kl_args(w, a, k, W, dtW, H, dtH);
    if (rc) return rc;
    if (!o || !stats) { set_error(w + ": null argument"); return SMK_BAD_PARAM; }
    rc = check_penalties(w, o->alpha_w, o->alpha_h, o->l1_ratio, o->tol, o->max_iter);
    int b = 0;
    if (!rc) rc = masked_dense_beta(w, beta, &b);
    if (!rc) rc = masked_dense_supported(w, a, k, b, o->update_w != 0);
    if (rc) return rc;
    MaskedDenseRun r(a, k, b);
    const DeviceView vW{W, dtW, rsW, csW}, vH{H, dtH, rsH, csH};
    rc = r.f.check(w, vW, vH, o->update_w != 0, true);
    if (rc) return rc;
    Entry e(r.f.st);
    rc = e.join(stream);
    if (!rc) rc = masked_dense_setup(r, e, o->update_w != 0, vW, vH, w);
    smk_kl_stats st{};
    if (!rc) rc = masked_dense_loop(r, *o, &st);
    g_md_matrix_passes = r.matrix_passes;
    g_md_divergence_passes = r.divergence_passes;
    if (!rc) rc = r.f.store(o->update_w ? &vW : nullptr, &vH);
    if (!rc) rc = e.sync();
    if (rc) return rc;
    *stats = st;
    return SMK_OK;
}

int smk_matrix_masked_divergence_dense_device(const smk_matrix* a, int k, double beta, const void* W, int dtW, int64_t rsW, int64_t csW,
                                              const void* H, int dtH, int64_t rsH, int64_t csH, void* stream, double* out)
{
    const std::string w("smk_matrix_masked_divergence_dense_device");
    int rc = kl_args(w, a, k, W, dtW, H, dtH);
    if (rc) return rc;
    if (!out) { set_error(w + ": null output"); return SMK_BAD_PARAM; }
    int b = 0;
    rc = masked_dense_beta(w, beta, &b);
    if (!rc) rc = masked_dense_supported(w, a, k, b, false);
    if (rc) return rc;
    MaskedDenseRun r(a, k, b);
    const DeviceView vW = DeviceView::in(W, dtW, rsW, csW), vH = DeviceView::in(H, dtH, rsH, csH);
    rc = r.f.check(w, vW, vH, false, false);
    if (rc) return rc;
    Entry e(r.f.st);
    rc = e.join(stream);
    if (!rc) rc = masked_dense_setup(r, e, false, vW, vH, w);
    double d[5] = {0.0, 0.0, 0.0, 0.0, 0.0};
    if (!rc) rc = e.synced(md_divergence(r, d));
    if (rc) return rc;
    for (int i = 0; i < 5; ++i) out[i] = d[i];
    return SMK_OK;
}

int smk_masked_dense_step_time(const smk_matrix* a, int which, int k, double beta, int reps, double* ms)
{
    const std::string w("smk_masked_dense_step_time");
    if (int rc = require_init()) return rc;
    if (!a || !ms || which < 0 || which > 2 || k < 1 || k > 128 || reps < 1) { set_error(w + ": bad argument"); return SMK_BAD_PARAM; }
    int b = 0;
    int rc = masked_dense_beta(w, beta, &b);
    if (rc) return rc;
    if (a->sparse || a->n != a->n_global || (which == 1 && (a->single || !a->At))) { set_error(w + ": a dense, unsharded matrix with the copy the step reads"); return SMK_UNSUPPORTED; }
    Entry e(matrix_stream(a));
    Owned& own = e.own;
    const hipStream_t st = e.st;
    const int KP = kp_of(k), cus = ctx().cus;
    const bool over_rows = which == 1;                        // the W side: the stored transpose, H the factor of its rows
    const i64 rows = over_rows ? a->n : a->m, cols = over_rows ? a->m : a->n;
    const void* A = over_rows ? a->At : a->A;
    const i64 ld = over_rows ? a->ldAt : a->ldA;
    double *R = nullptr, *X = nullptr, *scratch = nullptr;
    const size_t s_md = masked_dense_scratch_elems(rows, cols, k, cus), s_bd = beta_dense_scratch_elems(rows, cols, k, cus);
    rc = own.dev(&R, (size_t)KP * rows);
    if (!rc) rc = own.dev(&X, (size_t)KP * cols);
    if (!rc) rc = own.dev(&scratch, s_md > s_bd ? s_md : s_bd);
    if (rc) { set_error(w + ": no device memory"); return SMK_DEVICE_ERROR; }
    rc = launch_fill_factor_uniform(R, k, rows, 11, 0, st);
    if (!rc) rc = launch_fill_factor_uniform(X, k, cols, 12, 0, st);
    if (rc) return rc;
    return e.synced(time_launches(w, own, st, reps, [&]() -> int {
        if (which <= 1) return launch_masked_dense_step(A, a->storage, ld, rows, cols, R, X, k, b, 0.0, 0.0, 0, scratch, cus, st);
        return launch_beta_dense_step(A, a->storage, ld, rows, cols, R, X, k, 0.0, 0.0, 0.0, 0, scratch, cus, st);       // DESIGN.md 21's beta = 0 step
    }, ms));
}

int smk_masked_dense_last_profile(int* matrix_passes, int* divergence_passes)
{
    if (matrix_passes) *matrix_passes = g_md_matrix_passes;
    if (divergence_passes) *divergence_passes = g_md_divergence_passes;
    return SMK_OK;
}

}  // extern "C"
