// smallk_amd/csrc/kl_dense.cpp -- NMF of a resident DENSE matrix under the generalised Kullback-Leibler divergence by multiplicative
// updates (include/smallk_amd.h: smk_nmf_kl_dense_device, smk_matrix_kl_divergence_dense_device): kl.cpp's iteration
// over every entry of the stored matrix.  Each half-iteration is one streaming read of one stored copy by kl_dense.hip -- A for the
// H step, the stored transpose for the W step -- and the denominators are the row sums of the other factor.  The entries are
// synchronous; every workspace belongs to the smk::Entry local of the entry (entry.h: synchronised before it releases them, on
// every path); of the matrix handle only the once-per-matrix sign record is written.  W and H are written once, at the end: on any
// error they are untouched.  Between two checks of the stopping rule an iteration is launches on one stream; the pinned slot is
// read on check iterations only.
#include "entry.h"

#include <cmath>
#include <mutex>
#include <string>

namespace smk {

struct KlDenseRun {
    const smk_matrix* a = nullptr;
    FactorPair f;                                 // the factors: Wt KP x m and H KP x n, k, KP, the stream
    double *sumsW = nullptr, *sumsH = nullptr, *part = nullptr, *scratch = nullptr, *out4 = nullptr;
    double* pin = nullptr;                        // the pinned slot the host reads the divergence from (4 doubles)
    int matrix_passes = 0, divergence_passes = 0;
    KlDenseRun(const smk_matrix* a_, int k) : a(a_), f{a_->m, a_->n, k, kp_of(k), matrix_stream(a_)} {}
};

// the last run of the calling thread (smk_kl_dense_last_profile)
static thread_local int g_kld_matrix_passes = 0, g_kld_divergence_passes = 0;

// no stored value may be negative: looked up once per matrix by a reduction on the device (the matrix's contents change only
// through upload / adopt / fill, which reset the record).  The same look records whether a zero is stored (beta_dense.cpp).
int kl_dense_sign_check(const smk_matrix* a, const std::string& w)
{
    static std::mutex mu;             // lazily built part of a shared, nominally const matrix (as kl.cpp's)
    std::lock_guard<std::mutex> lk(mu);
    if (a->kl_negative < 0) {
        Entry e(matrix_stream(a));
        int* flag = nullptr;
        if (e.own.dev(&flag, 1)) { set_error(w + ": no device memory"); return SMK_DEVICE_ERROR; }
        int neg = 0;
        SMK_HIP(hipMemsetAsync(flag, 0, sizeof(int), e.st));
        int rc = launch_kl_dense_negative(a->A, a->storage, a->ldA, a->m, a->n, flag, e.st);
        if (rc) return rc;
        SMK_HIP(hipMemcpyAsync(&neg, flag, sizeof(int), hipMemcpyDeviceToHost, e.st));
        rc = e.sync();
        if (rc) return rc;
        a->kl_zero = (neg >> 1) & 1;
        a->kl_negative = neg & 1;
    }
    if (a->kl_negative == 1) { set_error(w + ": the matrix stores a negative value"); return SMK_BAD_PARAM; }
    return 0;
}

// needs_transpose: the W step runs on the stored transpose, and building one behind the caller's back doubles the footprint
static int kl_dense_supported(const std::string& w, const smk_matrix* a, int k, bool needs_transpose)
{
    if (a->sparse) { set_error(w + ": takes a dense matrix (smk_nmf_kl_device takes a sparse one)"); return SMK_UNSUPPORTED; }
    if (k > 128) { set_error(w + ": k > 128 is not supported yet"); return SMK_UNSUPPORTED; }
    if (a->n != a->n_global) { set_error(w + ": not available on a column shard"); return SMK_UNSUPPORTED; }
    if (needs_transpose && (a->single || !a->At)) {
        set_error(w + ": the W step needs the stored transpose; a single-copy matrix serves update_w = 0 only");
        return SMK_UNSUPPORTED;
    }
    return kl_dense_sign_check(a, w);
}

static size_t kl_dense_scratch(const smk_matrix* a, int k, bool both)
{
    const size_t sa = kl_dense_scratch_elems(a->m, a->n, k, ctx().cus);
    const size_t sat = both ? kl_dense_scratch_elems(a->n, a->m, k, ctx().cus) : 0;
    return sa > sat ? sa : sat;
}

// the sums' and the passes' scratch, the zeroed factor workspaces and the views converted in
static int kl_dense_setup(KlDenseRun& r, Entry& e, bool both, const DeviceView& W, const DeviceView& H, const std::string& who)
{
    Owned& own = e.own;
    const int KP = r.f.KP;
    const i64 nmax = r.a->m > r.a->n ? r.a->m : r.a->n;
    int rc = own.dev(&r.sumsW, (size_t)KP);
    if (!rc) rc = own.dev(&r.sumsH, (size_t)KP);
    if (!rc) rc = own.dev(&r.part, (size_t)kl_sums_blocks(nmax) * KP);
    if (!rc) rc = own.dev(&r.scratch, kl_dense_scratch(r.a, r.f.k, both));
    if (!rc) rc = own.dev(&r.out4, 4);
    if (!rc) rc = own.pinned((void**)&r.pin, 4 * sizeof(double));
    if (rc) { set_error(who + ": no memory for the factor workspace"); return SMK_DEVICE_ERROR; }
    rc = r.f.alloc_zeroed(own, who);
    return rc ? rc : r.f.load(W, H);
}

static int kld_sums_w(KlDenseRun& r) { return launch_kl_factor_sums(r.f.Wt, r.f.k, r.a->m, r.part, r.sumsW, r.f.st); }
static int kld_sums_h(KlDenseRun& r) { return launch_kl_factor_sums(r.f.H, r.f.k, r.a->n, r.part, r.sumsH, r.f.st); }

static int kld_step_h(KlDenseRun& r, double l1, double l2)
{
    const smk_matrix* a = r.a;
    ++r.matrix_passes;
    return launch_kl_dense_step(a->A, a->storage, a->ldA, a->m, a->n, r.f.Wt, r.f.H, r.f.k, r.sumsW, 0, l1, l2, 0, r.scratch, ctx().cus, r.f.st);
}

static int kld_step_w(KlDenseRun& r, double l1, double l2)
{
    const smk_matrix* a = r.a;
    ++r.matrix_passes;
    return launch_kl_dense_step(a->At, a->storage, a->ldAt, a->n, a->m, r.f.H, r.f.Wt, r.f.k, r.sumsH, 1, l1, l2, 1, r.scratch, ctx().cus, r.f.st);
}

// out[0 .. 3] = D, sum a log(a / d), sum WH, sum a of the current factors (their row sums in place), through the pinned slot: one
// synchronisation
static int kld_divergence(KlDenseRun& r, double* out)
{
    const smk_matrix* a = r.a;
    ++r.divergence_passes;
    const int rc = launch_kl_dense_divergence(a->A, a->storage, a->ldA, a->m, a->n, r.f.Wt, r.f.H, r.f.k, r.sumsW, r.sumsH, r.scratch, r.out4, r.pin,
                                              ctx().cus, r.f.st);
    if (rc) return rc;
    SMK_HIP(hipStreamSynchronize(r.f.st));
    for (int i = 0; i < 4; ++i) out[i] = r.pin[i];
    return 0;
}

static int kld_error(KlDenseRun& r, double* err)
{
    double d[4];
    const int rc = kld_divergence(r, d);
    if (rc) return rc;
    *err = std::sqrt(2.0 * (d[0] > 0.0 ? d[0] : 0.0));
    return 0;
}

// kl.cpp's loop: the same schedule of sums, steps and checks
static int kl_dense_loop(KlDenseRun& r, const smk_kl_options& o, smk_kl_stats* stats)
{
    const Penalties p(r.a->m, r.a->n, o.alpha_w, o.alpha_h, o.l1_ratio);
    int rc = kld_sums_w(r);                     // update_w = 0: formed once
    if (!rc) rc = kld_sums_h(r);
    double error_init = 0.0;
    if (!rc) rc = kld_error(r, &error_init);
    if (rc) return rc;
    double previous = error_init, error = error_init;
    int checked = 0, it = 0, converged = 0;
    for (it = 1; it <= o.max_iter; ++it) {
        rc = kld_step_h(r, p.l1h, p.l2h);
        if (!rc && o.update_w) {
            rc = kld_sums_h(r);
            if (!rc) rc = kld_step_w(r, p.l1w, p.l2w);
            if (!rc) rc = kld_sums_w(r);
        }
        if (rc) return rc;
        if (o.tol > 0.0 && it % 10 == 0) {
            if (!o.update_w) rc = kld_sums_h(r);
            if (!rc) rc = kld_error(r, &error);
            if (rc) return rc;
            checked = it;
            if ((previous - error) / error_init < o.tol) { converged = 1; break; }
            previous = error;
        }
    }
    if (it > o.max_iter) it = o.max_iter;
    if (checked != it) {                        // the error of the factors that go back
        if (!o.update_w) rc = kld_sums_h(r);
        if (!rc) rc = kld_error(r, &error);
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

int smk_nmf_kl_dense_device(const smk_matrix* a, int k, const smk_kl_options* o, void* W, int dtW, int64_t rsW, int64_t csW, void* H, int dtH,
                            int64_t rsH, int64_t csH, void* stream, smk_kl_stats* stats)
{
    const std::string w("smk_nmf_kl_dense_device");
    int rc = kl_args(w, a, k, W, dtW, H, dtH);
    if (rc) return rc;
    if (!o || !stats) { set_error(w + ": null argument"); return SMK_BAD_PARAM; }
    rc = check_penalties(w, o->alpha_w, o->alpha_h, o->l1_ratio, o->tol, o->max_iter);
    if (!rc) rc = kl_dense_supported(w, a, k, o->update_w != 0);
    if (rc) return rc;
    KlDenseRun r(a, k);
    const DeviceView vW{W, dtW, rsW, csW}, vH{H, dtH, rsH, csH};
    rc = r.f.check(w, vW, vH, o->update_w != 0, true);
    if (rc) return rc;
    Entry e(r.f.st);
    rc = e.join(stream);
    if (!rc) rc = kl_dense_setup(r, e, o->update_w != 0, vW, vH, w);
    smk_kl_stats st{};
    if (!rc) rc = kl_dense_loop(r, *o, &st);
    g_kld_matrix_passes = r.matrix_passes;
    g_kld_divergence_passes = r.divergence_passes;
    if (!rc) rc = r.f.store(o->update_w ? &vW : nullptr, &vH);
    if (!rc) rc = e.sync();
    if (rc) return rc;
    *stats = st;
    return SMK_OK;
}

int smk_matrix_kl_divergence_dense_device(const smk_matrix* a, int k, const void* W, int dtW, int64_t rsW, int64_t csW, const void* H, int dtH,
                                          int64_t rsH, int64_t csH, void* stream, double* out)
{
    const std::string w("smk_matrix_kl_divergence_dense_device");
    int rc = kl_args(w, a, k, W, dtW, H, dtH);
    if (rc) return rc;
    if (!out) { set_error(w + ": null output"); return SMK_BAD_PARAM; }
    rc = kl_dense_supported(w, a, k, false);
    if (rc) return rc;
    KlDenseRun r(a, k);
    const DeviceView vW = DeviceView::in(W, dtW, rsW, csW), vH = DeviceView::in(H, dtH, rsH, csH);
    rc = r.f.check(w, vW, vH, false, false);
    if (rc) return rc;
    Entry e(r.f.st);
    rc = e.join(stream);
    if (!rc) rc = kl_dense_setup(r, e, false, vW, vH, w);
    if (!rc) rc = kld_sums_w(r);
    if (!rc) rc = kld_sums_h(r);
    double d[4] = {0.0, 0.0, 0.0, 0.0};
    if (!rc) rc = e.synced(kld_divergence(r, d));
    if (rc) return rc;
    out[0] = d[0];
    out[1] = d[1];
    out[2] = d[2];
    return SMK_OK;
}

int smk_kl_dense_step_time(const smk_matrix* a, int which, int k, int reps, double* ms)
{
    const std::string w("smk_kl_dense_step_time");
    if (int rc = require_init()) return rc;
    if (!a || !ms || which < 0 || which > 2 || k < 1 || reps < 1) { set_error(w + ": bad argument"); return SMK_BAD_PARAM; }
    int rc = kl_dense_supported(w, a, k, which == 1);
    if (rc) return rc;
    Entry e(matrix_stream(a));
    Owned& own = e.own;
    const hipStream_t st = e.st;
    const int KP = kp_of(k), cus = ctx().cus;
    const bool over_rows = which == 1;                        // the W side: the stored transpose, H the factor of its rows
    const i64 rows = over_rows ? a->n : a->m, cols = over_rows ? a->m : a->n;
    const void* A = over_rows ? a->At : a->A;
    const i64 ld = over_rows ? a->ldAt : a->ldA;
    double *R = nullptr, *X = nullptr, *sums = nullptr, *part = nullptr, *scratch = nullptr, *col_r = nullptr, *col_a = nullptr, *out2 = nullptr;
    const size_t s_kl = kl_dense_scratch_elems(rows, cols, k, cus), s_res = residual_dense_scratch_elems(rows, cols, cus);
    rc = own.dev(&R, (size_t)KP * rows);
    if (!rc) rc = own.dev(&X, (size_t)KP * cols);
    if (!rc) rc = own.dev(&sums, (size_t)KP);
    if (!rc) rc = own.dev(&part, (size_t)kl_sums_blocks(rows) * KP);
    if (!rc) rc = own.dev(&scratch, s_kl > s_res ? s_kl : s_res);
    if (!rc) rc = own.dev(&col_r, (size_t)cols);
    if (!rc) rc = own.dev(&col_a, (size_t)cols);
    if (!rc) rc = own.dev(&out2, 2);
    if (rc) { set_error(w + ": no device memory"); return SMK_DEVICE_ERROR; }
    rc = launch_fill_factor_uniform(R, k, rows, 11, 0, st);
    if (!rc) rc = launch_fill_factor_uniform(X, k, cols, 12, 0, st);
    if (!rc) rc = launch_kl_factor_sums(R, k, rows, part, sums, st);
    if (rc) return rc;
    return e.synced(time_launches(w, own, st, reps, [&]() -> int {
        if (which <= 1) return launch_kl_dense_step(A, a->storage, ld, rows, cols, R, X, k, sums, which, 0.0, 0.0, which, scratch, cus, st);
        return launch_residual_dense(A, a->storage, ld, rows, cols, R, X, KP, k, scratch, col_r, col_a, out2, cus, st);
    }, ms));
}

int smk_kl_dense_last_profile(int* matrix_passes, int* divergence_passes)
{
    if (matrix_passes) *matrix_passes = g_kld_matrix_passes;
    if (divergence_passes) *divergence_passes = g_kld_divergence_passes;
    return SMK_OK;
}

}  // extern "C"
