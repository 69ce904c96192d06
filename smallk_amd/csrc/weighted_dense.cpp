// smallk_amd/csrc/weighted_dense.cpp -- WEIGHTED masked beta-divergence NMF (beta = 2, 1, 0) on a resident DENSE matrix: a second
// resident matrix V of A's shape holds a weight w >= 0 per entry, a NaN in A is still "not measured" (include/smallk_amd.h:
// smk_nmf_weighted_dense_device, smk_matrix_weighted_divergence_dense_device).  The driver is masked_dense_f32.cpp's:
// the factors live as fp32 between steps (weighted_dense.hip updates them), each beside its exact fp64 widening in the FactorPair;
// the start is rounded once on the way in; the widening is what goes back and what the fp64 weighted divergence judges, so
// stats->error is, to the bit, the weighted divergence of the returned factors.  The refusals of the masked solver are made by its
// own code (entry.h: masked_dense_beta, masked_dense_supported); what is added is the comparison of V with A and one look at V.  The
// entries are synchronous; every workspace belongs to the smk::Entry local of the entry; W and H are written once, at the end: on
// any error they are untouched.
#include "entry.h"

#include <algorithm>
#include <cmath>
#include <string>

namespace smk {

struct WeightedRun {
    const smk_matrix *a = nullptr, *v = nullptr;
    int beta = 0;
    FactorPair f;                                 // the fp64 widenings: Wt KP x m and H KP x n, k, KP, the stream
    float *Wt32 = nullptr, *H32 = nullptr;        // the factors themselves: KF x m and KF x n, KF = beta_dense_f32_pitch(k)
    double *scratch = nullptr, *out6 = nullptr;
    double* pin = nullptr;                        // the pinned slot the host reads the divergence from (6 doubles)
    int matrix_passes = 0, divergence_passes = 0;
    WeightedRun(const smk_matrix* a_, const smk_matrix* v_, int k, int beta_)
        : a(a_), v(v_), beta(beta_), f{a_->m, a_->n, k, kp_of(k), matrix_stream(a_)} {}
};

// the last run of the calling thread (smk_weighted_dense_last_profile)
static thread_local int g_wd_matrix_passes = 0, g_wd_divergence_passes = 0;

static size_t weighted_scratch_doubles(i64 rows, i64 cols, int k, int cus)
{
    return (weighted_dense_scratch_bytes(rows, cols, k, cus) + sizeof(double) - 1) / sizeof(double);
}

// V beside A: the same height, width, storage type, leading dimensions and stored copies, so that one offset serves both
static int weighted_same_layout(const std::string& w, const smk_matrix* a, const smk_matrix* v)
{
    if (v->sparse || v->m != a->m || v->n != a->n || v->n_global != a->n_global || v->storage != a->storage) {
        set_error(w + ": the weights must be a dense matrix of A's height, width and storage type");
        return SMK_BAD_PARAM;
    }
    if (v->single != a->single || !v->At != !a->At) { set_error(w + ": the weights must have A's stored copies (one or two)"); return SMK_BAD_PARAM; }
    if (v->ldA != a->ldA || (a->At && v->ldAt != a->ldAt)) { set_error(w + ": the weights must have A's leading dimensions"); return SMK_BAD_PARAM; }
    return SMK_OK;
}

// one look at V per call, beside masked_dense_supported's look at A: no negative, NaN or infinite weight, and a measured entry
// with a positive one
static int weighted_look(const std::string& w, const smk_matrix* a, const smk_matrix* v)
{
    Entry e(matrix_stream(a));
    int* flag = nullptr;
    if (e.own.dev(&flag, 1)) { set_error(w + ": no device memory"); return SMK_DEVICE_ERROR; }
    int found = 0;
    SMK_HIP(hipMemsetAsync(flag, 0, sizeof(int), e.st));
    int rc = launch_weighted_dense_look(a->A, v->A, a->storage, a->ldA, a->m, a->n, flag, e.st);
    if (rc) return rc;
    SMK_HIP(hipMemcpyAsync(&found, flag, sizeof(int), hipMemcpyDeviceToHost, e.st));
    rc = e.sync();
    if (rc) return rc;
    if (found & 1) { set_error(w + ": the weights hold a negative value, a NaN or an infinity"); return SMK_BAD_PARAM; }
    if (!(found & 2)) { set_error(w + ": no measured entry has a positive weight"); return SMK_BAD_PARAM; }
    return SMK_OK;
}

// everything the masked solver refuses, with its codes, then V
static int weighted_supported(const std::string& w, const smk_matrix* a, const smk_matrix* v, int k, int beta, bool needs_transpose)
{
    int rc = masked_dense_supported(w, a, k, beta, needs_transpose);
    if (!rc) rc = weighted_same_layout(w, a, v);
    return rc ? rc : weighted_look(w, a, v);
}

static int weighted_setup(WeightedRun& r, Entry& e, bool both, bool narrow, const DeviceView& W, const DeviceView& H, const std::string& who)
{
    Owned& own = e.own;
    const int KF = beta_dense_f32_pitch(r.f.k), cus = ctx().cus;
    const i64 m = r.a->m, n = r.a->n;
    const size_t sa = weighted_scratch_doubles(m, n, r.f.k, cus), sat = both ? weighted_scratch_doubles(n, m, r.f.k, cus) : 0;
    int rc = own.dev(&r.scratch, std::max(sa, sat));
    if (!rc && narrow) rc = own.dev(&r.Wt32, (size_t)KF * m);
    if (!rc && narrow) rc = own.dev(&r.H32, (size_t)KF * n);
    if (!rc) rc = own.dev(&r.out6, 6);
    if (!rc) rc = own.pinned((void**)&r.pin, 6 * sizeof(double));
    if (rc) { set_error(who + ": no memory for the factor workspace"); return SMK_DEVICE_ERROR; }
    rc = r.f.alloc_zeroed(own, who);
    if (!rc) rc = r.f.load(W, H);
    // the one rounding on the way in; from here on the FactorPair holds the widening of the fp32 factors
    if (!rc && narrow) rc = launch_beta_dense_f32_narrow(r.f.Wt, r.Wt32, r.f.k, m, r.f.st);
    if (!rc && narrow) rc = launch_beta_dense_f32_narrow(r.f.H, r.H32, r.f.k, n, r.f.st);
    return rc;
}

// the flushes are those of the masked form: scikit-learn's W (our H) when beta < 1, its H (our W) when beta <= 1; none at beta = 2
static int wd_step_h(WeightedRun& r, double l1, double l2)
{
    const smk_matrix* a = r.a;
    ++r.matrix_passes;
    return launch_weighted_dense_step(a->A, r.v->A, a->storage, a->ldA, a->m, a->n, r.Wt32, r.H32, r.f.H, r.f.k, r.beta, l1, l2, r.beta < 1,
                                      (float*)r.scratch, ctx().cus, r.f.st);
}

static int wd_step_w(WeightedRun& r, double l1, double l2)
{
    const smk_matrix* a = r.a;
    ++r.matrix_passes;
    return launch_weighted_dense_step(a->At, r.v->At, a->storage, a->ldAt, a->n, a->m, r.H32, r.Wt32, r.f.Wt, r.f.k, r.beta, l1, l2, r.beta <= 1,
                                      (float*)r.scratch, ctx().cus, r.f.st);
}

// out[0 .. 5] = D_w of the widenings, the three sums it is formed from, the number of measured entries and the sum of their
// weights, through the pinned slot: one synchronisation
static int wd_divergence(WeightedRun& r, double* out)
{
    const smk_matrix* a = r.a;
    ++r.divergence_passes;
    const int rc = launch_weighted_dense_divergence(a->A, r.v->A, a->storage, a->ldA, a->m, a->n, r.f.Wt, r.f.H, r.f.k, r.beta, r.scratch, r.out6,
                                                    r.pin, ctx().cus, r.f.st);
    if (rc) return rc;
    SMK_HIP(hipStreamSynchronize(r.f.st));
    for (int i = 0; i < 6; ++i) out[i] = r.pin[i];
    return 0;
}

static int wd_error(WeightedRun& r, double* err)
{
    double d[6];
    const int rc = wd_divergence(r, d);
    if (rc) return rc;
    *err = std::sqrt(2.0 * (d[0] > 0.0 ? d[0] : 0.0));
    return 0;
}

// masked_dense.cpp's loop: the same schedule of steps and checks
static int weighted_loop(WeightedRun& r, const smk_kl_options& o, smk_kl_stats* stats)
{
    const Penalties p(r.a->m, r.a->n, o.alpha_w, o.alpha_h, o.l1_ratio);
    double error_init = 0.0;
    int rc = wd_error(r, &error_init);
    if (rc) return rc;
    double previous = error_init, error = error_init;
    int checked = 0, it = 0, converged = 0;
    for (it = 1; it <= o.max_iter; ++it) {
        rc = wd_step_h(r, p.l1h, p.l2h);
        if (!rc && o.update_w) rc = wd_step_w(r, p.l1w, p.l2w);
        if (rc) return rc;
        if (o.tol > 0.0 && it % 10 == 0) {
            rc = wd_error(r, &error);
            if (rc) return rc;
            checked = it;
            if ((previous - error) / error_init < o.tol) { converged = 1; break; }
            previous = error;
        }
    }
    if (it > o.max_iter) it = o.max_iter;
    if (checked != it) {                        // the error of the factors that go back
        rc = wd_error(r, &error);
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

int smk_nmf_weighted_dense_device(const smk_matrix* a, const smk_matrix* v, int k, double beta, const smk_kl_options* o, void* W, int dtW,
                                  int64_t rsW, int64_t csW, void* H, int dtH, int64_t rsH, int64_t csH, void* stream, smk_kl_stats* stats)
{
    const std::string w("smk_nmf_weighted_dense_device");
    int rc = kl_args(w, a, k, W, dtW, H, dtH);
    if (rc) return rc;
    if (!v || !o || !stats) { set_error(w + ": null argument"); return SMK_BAD_PARAM; }
    rc = check_penalties(w, o->alpha_w, o->alpha_h, o->l1_ratio, o->tol, o->max_iter);
    int b = 0;
    if (!rc) rc = masked_dense_beta(w, beta, &b);
    if (!rc) rc = weighted_supported(w, a, v, k, b, o->update_w != 0);
    if (rc) return rc;
    WeightedRun r(a, v, k, b);
    const DeviceView vW{W, dtW, rsW, csW}, vH{H, dtH, rsH, csH};
    rc = r.f.check(w, vW, vH, o->update_w != 0, true);
    if (rc) return rc;
    Entry e(r.f.st);
    rc = e.join(stream);
    if (!rc) rc = weighted_setup(r, e, o->update_w != 0, true, vW, vH, w);
    smk_kl_stats st{};
    if (!rc) rc = weighted_loop(r, *o, &st);
    g_wd_matrix_passes = r.matrix_passes;
    g_wd_divergence_passes = r.divergence_passes;
    if (!rc) rc = r.f.store(o->update_w ? &vW : nullptr, &vH);
    if (!rc) rc = e.sync();
    if (rc) return rc;
    *stats = st;
    return SMK_OK;
}

int smk_matrix_weighted_divergence_dense_device(const smk_matrix* a, const smk_matrix* v, int k, double beta, const void* W, int dtW, int64_t rsW,
                                                int64_t csW, const void* H, int dtH, int64_t rsH, int64_t csH, void* stream, double* out)
{
    const std::string w("smk_matrix_weighted_divergence_dense_device");
    int rc = kl_args(w, a, k, W, dtW, H, dtH);
    if (rc) return rc;
    if (!v || !out) { set_error(w + ": null argument"); return SMK_BAD_PARAM; }
    int b = 0;
    rc = masked_dense_beta(w, beta, &b);
    if (!rc) rc = weighted_supported(w, a, v, k, b, false);
    if (rc) return rc;
    WeightedRun r(a, v, k, b);
    const DeviceView vW = DeviceView::in(W, dtW, rsW, csW), vH = DeviceView::in(H, dtH, rsH, csH);
    rc = r.f.check(w, vW, vH, false, false);
    if (rc) return rc;
    Entry e(r.f.st);
    rc = e.join(stream);
    if (!rc) rc = weighted_setup(r, e, false, false, vW, vH, w);
    double d[6] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
    if (!rc) rc = e.synced(wd_divergence(r, d));
    if (rc) return rc;
    for (int i = 0; i < 6; ++i) out[i] = d[i];
    return SMK_OK;
}

int smk_weighted_dense_step_time(const smk_matrix* a, const smk_matrix* v, int which, int k, double beta, int reps, double* ms)
{
    const std::string w("smk_weighted_dense_step_time");
    if (int rc = require_init()) return rc;
    if (!a || !v || !ms || which < 0 || which > 2 || k < 1 || k > 128 || reps < 1) { set_error(w + ": bad argument"); return SMK_BAD_PARAM; }
    int b = 0;
    int rc = masked_dense_beta(w, beta, &b);
    if (rc) return rc;
    if (a->sparse || a->n != a->n_global || (which == 1 && (a->single || !a->At))) { set_error(w + ": a dense, unsharded matrix with the copy the step reads"); return SMK_UNSUPPORTED; }
    rc = weighted_same_layout(w, a, v);
    if (rc) return rc;
    Entry e(matrix_stream(a));
    Owned& own = e.own;
    const hipStream_t st = e.st;
    const int KP = kp_of(k), KF = beta_dense_f32_pitch(k), cus = ctx().cus;
    const bool over_rows = which == 1;                        // the W side: the stored transposes, H the factor of their rows
    const i64 rows = over_rows ? a->n : a->m, cols = over_rows ? a->m : a->n;
    const void *A = over_rows ? a->At : a->A, *V = over_rows ? v->At : v->A;
    const i64 ld = over_rows ? a->ldAt : a->ldA;
    double *R = nullptr, *X = nullptr, *scratch = nullptr;
    float *R32 = nullptr, *X32 = nullptr;
    const size_t s_wd = weighted_scratch_doubles(rows, cols, k, cus);
    const size_t s_mf = (masked_dense_f32_scratch_bytes(rows, cols, k, cus) + sizeof(double) - 1) / sizeof(double);
    rc = own.dev(&R, (size_t)KP * rows);
    if (!rc) rc = own.dev(&X, (size_t)KP * cols);
    if (!rc) rc = own.dev(&R32, (size_t)KF * rows);
    if (!rc) rc = own.dev(&X32, (size_t)KF * cols);
    if (!rc) rc = own.dev(&scratch, std::max(s_wd, s_mf));
    if (rc) { set_error(w + ": no device memory"); return SMK_DEVICE_ERROR; }
    rc = launch_fill_factor_uniform(R, k, rows, 11, 0, st);
    if (!rc) rc = launch_fill_factor_uniform(X, k, cols, 12, 0, st);
    if (!rc) rc = launch_beta_dense_f32_narrow(R, R32, k, rows, st);
    if (!rc) rc = launch_beta_dense_f32_narrow(X, X32, k, cols, st);
    if (rc) return rc;
    return e.synced(time_launches(w, own, st, reps, [&]() -> int {
        if (which <= 1) return launch_weighted_dense_step(A, V, a->storage, ld, rows, cols, R32, X32, X, k, b, 0.0, 0.0, 0, (float*)scratch, cus, st);
        return launch_masked_dense_f32_step(A, a->storage, ld, rows, cols, R32, X32, X, k, b, 0.0, 0.0, 0, (float*)scratch, cus, st);   // the masked fp32 step
    }, ms));
}

int smk_weighted_dense_last_profile(int* matrix_passes, int* divergence_passes)
{
    if (matrix_passes) *matrix_passes = g_wd_matrix_passes;
    if (divergence_passes) *divergence_passes = g_wd_divergence_passes;
    return SMK_OK;
}

}  // extern "C"
