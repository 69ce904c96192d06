// smallk_amd/csrc/masked_dense_f32.cpp -- the fp32 form of masked beta-divergence NMF (beta = 2, 1, 0) on a resident DENSE matrix
// whose NaNs are "not measured" (include/smallk_amd.h: smk_nmf_masked_dense_f32_device).  The iteration, the schedule
// of checks, the look at the stored values and the refusals are masked_dense.cpp's; what differs is where each precision applies,
// as in beta_dense_f32.cpp.  Between steps the factors live as fp32 (masked_dense_f32.hip updates them), each beside its exact fp64
// widening in the FactorPair: the start is rounded once on the way in, the widening is what goes back to the caller and what the
// EXISTING fp64 divergence of masked_dense.hip judges -- so stats->error is, to the bit, the masked divergence of the returned
// factors and the stopping rule carries no fp32 noise.  The entries are synchronous; every workspace belongs to the smk::Entry
// local of the entry; W and H are written once, at the end: on any error they are untouched.
#include "entry.h"

#include <algorithm>
#include <cmath>
#include <string>

namespace smk {

struct MaskedF32Run {
    const smk_matrix* a = nullptr;
    int beta = 0;
    FactorPair f;                                 // the fp64 widenings: Wt KP x m and H KP x n, k, KP, the stream
    float *Wt32 = nullptr, *H32 = nullptr;        // the factors themselves: KF x m and KF x n, KF = beta_dense_f32_pitch(k)
    double *scratch = nullptr, *out5 = nullptr;
    double* pin = nullptr;                        // the pinned slot the host reads the divergence from (5 doubles)
    int matrix_passes = 0, divergence_passes = 0;
    MaskedF32Run(const smk_matrix* a_, int k, int beta_) : a(a_), beta(beta_), f{a_->m, a_->n, k, kp_of(k), matrix_stream(a_)} {}
};

// the last run of the calling thread (smk_masked_dense_f32_last_profile)
static thread_local int g_mf_matrix_passes = 0, g_mf_divergence_passes = 0;

// one block serves the fp32 partials of a step and the fp64 partials of the divergence (and, when timing, of the fp64 step)
static size_t masked_f32_scratch_doubles(i64 rows, i64 cols, int k, int cus)
{
    const size_t step = (masked_dense_f32_scratch_bytes(rows, cols, k, cus) + sizeof(double) - 1) / sizeof(double);
    return std::max(step, masked_dense_scratch_elems(rows, cols, k, cus));
}

static int masked_f32_setup(MaskedF32Run& r, Entry& e, bool both, const DeviceView& W, const DeviceView& H, const std::string& who)
{
    Owned& own = e.own;
    const int KF = beta_dense_f32_pitch(r.f.k), cus = ctx().cus;
    const i64 m = r.a->m, n = r.a->n;
    const size_t sa = masked_f32_scratch_doubles(m, n, r.f.k, cus), sat = both ? masked_f32_scratch_doubles(n, m, r.f.k, cus) : 0;
    int rc = own.dev(&r.scratch, std::max(sa, sat));
    if (!rc) rc = own.dev(&r.Wt32, (size_t)KF * m);
    if (!rc) rc = own.dev(&r.H32, (size_t)KF * n);
    if (!rc) rc = own.dev(&r.out5, 5);
    if (!rc) rc = own.pinned((void**)&r.pin, 5 * sizeof(double));
    if (rc) { set_error(who + ": no memory for the factor workspace"); return SMK_DEVICE_ERROR; }
    rc = r.f.alloc_zeroed(own, who);
    if (!rc) rc = r.f.load(W, H);
    // the one rounding on the way in; from here on the FactorPair holds the widening of the fp32 factors
    if (!rc) rc = launch_beta_dense_f32_narrow(r.f.Wt, r.Wt32, r.f.k, m, r.f.st);
    if (!rc) rc = launch_beta_dense_f32_narrow(r.f.H, r.H32, r.f.k, n, r.f.st);
    return rc;
}

// the flushes are those of the fp64 form: scikit-learn's W (our H) when beta < 1, its H (our W) when beta <= 1; none at beta = 2
static int mf_step_h(MaskedF32Run& r, double l1, double l2)
{
    const smk_matrix* a = r.a;
    ++r.matrix_passes;
    return launch_masked_dense_f32_step(a->A, a->storage, a->ldA, a->m, a->n, r.Wt32, r.H32, r.f.H, r.f.k, r.beta, l1, l2, r.beta < 1, (float*)r.scratch,
                                        ctx().cus, r.f.st);
}

static int mf_step_w(MaskedF32Run& r, double l1, double l2)
{
    const smk_matrix* a = r.a;
    ++r.matrix_passes;
    return launch_masked_dense_f32_step(a->At, a->storage, a->ldAt, a->n, a->m, r.H32, r.Wt32, r.f.Wt, r.f.k, r.beta, l1, l2, r.beta <= 1,
                                        (float*)r.scratch, ctx().cus, r.f.st);
}

// sqrt(2 max(D, 0)) of the current factors by the fp64 masked divergence on their widenings, through the pinned slot
static int mf_error(MaskedF32Run& r, double* err)
{
    const smk_matrix* a = r.a;
    ++r.divergence_passes;
    const int rc = launch_masked_dense_divergence(a->A, a->storage, a->ldA, a->m, a->n, r.f.Wt, r.f.H, r.f.k, r.beta, r.scratch, r.out5, r.pin,
                                                  ctx().cus, r.f.st);
    if (rc) return rc;
    SMK_HIP(hipStreamSynchronize(r.f.st));
    *err = std::sqrt(2.0 * (r.pin[0] > 0.0 ? r.pin[0] : 0.0));
    return 0;
}

// masked_dense.cpp's loop: the same schedule of steps and checks
static int masked_f32_loop(MaskedF32Run& r, const smk_kl_options& o, smk_kl_stats* stats)
{
    const Penalties p(r.a->m, r.a->n, o.alpha_w, o.alpha_h, o.l1_ratio);
    double error_init = 0.0;
    int rc = mf_error(r, &error_init);
    if (rc) return rc;
    double previous = error_init, error = error_init;
    int checked = 0, it = 0, converged = 0;
    for (it = 1; it <= o.max_iter; ++it) {
        rc = mf_step_h(r, p.l1h, p.l2h);
        if (!rc && o.update_w) rc = mf_step_w(r, p.l1w, p.l2w);
        if (rc) return rc;
        if (o.tol > 0.0 && it % 10 == 0) {
            rc = mf_error(r, &error);
            if (rc) return rc;
            checked = it;
            if ((previous - error) / error_init < o.tol) { converged = 1; break; }
            previous = error;
        }
    }
    if (it > o.max_iter) it = o.max_iter;
    if (checked != it) {                        // the error of the factors that go back
        rc = mf_error(r, &error);
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

int smk_nmf_masked_dense_f32_device(const smk_matrix* a, int k, double beta, const smk_kl_options* o, void* W, int dtW, int64_t rsW, int64_t csW,
                                    void* H, int dtH, int64_t rsH, int64_t csH, void* stream, smk_kl_stats* stats)
{
    const std::string w("smk_nmf_masked_dense_f32_device");
    int rc = kl_args(w, a, k, W, dtW, H, dtH);
    if (rc) return rc;
    if (!o || !stats) { set_error(w + ": null argument"); return SMK_BAD_PARAM; }
    rc = check_penalties(w, o->alpha_w, o->alpha_h, o->l1_ratio, o->tol, o->max_iter);
    int b = 0;
    if (!rc) rc = masked_dense_beta(w, beta, &b);
    if (!rc) rc = masked_dense_supported(w, a, k, b, o->update_w != 0);
    if (rc) return rc;
    MaskedF32Run r(a, k, b);
    const DeviceView vW{W, dtW, rsW, csW}, vH{H, dtH, rsH, csH};
    rc = r.f.check(w, vW, vH, o->update_w != 0, true);
    if (rc) return rc;
    Entry e(r.f.st);
    rc = e.join(stream);
    if (!rc) rc = masked_f32_setup(r, e, o->update_w != 0, vW, vH, w);
    smk_kl_stats st{};
    if (!rc) rc = masked_f32_loop(r, *o, &st);
    g_mf_matrix_passes = r.matrix_passes;
    g_mf_divergence_passes = r.divergence_passes;
    if (!rc) rc = r.f.store(o->update_w ? &vW : nullptr, &vH);
    if (!rc) rc = e.sync();
    if (rc) return rc;
    *stats = st;
    return SMK_OK;
}

int smk_masked_dense_f32_step_time(const smk_matrix* a, int which, int k, double beta, int reps, double* ms)
{
    const std::string w("smk_masked_dense_f32_step_time");
    if (int rc = require_init()) return rc;
    if (!a || !ms || which < 0 || which > 2 || k < 1 || k > 128 || reps < 1) { set_error(w + ": bad argument"); return SMK_BAD_PARAM; }
    int b = 0;
    int rc = masked_dense_beta(w, beta, &b);
    if (rc) return rc;
    if (a->sparse || a->n != a->n_global || (which == 1 && (a->single || !a->At))) { set_error(w + ": a dense, unsharded matrix with the copy the step reads"); return SMK_UNSUPPORTED; }
    Entry e(matrix_stream(a));
    Owned& own = e.own;
    const hipStream_t st = e.st;
    const int KP = kp_of(k), KF = beta_dense_f32_pitch(k), cus = ctx().cus;
    const bool over_rows = which == 1;                        // the W side: the stored transpose, H the factor of its rows
    const i64 rows = over_rows ? a->n : a->m, cols = over_rows ? a->m : a->n;
    const void* A = over_rows ? a->At : a->A;
    const i64 ld = over_rows ? a->ldAt : a->ldA;
    double *R = nullptr, *X = nullptr, *scratch = nullptr;
    float *R32 = nullptr, *X32 = nullptr;
    rc = own.dev(&R, (size_t)KP * rows);
    if (!rc) rc = own.dev(&X, (size_t)KP * cols);
    if (!rc) rc = own.dev(&R32, (size_t)KF * rows);
    if (!rc) rc = own.dev(&X32, (size_t)KF * cols);
    if (!rc) rc = own.dev(&scratch, masked_f32_scratch_doubles(rows, cols, k, cus));
    if (rc) { set_error(w + ": no device memory"); return SMK_DEVICE_ERROR; }
    rc = launch_fill_factor_uniform(R, k, rows, 11, 0, st);
    if (!rc) rc = launch_fill_factor_uniform(X, k, cols, 12, 0, st);
    if (!rc) rc = launch_beta_dense_f32_narrow(R, R32, k, rows, st);
    if (!rc) rc = launch_beta_dense_f32_narrow(X, X32, k, cols, st);
    if (rc) return rc;
    return e.synced(time_launches(w, own, st, reps, [&]() -> int {
        if (which <= 1) return launch_masked_dense_f32_step(A, a->storage, ld, rows, cols, R32, X32, X, k, b, 0.0, 0.0, 0, (float*)scratch, cus, st);
        return launch_masked_dense_step(A, a->storage, ld, rows, cols, R, X, k, b, 0.0, 0.0, 0, scratch, cus, st);    // the fp64 masked step of the same beta
    }, ms));
}

int smk_masked_dense_f32_last_profile(int* matrix_passes, int* divergence_passes)
{
    if (matrix_passes) *matrix_passes = g_mf_matrix_passes;
    if (divergence_passes) *divergence_passes = g_mf_divergence_passes;
    return SMK_OK;
}

}  // extern "C"
