// smallk_amd/csrc/beta_dense_f32.cpp -- the fp32 form of KL (beta = 1) and Itakura-Saito (beta = 0) NMF on a resident DENSE matrix
// (include/smallk_amd.h: smk_nmf_beta_dense_f32_device).  The iteration, the schedule of checks and the refusals are
// kl_dense.cpp's and beta_dense.cpp's; what differs is where each precision applies.  Between steps the factors live as fp32
// (beta_dense_f32.hip updates them), each beside its exact fp64 widening in the FactorPair: the start is rounded once on the way
// in, the widening is what goes back to the caller, what the EXISTING fp64 divergence kernels judge -- so stats->error is, to the
// bit, the divergence of the returned factors and the stopping rule carries no fp32 noise -- and, at beta = 1, what the existing
// row-sum launch forms the denominators from.  The entries are synchronous; every workspace belongs to the smk::Entry local of
// the entry; W and H are written once, at the end: on any error they are untouched.
#include "entry.h"

#include <algorithm>
#include <cmath>
#include <string>

namespace smk {

struct BetaF32Run {
    const smk_matrix* a = nullptr;
    double beta = 0.0;
    FactorPair f;                                 // the fp64 widenings: Wt KP x m and H KP x n, k, KP, the stream
    float *Wt32 = nullptr, *H32 = nullptr;        // the factors themselves: KF x m and KF x n, KF = beta_dense_f32_pitch(k)
    double *sumsW = nullptr, *sumsH = nullptr, *part = nullptr;       // beta = 1: the row sums of the factors
    double *scratch = nullptr, *out4 = nullptr;
    double* pin = nullptr;                        // the pinned slot the host reads the divergence from (4 doubles)
    int matrix_passes = 0, divergence_passes = 0;
    BetaF32Run(const smk_matrix* a_, int k, double beta_) : a(a_), beta(beta_), f{a_->m, a_->n, k, kp_of(k), matrix_stream(a_)} {}
    bool kl() const { return beta == 1.0; }
};

// the last run of the calling thread (smk_beta_dense_f32_last_profile)
static thread_local int g_bf_matrix_passes = 0, g_bf_divergence_passes = 0;

static int beta_f32_beta(const std::string& w, double beta)
{
    if (!std::isfinite(beta) || beta < 0.0) { set_error(w + ": beta must be finite and >= 0"); return SMK_BAD_PARAM; }
    if (beta == 2.0) { set_error(w + ": beta = 2 is the Frobenius norm: smk_nmf_run, smk_nmf_cd_device"); return SMK_UNSUPPORTED; }
    if (beta != 0.0 && beta != 1.0) { set_error(w + ": the fp32 form serves beta = 0 and beta = 1; smk_nmf_beta_dense_device takes any beta"); return SMK_UNSUPPORTED; }
    return SMK_OK;
}

// the conditions of smk_nmf_beta_dense_device on the matrix and its data
static int beta_f32_supported(const std::string& w, const smk_matrix* a, int k, double beta, bool needs_transpose)
{
    if (a->sparse) { set_error(w + ": takes a dense matrix"); return SMK_UNSUPPORTED; }
    if (k > 128) { set_error(w + ": k > 128 is not supported yet"); return SMK_UNSUPPORTED; }
    if (a->n != a->n_global) { set_error(w + ": not available on a column shard"); return SMK_UNSUPPORTED; }
    if (needs_transpose && (a->single || !a->At)) {
        set_error(w + ": the W step needs the stored transpose; a single-copy matrix serves update_w = 0 only");
        return SMK_UNSUPPORTED;
    }
    const int rc = kl_dense_sign_check(a, w);
    if (rc) return rc;
    if (beta <= 0.0 && a->kl_zero) {
        set_error(w + ": beta <= 0 and the matrix stores a zero: the iteration may diverge; add a small value to the matrix or use a positive beta");
        return SMK_BAD_PARAM;
    }
    return SMK_OK;
}

// one block serves the fp32 partials of a step and the fp64 partials of the divergence
static size_t beta_f32_scratch_doubles(i64 rows, i64 cols, int k, double beta, int cus)
{
    const size_t step = (beta_dense_f32_scratch_bytes(rows, cols, k, beta, cus) + sizeof(double) - 1) / sizeof(double);
    const size_t div = beta == 1.0 ? kl_dense_scratch_elems(rows, cols, k, cus) : beta_dense_scratch_elems(rows, cols, k, cus);
    return std::max(step, div);
}

static int beta_f32_setup(BetaF32Run& r, Entry& e, bool both, const DeviceView& W, const DeviceView& H, const std::string& who)
{
    Owned& own = e.own;
    const int KP = r.f.KP, KF = beta_dense_f32_pitch(r.f.k), cus = ctx().cus;
    const i64 m = r.a->m, n = r.a->n, nmax = m > n ? m : n;
    const size_t sa = beta_f32_scratch_doubles(m, n, r.f.k, r.beta, cus), sat = both ? beta_f32_scratch_doubles(n, m, r.f.k, r.beta, cus) : 0;
    int rc = own.dev(&r.scratch, std::max(sa, sat));
    if (!rc) rc = own.dev(&r.Wt32, (size_t)KF * m);
    if (!rc) rc = own.dev(&r.H32, (size_t)KF * n);
    if (!rc) rc = own.dev(&r.out4, 4);
    if (!rc && r.kl()) {
        rc = own.dev(&r.sumsW, (size_t)KP);
        if (!rc) rc = own.dev(&r.sumsH, (size_t)KP);
        if (!rc) rc = own.dev(&r.part, (size_t)kl_sums_blocks(nmax) * KP);
    }
    if (!rc) rc = own.pinned((void**)&r.pin, 4 * sizeof(double));
    if (rc) { set_error(who + ": no memory for the factor workspace"); return SMK_DEVICE_ERROR; }
    rc = r.f.alloc_zeroed(own, who);
    if (!rc) rc = r.f.load(W, H);
    // the one rounding on the way in; from here on the FactorPair holds the widening of the fp32 factors
    if (!rc) rc = launch_beta_dense_f32_narrow(r.f.Wt, r.Wt32, r.f.k, m, r.f.st);
    if (!rc) rc = launch_beta_dense_f32_narrow(r.f.H, r.H32, r.f.k, n, r.f.st);
    return rc;
}

static int bf_sums_w(BetaF32Run& r) { return r.kl() ? launch_kl_factor_sums(r.f.Wt, r.f.k, r.a->m, r.part, r.sumsW, r.f.st) : 0; }
static int bf_sums_h(BetaF32Run& r) { return r.kl() ? launch_kl_factor_sums(r.f.H, r.f.k, r.a->n, r.part, r.sumsH, r.f.st) : 0; }

// the flushes are those of the fp64 forms: at beta = 1 the W side alone, at beta = 0 both
static int bf_step_h(BetaF32Run& r, double l1, double l2)
{
    const smk_matrix* a = r.a;
    ++r.matrix_passes;
    return launch_beta_dense_f32_step(a->A, a->storage, a->ldA, a->m, a->n, r.Wt32, r.H32, r.f.H, r.f.k, r.beta, r.sumsW, 0, l1, l2, r.kl() ? 0 : 1,
                                      (float*)r.scratch, ctx().cus, r.f.st);
}

static int bf_step_w(BetaF32Run& r, double l1, double l2)
{
    const smk_matrix* a = r.a;
    ++r.matrix_passes;
    return launch_beta_dense_f32_step(a->At, a->storage, a->ldAt, a->n, a->m, r.H32, r.Wt32, r.f.Wt, r.f.k, r.beta, r.sumsH, 1, l1, l2, 1,
                                      (float*)r.scratch, ctx().cus, r.f.st);
}

// sqrt(2 max(D, 0)) of the current factors by the fp64 divergence kernels on their widenings, through the pinned slot
static int bf_error(BetaF32Run& r, double* err)
{
    const smk_matrix* a = r.a;
    ++r.divergence_passes;
    const int rc = r.kl() ? launch_kl_dense_divergence(a->A, a->storage, a->ldA, a->m, a->n, r.f.Wt, r.f.H, r.f.k, r.sumsW, r.sumsH, r.scratch, r.out4,
                                                       r.pin, ctx().cus, r.f.st)
                          : launch_beta_dense_divergence(a->A, a->storage, a->ldA, a->m, a->n, r.f.Wt, r.f.H, r.f.k, r.beta, r.scratch, r.out4, r.pin,
                                                         ctx().cus, r.f.st);
    if (rc) return rc;
    SMK_HIP(hipStreamSynchronize(r.f.st));
    *err = std::sqrt(2.0 * (r.pin[0] > 0.0 ? r.pin[0] : 0.0));
    return 0;
}

// kl_dense.cpp's loop (beta = 0: without the factor sums, as beta_dense.cpp's)
static int beta_f32_loop(BetaF32Run& r, const smk_kl_options& o, smk_kl_stats* stats)
{
    const Penalties p(r.a->m, r.a->n, o.alpha_w, o.alpha_h, o.l1_ratio);
    int rc = bf_sums_w(r);                      // update_w = 0: formed once
    if (!rc) rc = bf_sums_h(r);
    double error_init = 0.0;
    if (!rc) rc = bf_error(r, &error_init);
    if (rc) return rc;
    double previous = error_init, error = error_init;
    int checked = 0, it = 0, converged = 0;
    for (it = 1; it <= o.max_iter; ++it) {
        rc = bf_step_h(r, p.l1h, p.l2h);
        if (!rc && o.update_w) {
            rc = bf_sums_h(r);
            if (!rc) rc = bf_step_w(r, p.l1w, p.l2w);
            if (!rc) rc = bf_sums_w(r);
        }
        if (rc) return rc;
        if (o.tol > 0.0 && it % 10 == 0) {
            if (!o.update_w) rc = bf_sums_h(r);
            if (!rc) rc = bf_error(r, &error);
            if (rc) return rc;
            checked = it;
            if ((previous - error) / error_init < o.tol) { converged = 1; break; }
            previous = error;
        }
    }
    if (it > o.max_iter) it = o.max_iter;
    if (checked != it) {                        // the error of the factors that go back
        if (!o.update_w) rc = bf_sums_h(r);
        if (!rc) rc = bf_error(r, &error);
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

int smk_nmf_beta_dense_f32_device(const smk_matrix* a, int k, double beta, const smk_kl_options* o, void* W, int dtW, int64_t rsW, int64_t csW,
                                  void* H, int dtH, int64_t rsH, int64_t csH, void* stream, smk_kl_stats* stats)
{
    const std::string w("smk_nmf_beta_dense_f32_device");
    int rc = kl_args(w, a, k, W, dtW, H, dtH);
    if (rc) return rc;
    if (!o || !stats) { set_error(w + ": null argument"); return SMK_BAD_PARAM; }
    rc = check_penalties(w, o->alpha_w, o->alpha_h, o->l1_ratio, o->tol, o->max_iter);
    if (!rc) rc = beta_f32_beta(w, beta);
    if (!rc) rc = beta_f32_supported(w, a, k, beta, o->update_w != 0);
    if (rc) return rc;
    BetaF32Run r(a, k, beta);
    const DeviceView vW{W, dtW, rsW, csW}, vH{H, dtH, rsH, csH};
    rc = r.f.check(w, vW, vH, o->update_w != 0, true);
    if (rc) return rc;
    Entry e(r.f.st);
    rc = e.join(stream);
    if (!rc) rc = beta_f32_setup(r, e, o->update_w != 0, vW, vH, w);
    smk_kl_stats st{};
    if (!rc) rc = beta_f32_loop(r, *o, &st);
    g_bf_matrix_passes = r.matrix_passes;
    g_bf_divergence_passes = r.divergence_passes;
    if (!rc) rc = r.f.store(o->update_w ? &vW : nullptr, &vH);
    if (!rc) rc = e.sync();
    if (rc) return rc;
    *stats = st;
    return SMK_OK;
}

int smk_beta_dense_f32_step_time(const smk_matrix* a, int which, int k, double beta, int reps, double* ms)
{
    const std::string w("smk_beta_dense_f32_step_time");
    if (int rc = require_init()) return rc;
    if (!a || !ms || which < 0 || which > 3 || k < 1 || reps < 1) { set_error(w + ": bad argument"); return SMK_BAD_PARAM; }
    int rc = beta_f32_beta(w, beta);
    if (!rc) rc = beta_f32_supported(w, a, k, beta, which == 1);
    if (rc) return rc;
    Entry e(matrix_stream(a));
    Owned& own = e.own;
    const hipStream_t st = e.st;
    const int KP = kp_of(k), KF = beta_dense_f32_pitch(k), cus = ctx().cus;
    const bool over_rows = which == 1;                        // the W side: the stored transpose, H the factor of its rows
    const i64 rows = over_rows ? a->n : a->m, cols = over_rows ? a->m : a->n;
    const void* A = over_rows ? a->At : a->A;
    const i64 ld = over_rows ? a->ldAt : a->ldA;
    double *R = nullptr, *X = nullptr, *sums = nullptr, *part = nullptr, *scratch = nullptr, *col_r = nullptr, *col_a = nullptr, *out2 = nullptr;
    float *R32 = nullptr, *X32 = nullptr;
    const size_t s = std::max(beta_f32_scratch_doubles(rows, cols, k, beta, cus), residual_dense_scratch_elems(rows, cols, cus));
    rc = own.dev(&R, (size_t)KP * rows);
    if (!rc) rc = own.dev(&X, (size_t)KP * cols);
    if (!rc) rc = own.dev(&R32, (size_t)KF * rows);
    if (!rc) rc = own.dev(&X32, (size_t)KF * cols);
    if (!rc) rc = own.dev(&sums, (size_t)KP);
    if (!rc) rc = own.dev(&part, (size_t)kl_sums_blocks(rows) * KP);
    if (!rc) rc = own.dev(&scratch, s);
    if (!rc) rc = own.dev(&col_r, (size_t)cols);
    if (!rc) rc = own.dev(&col_a, (size_t)cols);
    if (!rc) rc = own.dev(&out2, 2);
    if (rc) { set_error(w + ": no device memory"); return SMK_DEVICE_ERROR; }
    rc = launch_fill_factor_uniform(R, k, rows, 11, 0, st);
    if (!rc) rc = launch_fill_factor_uniform(X, k, cols, 12, 0, st);
    if (!rc) rc = launch_beta_dense_f32_narrow(R, R32, k, rows, st);
    if (!rc) rc = launch_beta_dense_f32_narrow(X, X32, k, cols, st);
    if (!rc) rc = launch_kl_factor_sums(R, k, rows, part, sums, st);
    if (rc) return rc;
    return e.synced(time_launches(w, own, st, reps, [&]() -> int {
        if (which <= 1) return launch_beta_dense_f32_step(A, a->storage, ld, rows, cols, R32, X32, X, k, beta, sums, 0, 0.0, 0.0, 0, (float*)scratch, cus, st);
        if (which == 2) {
            if (beta == 1.0) return launch_kl_dense_step(A, a->storage, ld, rows, cols, R, X, k, sums, 0, 0.0, 0.0, 0, scratch, cus, st);
            return launch_beta_dense_step(A, a->storage, ld, rows, cols, R, X, k, beta, 0.0, 0.0, 0, scratch, cus, st);
        }
        return launch_residual_dense(A, a->storage, ld, rows, cols, R, X, KP, k, scratch, col_r, col_a, out2, cus, st);
    }, ms));
}

int smk_beta_dense_f32_last_profile(int* matrix_passes, int* divergence_passes)
{
    if (matrix_passes) *matrix_passes = g_bf_matrix_passes;
    if (divergence_passes) *divergence_passes = g_bf_divergence_passes;
    return SMK_OK;
}

}  // extern "C"
