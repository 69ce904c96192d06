// smallk_amd/csrc/beta_dense.cpp -- NMF of a resident DENSE matrix under a beta-divergence by multiplicative updates
// (include/smallk_amd.h: smk_nmf_beta_dense_device, smk_matrix_beta_divergence_dense_device): scikit-learn's
// solver="mu" for beta_loss = "itakura-saito" (beta = 0) and every other beta >= 0 but 2; beta = 1 is kl_dense.cpp's and is forwarded
// there.  The shape is kl_dense.cpp's: each half-iteration is one streaming read of one stored copy by beta_dense.hip -- A for the H
// step, the stored transpose for the W step --, but the denominators come out of the same pass, so no factor sums are kept.  The
// entries are synchronous; every workspace belongs to the smk::Entry local of the entry; of the matrix handle only the
// once-per-contents sign record is written.  W and H are written once, at the end: on any error they are untouched.  The pinned
// slot is read on check iterations only.
#include "entry.h"

#include <algorithm>
#include <cmath>
#include <string>

namespace smk {

struct BetaDenseRun {
    const smk_matrix* a = nullptr;
    double beta = 0.0;
    FactorPair f;                                 // the factors: Wt KP x m and H KP x n, k, KP, the stream
    double *scratch = nullptr, *out4 = nullptr;
    double* pin = nullptr;                        // the pinned slot the host reads the divergence from (4 doubles)
    int matrix_passes = 0, divergence_passes = 0;
    BetaDenseRun(const smk_matrix* a_, int k, double beta_) : a(a_), beta(beta_), f{a_->m, a_->n, k, kp_of(k), matrix_stream(a_)} {}
};

// the last run of the calling thread (smk_beta_dense_last_profile)
static thread_local int g_bd_matrix_passes = 0, g_bd_divergence_passes = 0;

// beta itself: finite and >= 0 (SMK_BAD_PARAM), not 2 (SMK_UNSUPPORTED)
static int beta_dense_beta(const std::string& w, double beta)
{
    if (!std::isfinite(beta) || beta < 0.0) { set_error(w + ": beta must be finite and >= 0"); return SMK_BAD_PARAM; }
    if (beta == 2.0) { set_error(w + ": beta = 2 is the Frobenius norm: smk_nmf_run, smk_nmf_cd_device"); return SMK_UNSUPPORTED; }
    return SMK_OK;
}

// kl_dense.cpp's conditions on the matrix, then the data: no negative value, and no zero when beta <= 0
static int beta_dense_supported(const std::string& w, const smk_matrix* a, int k, double beta, bool needs_transpose)
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

static int beta_dense_setup(BetaDenseRun& r, Entry& e, bool both, const DeviceView& W, const DeviceView& H, const std::string& who)
{
    Owned& own = e.own;
    const size_t sa = beta_dense_scratch_elems(r.a->m, r.a->n, r.f.k, ctx().cus);
    const size_t sat = both ? beta_dense_scratch_elems(r.a->n, r.a->m, r.f.k, ctx().cus) : 0;
    int rc = own.dev(&r.scratch, sa > sat ? sa : sat);
    if (!rc) rc = own.dev(&r.out4, 4);
    if (!rc) rc = own.pinned((void**)&r.pin, 4 * sizeof(double));
    if (rc) { set_error(who + ": no memory for the factor workspace"); return SMK_DEVICE_ERROR; }
    rc = r.f.alloc_zeroed(own, who);
    return rc ? rc : r.f.load(W, H);
}

// the flushes: scikit-learn's W (our H) below 2^-52 becomes 0 when beta < 1, its H (our W) when beta <= 1; beta = 1 is not served
// here, so both sides flush below 1 and neither above
static int bd_step_h(BetaDenseRun& r, double l1, double l2)
{
    const smk_matrix* a = r.a;
    ++r.matrix_passes;
    return launch_beta_dense_step(a->A, a->storage, a->ldA, a->m, a->n, r.f.Wt, r.f.H, r.f.k, r.beta, l1, l2, r.beta < 1.0, r.scratch, ctx().cus, r.f.st);
}

static int bd_step_w(BetaDenseRun& r, double l1, double l2)
{
    const smk_matrix* a = r.a;
    ++r.matrix_passes;
    return launch_beta_dense_step(a->At, a->storage, a->ldAt, a->n, a->m, r.f.H, r.f.Wt, r.f.k, r.beta, l1, l2, r.beta < 1.0, r.scratch, ctx().cus,
                                  r.f.st);
}

// out[0 .. 3] = D and the three sums it is formed from, through the pinned slot: one synchronisation
static int bd_divergence(BetaDenseRun& r, double* out)
{
    const smk_matrix* a = r.a;
    ++r.divergence_passes;
    const int rc = launch_beta_dense_divergence(a->A, a->storage, a->ldA, a->m, a->n, r.f.Wt, r.f.H, r.f.k, r.beta, r.scratch, r.out4, r.pin, ctx().cus,
                                                r.f.st);
    if (rc) return rc;
    SMK_HIP(hipStreamSynchronize(r.f.st));
    for (int i = 0; i < 4; ++i) out[i] = r.pin[i];
    return 0;
}

static int bd_error(BetaDenseRun& r, double* err)
{
    double d[4];
    const int rc = bd_divergence(r, d);
    if (rc) return rc;
    *err = std::sqrt(2.0 * (d[0] > 0.0 ? d[0] : 0.0));
    return 0;
}

// kl_dense.cpp's loop without the factor sums: the same schedule of steps and checks
static int beta_dense_loop(BetaDenseRun& r, const smk_kl_options& o, smk_kl_stats* stats)
{
    const Penalties p(r.a->m, r.a->n, o.alpha_w, o.alpha_h, o.l1_ratio);
    double error_init = 0.0;
    int rc = bd_error(r, &error_init);
    if (rc) return rc;
    double previous = error_init, error = error_init;
    int checked = 0, it = 0, converged = 0;
    for (it = 1; it <= o.max_iter; ++it) {
        rc = bd_step_h(r, p.l1h, p.l2h);
        if (!rc && o.update_w) rc = bd_step_w(r, p.l1w, p.l2w);
        if (rc) return rc;
        if (o.tol > 0.0 && it % 10 == 0) {
            rc = bd_error(r, &error);
            if (rc) return rc;
            checked = it;
            if ((previous - error) / error_init < o.tol) { converged = 1; break; }
            previous = error;
        }
    }
    if (it > o.max_iter) it = o.max_iter;
    if (checked != it) {                        // the error of the factors that go back
        rc = bd_error(r, &error);
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

int smk_nmf_beta_dense_device(const smk_matrix* a, int k, double beta, const smk_kl_options* o, void* W, int dtW, int64_t rsW, int64_t csW, void* H,
                              int dtH, int64_t rsH, int64_t csH, void* stream, smk_kl_stats* stats)
{
    const std::string w("smk_nmf_beta_dense_device");
    int rc = kl_args(w, a, k, W, dtW, H, dtH);
    if (rc) return rc;
    if (!o || !stats) { set_error(w + ": null argument"); return SMK_BAD_PARAM; }
    rc = check_penalties(w, o->alpha_w, o->alpha_h, o->l1_ratio, o->tol, o->max_iter);
    if (!rc) rc = beta_dense_beta(w, beta);
    if (rc) return rc;
    if (beta == 1.0) return smk_nmf_kl_dense_device(a, k, o, W, dtW, rsW, csW, H, dtH, rsH, csH, stream, stats);
    rc = beta_dense_supported(w, a, k, beta, o->update_w != 0);
    if (rc) return rc;
    BetaDenseRun r(a, k, beta);
    const DeviceView vW{W, dtW, rsW, csW}, vH{H, dtH, rsH, csH};
    rc = r.f.check(w, vW, vH, o->update_w != 0, true);
    if (rc) return rc;
    Entry e(r.f.st);
    rc = e.join(stream);
    if (!rc) rc = beta_dense_setup(r, e, o->update_w != 0, vW, vH, w);
    smk_kl_stats st{};
    if (!rc) rc = beta_dense_loop(r, *o, &st);
    g_bd_matrix_passes = r.matrix_passes;
    g_bd_divergence_passes = r.divergence_passes;
    if (!rc) rc = r.f.store(o->update_w ? &vW : nullptr, &vH);
    if (!rc) rc = e.sync();
    if (rc) return rc;
    *stats = st;
    return SMK_OK;
}

int smk_matrix_beta_divergence_dense_device(const smk_matrix* a, int k, double beta, const void* W, int dtW, int64_t rsW, int64_t csW, const void* H,
                                            int dtH, int64_t rsH, int64_t csH, void* stream, double* out)
{
    const std::string w("smk_matrix_beta_divergence_dense_device");
    int rc = kl_args(w, a, k, W, dtW, H, dtH);
    if (rc) return rc;
    if (!out) { set_error(w + ": null output"); return SMK_BAD_PARAM; }
    rc = beta_dense_beta(w, beta);
    if (rc) return rc;
    if (beta == 1.0) {                          // D, sum a log(a / d), sum WH; the fourth slot has no KL counterpart
        out[3] = 0.0;
        return smk_matrix_kl_divergence_dense_device(a, k, W, dtW, rsW, csW, H, dtH, rsH, csH, stream, out);
    }
    rc = beta_dense_supported(w, a, k, beta, false);
    if (rc) return rc;
    BetaDenseRun r(a, k, beta);
    const DeviceView vW = DeviceView::in(W, dtW, rsW, csW), vH = DeviceView::in(H, dtH, rsH, csH);
    rc = r.f.check(w, vW, vH, false, false);
    if (rc) return rc;
    Entry e(r.f.st);
    rc = e.join(stream);
    if (!rc) rc = beta_dense_setup(r, e, false, vW, vH, w);
    double d[4] = {0.0, 0.0, 0.0, 0.0};
    if (!rc) rc = e.synced(bd_divergence(r, d));
    if (rc) return rc;
    for (int i = 0; i < 4; ++i) out[i] = d[i];
    return SMK_OK;
}

int smk_beta_dense_step_time(const smk_matrix* a, int which, int k, double beta, int reps, double* ms)
{
    const std::string w("smk_beta_dense_step_time");
    if (int rc = require_init()) return rc;
    if (!a || !ms || which < 0 || which > 3 || k < 1 || reps < 1) { set_error(w + ": bad argument"); return SMK_BAD_PARAM; }
    int rc = beta_dense_beta(w, beta);
    if (!rc && beta == 1.0) { set_error(w + ": beta = 1 is smk_kl_dense_step_time's"); rc = SMK_BAD_PARAM; }
    if (!rc) rc = beta_dense_supported(w, a, k, beta, which == 1);
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
    size_t s = beta_dense_scratch_elems(rows, cols, k, cus);
    s = std::max(s, kl_dense_scratch_elems(rows, cols, k, cus));
    s = std::max(s, residual_dense_scratch_elems(rows, cols, cus));
    rc = own.dev(&R, (size_t)KP * rows);
    if (!rc) rc = own.dev(&X, (size_t)KP * cols);
    if (!rc) rc = own.dev(&sums, (size_t)KP);
    if (!rc) rc = own.dev(&part, (size_t)kl_sums_blocks(rows) * KP);
    if (!rc) rc = own.dev(&scratch, s);
    if (!rc) rc = own.dev(&col_r, (size_t)cols);
    if (!rc) rc = own.dev(&col_a, (size_t)cols);
    if (!rc) rc = own.dev(&out2, 2);
    if (rc) { set_error(w + ": no device memory"); return SMK_DEVICE_ERROR; }
    rc = launch_fill_factor_uniform(R, k, rows, 11, 0, st);
    if (!rc) rc = launch_fill_factor_uniform(X, k, cols, 12, 0, st);
    if (!rc) rc = launch_kl_factor_sums(R, k, rows, part, sums, st);
    if (rc) return rc;
    return e.synced(time_launches(w, own, st, reps, [&]() -> int {
        if (which <= 1) return launch_beta_dense_step(A, a->storage, ld, rows, cols, R, X, k, beta, 0.0, 0.0, 0, scratch, cus, st);
        if (which == 2) return launch_kl_dense_step(A, a->storage, ld, rows, cols, R, X, k, sums, 0, 0.0, 0.0, 0, scratch, cus, st);
        return launch_residual_dense(A, a->storage, ld, rows, cols, R, X, KP, k, scratch, col_r, col_a, out2, cus, st);
    }, ms));
}

int smk_beta_dense_last_profile(int* matrix_passes, int* divergence_passes)
{
    if (matrix_passes) *matrix_passes = g_bd_matrix_passes;
    if (divergence_passes) *divergence_passes = g_bd_divergence_passes;
    return SMK_OK;
}

}  // extern "C"
