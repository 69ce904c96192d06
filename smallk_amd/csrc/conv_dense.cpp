// smallk_amd/csrc/conv_dense.cpp -- convolutive NMF of a resident DENSE matrix under the Kullback-Leibler or the Itakura-Saito
// divergence by multiplicative updates (include/smallk_amd.h: smk_nmf_conv_dense_device, smk_matrix_conv_divergence_dense_device;
// DESIGN.md 27): a component is a pattern of T consecutive columns, A ~ sum_t W_t shift_t(H).  The shape is beta_dense.cpp's: each
// half-iteration is one streaming read of one stored copy by conv_dense.hip -- A for the H step, the stored transpose for the W
// step -- and numerators and denominators come out of the same pass.  The entries are synchronous; every workspace belongs to the
// smk::Entry local of the entry; of the matrix handle only the once-per-contents sign record is written.  W and H are written once,
// at the end: on any error they are untouched.  The pinned slot is read on check iterations only.
#include "conv_dense.h"
#include "entry.h"

#include <cmath>
#include <string>

namespace smk {

struct ConvDenseRun {
    const smk_matrix* a = nullptr;
    int k, T, KP4, beta;
    hipStream_t st;
    double *Wc = nullptr, *Hc = nullptr;           // m x T KP4 and KP4 x n (conv_dense.h)
    double *scratch = nullptr, *out4 = nullptr;
    double* pin = nullptr;                        // the pinned slot the host reads the divergence from (4 doubles)
    int matrix_passes = 0, divergence_passes = 0;
    ConvDenseRun(const smk_matrix* a_, int k_, int T_, int beta_) : a(a_), k(k_), T(T_), KP4(conv_kp4(k_)), beta(beta_), st(matrix_stream(a_)) {}
    // slice t of W (m x k) and H (k x n) in the workspaces
    DeviceView slice(int t) const { return DeviceView::rows(Wc + (size_t)t * KP4, (i64)T * KP4); }
    DeviceView h() const { return DeviceView::cols(Hc, KP4); }
};

// slice t of the caller's W: ss elements further per slice
static DeviceView conv_slice(const DeviceView& W, i64 ss, int t)
{
    return {(char*)W.p + (size_t)t * ss * (W.dtype == SMK_DT_F64 ? 8 : 4), W.dtype, W.rs, W.cs};
}

// the last run of the calling thread (smk_conv_dense_last_profile)
static thread_local int g_cv_matrix_passes = 0, g_cv_divergence_passes = 0;

// T and beta themselves.  SMK_BAD_PARAM: T < 1, T > n, a beta that is negative or not finite; SMK_UNSUPPORTED: T roundup(k, 4) > 128
// (the inner dimension of the product), a beta other than 0 and 1
static int conv_dense_shape(const std::string& w, const smk_matrix* a, int k, int T, double beta, int* beta_out)
{
    if (T < 1) { set_error(w + ": T < 1"); return SMK_BAD_PARAM; }
    if (T > a->n_global) { set_error(w + ": T exceeds the number of columns"); return SMK_BAD_PARAM; }
    if (!std::isfinite(beta) || beta < 0.0) { set_error(w + ": beta must be finite and >= 0"); return SMK_BAD_PARAM; }
    if (beta != 0.0 && beta != 1.0) { set_error(w + ": beta must be 0 (Itakura-Saito) or 1 (Kullback-Leibler)"); return SMK_UNSUPPORTED; }
    if ((i64)T * conv_kp4(k) > 128) { set_error(w + ": T * roundup(k, 4) > 128 is not supported"); return SMK_UNSUPPORTED; }
    *beta_out = (int)beta;
    return SMK_OK;
}

// beta_dense.cpp's conditions on the matrix, then the data: no negative value, and no zero at beta = 0
static int conv_dense_supported(const std::string& w, const smk_matrix* a, int beta, bool needs_transpose)
{
    if (a->sparse) { set_error(w + ": takes a dense matrix"); return SMK_UNSUPPORTED; }
    if (a->n != a->n_global) { set_error(w + ": not available on a column shard"); return SMK_UNSUPPORTED; }
    if (needs_transpose && (a->single || !a->At)) {
        set_error(w + ": the W step needs the stored transpose; a single-copy matrix serves update_w = 0 only");
        return SMK_UNSUPPORTED;
    }
    const int rc = kl_dense_sign_check(a, w);
    if (rc) return rc;
    if (beta == 0 && a->kl_zero) {
        set_error(w + ": beta = 0 and the matrix stores a zero: the iteration may diverge; add a small value to the matrix or use beta = 1");
        return SMK_BAD_PARAM;
    }
    return SMK_OK;
}

// every slice of W (ss elements apart) and H as views of the caller's memory
static int conv_dense_check_views(const std::string& w, const ConvDenseRun& r, const DeviceView& W, i64 ss, const DeviceView& H, bool writeW, bool writeH)
{
    if (ss < 0) { set_error(w + "(W): negative stride"); return SMK_BAD_PARAM; }
    if (writeW && r.T > 1 && ss == 0) { set_error(w + "(W): the elements of an output overlap"); return SMK_BAD_PARAM; }
    for (int t = 0; t < r.T; ++t) {
        const DeviceView s = conv_slice(W, ss, t);
        const int rc = check_device_view(s.p, s.dtype, r.a->m, r.k, s.rs, s.cs, writeW, (w + "(W)").c_str());
        if (rc) return rc;
    }
    return check_device_view(H.p, H.dtype, r.k, r.a->n, H.rs, H.cs, writeH, (w + "(H)").c_str());
}

// the scratch, the zeroed factor workspaces (pad entries must be, and stay, zero) and the views converted in
static int conv_dense_setup(ConvDenseRun& r, Entry& e, const DeviceView& W, i64 ss, const DeviceView& H, const std::string& who)
{
    Owned& own = e.own;
    const size_t we = (size_t)r.a->m * r.T * r.KP4, he = (size_t)r.a->n * r.KP4;
    int rc = own.dev(&r.scratch, conv_dense_scratch_elems(r.a->m, r.a->n, r.k, r.T, ctx().cus));
    if (!rc) rc = own.dev(&r.out4, 4);
    if (!rc) rc = own.pinned((void**)&r.pin, 4 * sizeof(double));
    if (!rc) rc = own.dev(&r.Wc, we);
    if (!rc) rc = own.dev(&r.Hc, he);
    if (rc) { set_error(who + ": no memory for the factor workspace"); return SMK_DEVICE_ERROR; }
    SMK_HIP(hipMemsetAsync(r.Wc, 0, we * sizeof(double), r.st));
    SMK_HIP(hipMemsetAsync(r.Hc, 0, he * sizeof(double), r.st));
    for (int t = 0; t < r.T && !rc; ++t) rc = convert_view(conv_slice(W, ss, t), r.slice(t), r.a->m, r.k, r.st);
    return rc ? rc : convert_view(H, r.h(), r.k, r.a->n, r.st);
}

static int conv_dense_store(const ConvDenseRun& r, const DeviceView* W, i64 ss, const DeviceView& H)
{
    int rc = 0;
    for (int t = 0; W && t < r.T && !rc; ++t) rc = convert_view(r.slice(t), conv_slice(*W, ss, t), r.a->m, r.k, r.st);
    return rc ? rc : convert_view(r.h(), H, r.k, r.a->n, r.st);
}

// the flushes are nmf_kl_dense's at beta = 1 (W only) and nmf_beta_dense's at beta = 0 (both sides)
static int cv_step_h(ConvDenseRun& r, double l1, double l2)
{
    const smk_matrix* a = r.a;
    ++r.matrix_passes;
    return launch_conv_dense_step(a->A, a->storage, a->ldA, a->m, a->n, 0, r.Wc, r.Hc, r.k, r.T, r.beta, l1, l2, r.beta == 0, r.scratch, ctx().cus, r.st);
}

static int cv_step_w(ConvDenseRun& r, double l1, double l2)
{
    const smk_matrix* a = r.a;
    ++r.matrix_passes;
    return launch_conv_dense_step(a->At, a->storage, a->ldAt, a->m, a->n, 1, r.Wc, r.Hc, r.k, r.T, r.beta, l1, l2, 1, r.scratch, ctx().cus, r.st);
}

// out[0 .. 3] = D and the sums it is formed from, through the pinned slot: one synchronisation
static int cv_divergence(ConvDenseRun& r, double* out)
{
    const smk_matrix* a = r.a;
    ++r.divergence_passes;
    const int rc = launch_conv_dense_divergence(a->A, a->storage, a->ldA, a->m, a->n, r.Wc, r.Hc, r.k, r.T, r.beta, r.scratch, r.out4, r.pin, ctx().cus, r.st);
    if (rc) return rc;
    SMK_HIP(hipStreamSynchronize(r.st));
    for (int i = 0; i < 4; ++i) out[i] = r.pin[i];
    return 0;
}

static int cv_error(ConvDenseRun& r, double* err)
{
    double d[4];
    const int rc = cv_divergence(r, d);
    if (rc) return rc;
    *err = std::sqrt(2.0 * (d[0] > 0.0 ? d[0] : 0.0));
    return 0;
}

// beta_dense.cpp's loop: the same schedule of steps and checks
static int conv_dense_loop(ConvDenseRun& r, const smk_kl_options& o, smk_kl_stats* stats)
{
    const Penalties p(r.a->m, r.a->n, o.alpha_w, o.alpha_h, o.l1_ratio);
    double error_init = 0.0;
    int rc = cv_error(r, &error_init);
    if (rc) return rc;
    double previous = error_init, error = error_init;
    int checked = 0, it = 0, converged = 0;
    for (it = 1; it <= o.max_iter; ++it) {
        rc = cv_step_h(r, p.l1h, p.l2h);
        if (!rc && o.update_w) rc = cv_step_w(r, p.l1w, p.l2w);
        if (rc) return rc;
        if (o.tol > 0.0 && it % 10 == 0) {
            rc = cv_error(r, &error);
            if (rc) return rc;
            checked = it;
            if ((previous - error) / error_init < o.tol) { converged = 1; break; }
            previous = error;
        }
    }
    if (it > o.max_iter) it = o.max_iter;
    if (checked != it) {                        // the error of the factors that go back
        rc = cv_error(r, &error);
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

int smk_nmf_conv_dense_device(const smk_matrix* a, int k, int T, double beta, const smk_kl_options* o, void* W, int dtW, int64_t ssW, int64_t rsW,
                              int64_t csW, void* H, int dtH, int64_t rsH, int64_t csH, void* stream, smk_kl_stats* stats)
{
    const std::string w("smk_nmf_conv_dense_device");
    int rc = kl_args(w, a, k, W, dtW, H, dtH);
    if (rc) return rc;
    if (!o || !stats) { set_error(w + ": null argument"); return SMK_BAD_PARAM; }
    rc = check_penalties(w, o->alpha_w, o->alpha_h, o->l1_ratio, o->tol, o->max_iter);
    int b = 0;
    if (!rc) rc = conv_dense_shape(w, a, k, T, beta, &b);
    if (!rc) rc = conv_dense_supported(w, a, b, o->update_w != 0);
    if (rc) return rc;
    ConvDenseRun r(a, k, T, b);
    const DeviceView vW{W, dtW, rsW, csW}, vH{H, dtH, rsH, csH};
    rc = conv_dense_check_views(w, r, vW, ssW, vH, o->update_w != 0, true);
    if (rc) return rc;
    Entry e(r.st);
    rc = e.join(stream);
    if (!rc) rc = conv_dense_setup(r, e, vW, ssW, vH, w);
    smk_kl_stats st{};
    if (!rc) rc = conv_dense_loop(r, *o, &st);
    g_cv_matrix_passes = r.matrix_passes;
    g_cv_divergence_passes = r.divergence_passes;
    if (!rc) rc = conv_dense_store(r, o->update_w ? &vW : nullptr, ssW, vH);
    if (!rc) rc = e.sync();
    if (rc) return rc;
    *stats = st;
    return SMK_OK;
}

int smk_matrix_conv_divergence_dense_device(const smk_matrix* a, int k, int T, double beta, const void* W, int dtW, int64_t ssW, int64_t rsW,
                                            int64_t csW, const void* H, int dtH, int64_t rsH, int64_t csH, void* stream, double* out)
{
    const std::string w("smk_matrix_conv_divergence_dense_device");
    int rc = kl_args(w, a, k, W, dtW, H, dtH);
    if (rc) return rc;
    if (!out) { set_error(w + ": null output"); return SMK_BAD_PARAM; }
    int b = 0;
    rc = conv_dense_shape(w, a, k, T, beta, &b);
    if (!rc) rc = conv_dense_supported(w, a, b, false);
    if (rc) return rc;
    ConvDenseRun r(a, k, T, b);
    const DeviceView vW = DeviceView::in(W, dtW, rsW, csW), vH = DeviceView::in(H, dtH, rsH, csH);
    rc = conv_dense_check_views(w, r, vW, ssW, vH, false, false);
    if (rc) return rc;
    Entry e(r.st);
    rc = e.join(stream);
    if (!rc) rc = conv_dense_setup(r, e, vW, ssW, vH, w);
    double d[4] = {0.0, 0.0, 0.0, 0.0};
    if (!rc) rc = e.synced(cv_divergence(r, d));
    if (rc) return rc;
    for (int i = 0; i < 4; ++i) out[i] = d[i];
    return SMK_OK;
}

int smk_conv_dense_step_time(const smk_matrix* a, int which, int k, int T, double beta, int reps, double* ms)
{
    const std::string w("smk_conv_dense_step_time");
    if (int rc = require_init()) return rc;
    if (!a || !ms || which < 0 || which > 1 || k < 1 || reps < 1) { set_error(w + ": bad argument"); return SMK_BAD_PARAM; }
    int b = 0;
    int rc = conv_dense_shape(w, a, k, T, beta, &b);
    if (!rc) rc = conv_dense_supported(w, a, b, which == 1);
    if (rc) return rc;
    // the synthetic factors are launch_fill_factor_uniform's, whose pitch is kp_of: served where that is this layout's pitch
    const int KP4 = conv_kp4(k), KR = T * KP4;
    if (kp_of(k) != KP4 || kp_of(KR) != KR) { set_error(w + ": k and T * k must be 8, 16, 32, 64 or 128"); return SMK_BAD_PARAM; }
    Entry e(matrix_stream(a));
    Owned& own = e.own;
    const hipStream_t st = e.st;
    double *Wc = nullptr, *Hc = nullptr, *scratch = nullptr;
    rc = own.dev(&Wc, (size_t)KR * a->m);
    if (!rc) rc = own.dev(&Hc, (size_t)KP4 * a->n);
    if (!rc) rc = own.dev(&scratch, conv_dense_scratch_elems(a->m, a->n, k, T, ctx().cus));
    if (rc) { set_error(w + ": no device memory"); return SMK_DEVICE_ERROR; }
    rc = launch_fill_factor_uniform(Wc, KR, a->m, 11, 0, st);
    if (!rc) rc = launch_fill_factor_uniform(Hc, k, a->n, 12, 0, st);
    if (rc) return rc;
    return e.synced(time_launches(w, own, st, reps, [&]() -> int {
        return launch_conv_dense_step(which ? a->At : a->A, a->storage, which ? a->ldAt : a->ldA, a->m, a->n, which, Wc, Hc, k, T, b, 0.0, 0.0, 0, scratch,
                                      ctx().cus, st);
    }, ms));
}

int smk_conv_dense_last_profile(int* matrix_passes, int* divergence_passes)
{
    if (matrix_passes) *matrix_passes = g_cv_matrix_passes;
    if (divergence_passes) *divergence_passes = g_cv_divergence_passes;
    return SMK_OK;
}

}  // extern "C"
