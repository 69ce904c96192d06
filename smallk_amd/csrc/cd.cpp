// smallk_amd/csrc/cd.cpp -- regularised NMF by cyclic coordinate descent on a resident matrix (include/smallk_amd.h:
// smk_nmf_cd_device, smk_cd_sweep): scikit-learn's solver="cd" without the shuffle.  A driver by itself, beside the
// solver's schedules: every pass over A is the product svd.cpp runs (factor_product.h), the Gram matrices are launch_gram, the
// sweep is cd.hip.  The entries are synchronous; every workspace belongs to an smk::Owned / Scratch local of the entry and is
// released on every path; no field of the matrix handle is written here.
#include "state.h"
#include "factor_product.h"

#include <cmath>
#include <string>
#include <vector>

namespace smk {

// dense A: the sweeps read the partial products of the streaming pass themselves (load_rhs4 adds the slabs), so that their
// reduction is not a launch and a round trip through memory of its own (measured)
static const bool CD_READ_PARTIALS = true;

struct CdRun {
    const smk_matrix* a = nullptr;
    int k = 0, KP = 0;
    hipStream_t st = nullptr;
    double *Wt = nullptr, *H = nullptr;           // the factors: KP x m and KP x n
    double *Gw = nullptr, *Gh = nullptr, *gscratch = nullptr, *R = nullptr, *part = nullptr, *vdev = nullptr;
    double* vpin = nullptr;                       // the pinned slot the host reads the violation from
    FactorProduct fp;
    int products = 0, sweeps = 0;
};

// the last run of the calling thread (smk_cd_last_profile)
static thread_local int g_cd_products = 0, g_cd_sweeps = 0;

static int cd_alloc(CdRun& r, Owned& own)
{
    const smk_matrix* a = r.a;
    const size_t kk = (size_t)r.KP * r.KP;
    const i64 nmax = a->m > a->n ? a->m : a->n;
    int rc = own.dev(&r.Wt, (size_t)r.KP * a->m);
    if (!rc) rc = own.dev(&r.H, (size_t)r.KP * a->n);
    if (!rc) rc = own.dev(&r.Gw, kk);
    if (!rc) rc = own.dev(&r.Gh, kk);
    if (!rc) rc = own.dev(&r.gscratch, gram_scratch_elems(r.k, GRAM_BLOCKS));
    if (!rc && (a->sparse || !CD_READ_PARTIALS)) rc = own.dev(&r.R, (size_t)r.KP * nmax);
    if (!rc) rc = own.dev(&r.part, (size_t)cd_sweep_blocks(r.k, a->m) + cd_sweep_blocks(r.k, a->n));
    if (!rc) rc = own.dev(&r.vdev, 1);
    if (!rc) rc = own.pinned((void**)&r.vpin, sizeof(double));
    if (rc) { set_error("smk_nmf_cd_device: no memory for the factor workspace"); return SMK_DEVICE_ERROR; }
    r.fp.a = a;
    r.fp.l = r.k;
    r.fp.KP = r.KP;
    r.fp.st = r.st;
    return factor_product_alloc(r.fp, own, "smk_nmf_cd_device");
}

// R = the product of A with the factor X, as the view the sweep reads
static int cd_product(CdRun& r, bool over_rows, const double* X, PartialView* pv)
{
    ++r.products;
    if (!r.a->sparse && CD_READ_PARTIALS) return factor_product_partials(r.fp, over_rows, X, pv);
    *pv = PartialView{r.R, 1, 0, r.KP, 1};
    return factor_product(r.fp, over_rows, X, r.R);
}

static int cd_sweep(CdRun& r, double* X, i64 N, PartialView R, const double* G, double l1, double l2, double* part)
{
    ++r.sweeps;
    return launch_cd_sweep(X, r.k, N, R, G, l1, l2, part, r.st);
}

// the sum of n partials -> the host, through the pinned slot (one synchronisation)
static int cd_violation(CdRun& r, int n, double* out)
{
    const int rc = launch_cd_violation(r.part, n, r.vdev, r.vpin, r.st);
    if (rc) return rc;
    SMK_HIP(hipStreamSynchronize(r.st));
    *out = *r.vpin;
    return 0;
}

static int cd_loop(CdRun& r, const smk_cd_options& o, smk_cd_stats* stats)
{
    const smk_matrix* a = r.a;
    const double m = (double)a->m, n = (double)a->n;
    const double l1h = m * o.alpha_h * o.l1_ratio, l2h = m * o.alpha_h * (1.0 - o.l1_ratio);
    const double l1w = n * o.alpha_w * o.l1_ratio, l2w = n * o.alpha_w * (1.0 - o.l1_ratio);
    const int gh = cd_sweep_blocks(r.k, a->n), gw = cd_sweep_blocks(r.k, a->m);
    PartialView R1{}, R2{};
    int rc = 0;
    if (!o.update_w) {        // W'W and W'A once: the sweeps repeat on them
        rc = launch_gram(r.Wt, r.k, a->m, r.Gw, r.gscratch, GRAM_BLOCKS, r.st);
        if (!rc) rc = cd_product(r, true, r.Wt, &R1);
        if (rc) return rc;
    }
    stats->iterations = 0;
    stats->converged = 0;
    stats->violation_init = stats->violation = 0.0;
    for (int it = 1; it <= o.max_iter; ++it) {
        if (o.update_w) {
            rc = launch_gram(r.Wt, r.k, a->m, r.Gw, r.gscratch, GRAM_BLOCKS, r.st);
            if (!rc) rc = cd_product(r, true, r.Wt, &R1);
        }
        if (!rc) rc = cd_sweep(r, r.H, a->n, R1, r.Gw, l1h, l2h, r.part);
        if (!rc && o.update_w) {
            rc = launch_gram(r.H, r.k, a->n, r.Gh, r.gscratch, GRAM_BLOCKS, r.st);
            if (!rc) rc = cd_product(r, false, r.H, &R2);
            if (!rc) rc = cd_sweep(r, r.Wt, a->m, R2, r.Gh, l1w, l2w, r.part + gh);
        }
        double v = 0.0;
        if (!rc) rc = cd_violation(r, o.update_w ? gh + gw : gh, &v);
        if (rc) return rc;
        stats->iterations = it;
        stats->violation = v;
        if (it == 1) stats->violation_init = v;
        if (stats->violation_init == 0.0 || v / stats->violation_init <= o.tol) { stats->converged = 1; break; }
    }
    return 0;
}

static bool cd_dtype(int dt) { return dt == SMK_DT_F64 || dt == SMK_DT_F32; }

}  // namespace smk

extern "C" {

int smk_nmf_cd_device(const smk_matrix* a, int k, const smk_cd_options* o, void* W, int dtW, int64_t rsW, int64_t csW, void* H, int dtH,
                      int64_t rsH, int64_t csH, void* stream, smk_cd_stats* stats)
{
    const std::string w("smk_nmf_cd_device");
    if (!ctx().init) { set_error("smk_initialize() has not been called"); return SMK_NOTINITIALIZED; }
    if (!a || !o || !W || !H || !stats) { set_error(w + ": null argument"); return SMK_BAD_PARAM; }
    if (k < 1) { set_error(w + ": k < 1"); return SMK_BAD_PARAM; }
    if (k > a->m || k > a->n_global) { set_error(w + ": k exceeds min(m, n)"); return SMK_BAD_PARAM; }
    if (!(o->alpha_w >= 0.0) || !(o->alpha_h >= 0.0)) { set_error(w + ": alpha_w and alpha_h must be >= 0"); return SMK_BAD_PARAM; }
    if (!(o->l1_ratio >= 0.0 && o->l1_ratio <= 1.0)) { set_error(w + ": l1_ratio must lie in [0, 1]"); return SMK_BAD_PARAM; }
    if (!(o->tol >= 0.0)) { set_error(w + ": tol must be >= 0"); return SMK_BAD_PARAM; }
    if (o->max_iter < 1) { set_error(w + ": max_iter < 1"); return SMK_BAD_PARAM; }
    if (!cd_dtype(dtW) || !cd_dtype(dtH)) { set_error(w + ": W and H are fp64 or fp32"); return SMK_BAD_PARAM; }
    if (k > 128) { set_error(w + ": k > 128 is not supported yet"); return SMK_UNSUPPORTED; }
    if (a->n != a->n_global) { set_error(w + ": not available on a column shard"); return SMK_UNSUPPORTED; }
    if (!a->sparse && (a->single || !a->At)) {
        set_error(w + ": a single-copy dense matrix has no stored transpose, and the accurate-form product has no transposed-source kernel");
        return SMK_UNSUPPORTED;
    }
    int rc = check_device_view(W, dtW, a->m, k, rsW, csW, o->update_w != 0, "smk_nmf_cd_device(W)");
    if (!rc) rc = check_device_view(H, dtH, k, a->n, rsH, csH, true, "smk_nmf_cd_device(H)");
    if (rc) return rc;
    Owned own;
    CdRun r;
    r.a = a;
    r.k = k;
    r.KP = kp_of(k);
    r.st = a->st ? a->st : ctx().stream;
    rc = join_caller_stream(own, r.st, stream);
    if (!rc) rc = cd_alloc(r, own);
    if (rc) return rc;
    // the views in: pad rows of the resident layout are zeros
    SMK_HIP(hipMemsetAsync(r.Wt, 0, (size_t)r.KP * a->m * sizeof(double), r.st));
    SMK_HIP(hipMemsetAsync(r.H, 0, (size_t)r.KP * a->n * sizeof(double), r.st));
    rc = launch_strided_convert(W, dtW, rsW, csW, r.Wt, DT_F64, r.KP, 1, a->m, k, r.st);
    if (!rc) rc = launch_strided_convert(H, dtH, rsH, csH, r.H, DT_F64, 1, r.KP, k, a->n, r.st);
    smk_cd_stats st{};
    if (!rc) rc = cd_loop(r, *o, &st);
    g_cd_products = r.products;
    g_cd_sweeps = r.sweeps;
    if (!rc && o->update_w) rc = launch_strided_convert(r.Wt, DT_F64, r.KP, 1, W, dtW, rsW, csW, a->m, k, r.st);
    if (!rc) rc = launch_strided_convert(r.H, DT_F64, 1, r.KP, H, dtH, rsH, csH, k, a->n, r.st);
    if (rc) return rc;
    SMK_HIP(hipStreamSynchronize(r.st));
    *stats = st;
    return SMK_OK;
}

int smk_cd_last_profile(int* products, int* sweeps)
{
    if (products) *products = g_cd_products;
    if (sweeps) *sweeps = g_cd_sweeps;
    return SMK_OK;
}

int smk_cd_sweep(int k, int64_t ncols, const double* G, int64_t ldG, const double* R, int64_t ldR, double* X, int64_t ldX, double l1,
                 double l2, double* violation)
{
    if (!ctx().init) { set_error("smk_initialize() has not been called"); return SMK_NOTINITIALIZED; }
    if (k < 1 || ncols < 1 || !G || !R || !X || !violation || ldG < k || ldR < k || ldX < k) { set_error("smk_cd_sweep: bad argument"); return SMK_BAD_PARAM; }
    if (k > 128) { set_error("smk_cd_sweep: k > 128 is not supported yet"); return SMK_UNSUPPORTED; }
    const int KP = kp_of(k);
    hipStream_t st = ctx().stream;
    std::vector<double> hg((size_t)KP * KP, 0.0), hr((size_t)KP * ncols, 0.0), hx((size_t)KP * ncols, 0.0);
    for (int t = 0; t < k; ++t)
        for (int c = 0; c < k; ++c) hg[(size_t)t * KP + c] = G[(size_t)c * ldG + t];       // row t of G contiguous
    for (int64_t c = 0; c < ncols; ++c)
        for (int t = 0; t < k; ++t) {
            hr[(size_t)c * KP + t] = R[(size_t)c * ldR + t];
            hx[(size_t)c * KP + t] = X[(size_t)c * ldX + t];
        }
    const int nblk = cd_sweep_blocks(k, ncols);
    Scratch<double> dg, dr, dx, dpart, dv;
    int rc = dg.alloc(hg.size());
    rc |= dr.alloc(hr.size());
    rc |= dx.alloc(hx.size());
    rc |= dpart.alloc((size_t)nblk);
    rc |= dv.alloc(1);
    if (rc) { set_error("smk_cd_sweep: no device memory"); return SMK_DEVICE_ERROR; }
    SMK_HIP(hipMemcpyAsync(dg, hg.data(), hg.size() * sizeof(double), hipMemcpyHostToDevice, st));
    SMK_HIP(hipMemcpyAsync(dr, hr.data(), hr.size() * sizeof(double), hipMemcpyHostToDevice, st));
    SMK_HIP(hipMemcpyAsync(dx, hx.data(), hx.size() * sizeof(double), hipMemcpyHostToDevice, st));
    const PartialView pv{dr, 1, 0, KP, 1};
    rc = launch_cd_sweep(dx, k, ncols, pv, dg, l1, l2, dpart, st);
    if (!rc) rc = launch_cd_violation(dpart, nblk, dv, nullptr, st);
    if (rc) return rc;
    double v = 0.0;
    SMK_HIP(hipMemcpyAsync(hx.data(), dx, hx.size() * sizeof(double), hipMemcpyDeviceToHost, st));
    SMK_HIP(hipMemcpyAsync(&v, dv, sizeof(double), hipMemcpyDeviceToHost, st));
    SMK_HIP(hipStreamSynchronize(st));
    for (int64_t c = 0; c < ncols; ++c)
        for (int t = 0; t < k; ++t) X[(size_t)c * ldX + t] = hx[(size_t)c * KP + t];
    *violation = v;
    return SMK_OK;
}

int smk_cd_sweep_time(int which, int k, int64_t ncols, int slabs, int reps, double* ms, double* checksum)
{
    if (!ctx().init) { set_error("smk_initialize() has not been called"); return SMK_NOTINITIALIZED; }
    if (which < 0 || which > 3 || k < 1 || k > 128 || ncols < 1 || slabs < 1 || slabs > 64 || reps < 1 || !ms) {
        set_error("smk_cd_sweep_time: bad argument");
        return SMK_BAD_PARAM;
    }
    const int KP = kp_of(k);
    hipStream_t st = ctx().stream;
    Owned own;
    double *X = nullptr, *R = nullptr, *Rsum = nullptr, *G = nullptr, *gs = nullptr, *part = nullptr, *v = nullptr;
    const int nblk = cd_sweep_blocks(k, ncols);
    int rc = own.dev(&X, (size_t)KP * ncols);
    if (!rc) rc = own.dev(&R, (size_t)KP * ncols * slabs);
    if (!rc) rc = own.dev(&Rsum, (size_t)KP * ncols);
    if (!rc) rc = own.dev(&G, (size_t)KP * KP);
    if (!rc) rc = own.dev(&gs, gram_scratch_elems(k, GRAM_BLOCKS));
    if (!rc) rc = own.dev(&part, (size_t)nblk);
    if (!rc) rc = own.dev(&v, 1);
    hipEvent_t e0 = nullptr, e1 = nullptr;
    if (!rc) rc = own.event(&e0, hipEventDefault);
    if (!rc) rc = own.event(&e1, hipEventDefault);
    if (rc) { set_error("smk_cd_sweep_time: no device memory"); return SMK_DEVICE_ERROR; }
    rc = launch_fill_factor_uniform(X, k, ncols, 11, 0, st);
    if (!rc) rc = launch_fill_factor_uniform(R, k, ncols * slabs, 12, 0, st);
    if (!rc) rc = launch_gram(X, k, ncols, G, gs, GRAM_BLOCKS, st);
    if (rc) return rc;
    const PartialView pv{R, slabs, (i64)ncols * KP, KP, 1};
    auto once = [&]() -> int {
        switch (which) {
            case 0: return launch_cd_sweep(X, k, ncols, pv, G, 0.0, 0.0, part, st, 0);
            case 1: return launch_cd_sweep(X, k, ncols, pv, G, 0.0, 0.0, part, st, 1);
            case 2: return launch_hals_sweep(X, k, ncols, pv, G, st);
            default: return launch_reduce_partials(pv, k, 0, ncols, Rsum, 1, st);
        }
    };
    for (int i = 0; i < 3 && !rc; ++i) rc = once();         // warm-up: the code object, the LDS opt-in
    if (rc) return rc;
    SMK_HIP(hipEventRecord(e0, st));
    for (int i = 0; i < reps && !rc; ++i) rc = once();
    if (rc) return rc;
    SMK_HIP(hipEventRecord(e1, st));
    SMK_HIP(hipEventSynchronize(e1));
    float t = 0.f;
    SMK_HIP(hipEventElapsedTime(&t, e0, e1));
    *ms = (double)t / reps;
    double c = 0.0;
    if (which <= 1) {
        rc = launch_cd_violation(part, nblk, v, nullptr, st);
        if (rc) return rc;
        SMK_HIP(hipMemcpyAsync(&c, v, sizeof(double), hipMemcpyDeviceToHost, st));
        SMK_HIP(hipStreamSynchronize(st));
    }
    if (checksum) *checksum = c;
    return SMK_OK;
}

}  // extern "C"
