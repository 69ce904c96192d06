// smallk_amd/csrc/cd.cpp -- regularised NMF by cyclic coordinate descent on a resident matrix (include/smallk_amd.h:
// smk_nmf_cd_device, smk_cd_sweep): scikit-learn's solver="cd" without the shuffle.  A driver by itself, beside the
// solver's schedules: every pass over A is the product svd.cpp runs (factor_product.h), the Gram matrices are launch_gram, the
// sweep is cd.hip.  The entries are synchronous; every workspace belongs to the smk::Entry (entry.h: synchronised before it
// releases them, on every path) or a Scratch local of the entry; no field of the matrix handle is written here.
#include "entry.h"
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
    FactorPair f;                                 // the factors: Wt KP x m and H KP x n, k, KP, the stream
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
    const int k = r.f.k, KP = r.f.KP;
    const size_t kk = (size_t)KP * KP;
    const i64 nmax = a->m > a->n ? a->m : a->n;
    int rc = own.dev(&r.Gw, kk);
    if (!rc) rc = own.dev(&r.Gh, kk);
    if (!rc) rc = own.dev(&r.gscratch, gram_scratch_elems(k, GRAM_BLOCKS));
    if (!rc && (a->sparse || !CD_READ_PARTIALS)) rc = own.dev(&r.R, (size_t)KP * nmax);
    if (!rc) rc = own.dev(&r.part, (size_t)cd_sweep_blocks(k, a->m) + cd_sweep_blocks(k, a->n));
    if (!rc) rc = own.dev(&r.vdev, 1);
    if (!rc) rc = own.pinned((void**)&r.vpin, sizeof(double));
    if (rc) { set_error("smk_nmf_cd_device: no memory for the factor workspace"); return SMK_DEVICE_ERROR; }
    return factor_product_alloc(r.fp, a, k, KP, r.f.st, own, "smk_nmf_cd_device");
}

// R = the product of A with the factor X, as the view the sweep reads
static int cd_product(CdRun& r, bool over_rows, const double* X, PartialView* pv)
{
    ++r.products;
    if (!r.a->sparse && CD_READ_PARTIALS) return factor_product_partials(r.fp, over_rows, X, pv);
    *pv = PartialView{r.R, 1, 0, r.f.KP, 1};
    return factor_product(r.fp, over_rows, X, r.R);
}

static int cd_sweep(CdRun& r, double* X, i64 N, PartialView R, const double* G, double l1, double l2, double* part)
{
    ++r.sweeps;
    return launch_cd_sweep(X, r.f.k, N, R, G, l1, l2, part, r.f.st);
}

// the sum of n partials -> the host, through the pinned slot (one synchronisation)
static int cd_violation(CdRun& r, int n, double* out)
{
    const int rc = launch_cd_violation(r.part, n, r.vdev, r.vpin, r.f.st);
    if (rc) return rc;
    SMK_HIP(hipStreamSynchronize(r.f.st));
    *out = *r.vpin;
    return 0;
}

static int cd_loop(CdRun& r, const smk_cd_options& o, smk_cd_stats* stats)
{
    const smk_matrix* a = r.a;
    const FactorPair& f = r.f;
    const Penalties p(a->m, a->n, o.alpha_w, o.alpha_h, o.l1_ratio);
    const int gh = cd_sweep_blocks(f.k, a->n), gw = cd_sweep_blocks(f.k, a->m);
    PartialView R1{}, R2{};
    int rc = 0;
    if (!o.update_w) {        // W'W and W'A once: the sweeps repeat on them
        rc = launch_gram(f.Wt, f.k, a->m, r.Gw, r.gscratch, GRAM_BLOCKS, f.st);
        if (!rc) rc = cd_product(r, true, f.Wt, &R1);
        if (rc) return rc;
    }
    stats->iterations = 0;
    stats->converged = 0;
    stats->violation_init = stats->violation = 0.0;
    for (int it = 1; it <= o.max_iter; ++it) {
        if (o.update_w) {
            rc = launch_gram(f.Wt, f.k, a->m, r.Gw, r.gscratch, GRAM_BLOCKS, f.st);
            if (!rc) rc = cd_product(r, true, f.Wt, &R1);
        }
        if (!rc) rc = cd_sweep(r, f.H, a->n, R1, r.Gw, p.l1h, p.l2h, r.part);
        if (!rc && o.update_w) {
            rc = launch_gram(f.H, f.k, a->n, r.Gh, r.gscratch, GRAM_BLOCKS, f.st);
            if (!rc) rc = cd_product(r, false, f.H, &R2);
            if (!rc) rc = cd_sweep(r, f.Wt, a->m, R2, r.Gh, p.l1w, p.l2w, r.part + gh);
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

}  // namespace smk

extern "C" {

int smk_nmf_cd_device(const smk_matrix* a, int k, const smk_cd_options* o, void* W, int dtW, int64_t rsW, int64_t csW, void* H, int dtH,
                      int64_t rsH, int64_t csH, void* stream, smk_cd_stats* stats)
{
    const std::string w("smk_nmf_cd_device");
    if (int rc = require_init()) return rc;
    if (!a || !o || !W || !H || !stats) { set_error(w + ": null argument"); return SMK_BAD_PARAM; }
    if (k < 1) { set_error(w + ": k < 1"); return SMK_BAD_PARAM; }
    if (k > a->m || k > a->n_global) { set_error(w + ": k exceeds min(m, n)"); return SMK_BAD_PARAM; }
    int rc = check_penalties(w, o->alpha_w, o->alpha_h, o->l1_ratio, o->tol, o->max_iter);
    if (!rc) rc = check_factor_dtypes(w, "W and H", dtW, dtH);
    if (rc) return rc;
    if (k > 128) { set_error(w + ": k > 128 is not supported yet"); return SMK_UNSUPPORTED; }
    if (a->n != a->n_global) { set_error(w + ": not available on a column shard"); return SMK_UNSUPPORTED; }
    if (!a->sparse && (a->single || !a->At)) {
        set_error(w + ": a single-copy dense matrix has no stored transpose, and the accurate-form product has no transposed-source kernel");
        return SMK_UNSUPPORTED;
    }
    CdRun r;
    r.a = a;
    r.f = FactorPair{a->m, a->n, k, kp_of(k), matrix_stream(a)};
    const DeviceView vW{W, dtW, rsW, csW}, vH{H, dtH, rsH, csH};
    rc = r.f.check(w, vW, vH, o->update_w != 0, true);
    if (rc) return rc;
    Entry e(r.f.st);
    rc = e.join(stream);
    if (!rc) rc = cd_alloc(r, e.own);
    if (!rc) rc = r.f.alloc_zeroed(e.own, w);
    if (rc) return rc;
    rc = r.f.load(vW, vH);
    smk_cd_stats st{};
    if (!rc) rc = cd_loop(r, *o, &st);
    g_cd_products = r.products;
    g_cd_sweeps = r.sweeps;
    if (!rc) rc = r.f.store(o->update_w ? &vW : nullptr, &vH);
    if (!rc) rc = e.sync();
    if (rc) return rc;
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
    if (int rc = require_init()) return rc;
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
    if (int rc = require_init()) return rc;
    if (which < 0 || which > 3 || k < 1 || k > 128 || ncols < 1 || slabs < 1 || slabs > 64 || reps < 1 || !ms) {
        set_error("smk_cd_sweep_time: bad argument");
        return SMK_BAD_PARAM;
    }
    const int KP = kp_of(k);
    Entry e(ctx().stream);
    Owned& own = e.own;
    const hipStream_t st = e.st;
    double *X = nullptr, *R = nullptr, *Rsum = nullptr, *G = nullptr, *gs = nullptr, *part = nullptr, *v = nullptr;
    const int nblk = cd_sweep_blocks(k, ncols);
    int rc = own.dev(&X, (size_t)KP * ncols);
    if (!rc) rc = own.dev(&R, (size_t)KP * ncols * slabs);
    if (!rc) rc = own.dev(&Rsum, (size_t)KP * ncols);
    if (!rc) rc = own.dev(&G, (size_t)KP * KP);
    if (!rc) rc = own.dev(&gs, gram_scratch_elems(k, GRAM_BLOCKS));
    if (!rc) rc = own.dev(&part, (size_t)nblk);
    if (!rc) rc = own.dev(&v, 1);
    if (rc) { set_error("smk_cd_sweep_time: no device memory"); return SMK_DEVICE_ERROR; }
    rc = launch_fill_factor_uniform(X, k, ncols, 11, 0, st);
    if (!rc) rc = launch_fill_factor_uniform(R, k, ncols * slabs, 12, 0, st);
    if (!rc) rc = launch_gram(X, k, ncols, G, gs, GRAM_BLOCKS, st);
    if (rc) return rc;
    const PartialView pv{R, slabs, (i64)ncols * KP, KP, 1};
    rc = time_launches("smk_cd_sweep_time", own, st, reps, [&]() -> int {
        switch (which) {
            case 0: return launch_cd_sweep(X, k, ncols, pv, G, 0.0, 0.0, part, st, 0);
            case 1: return launch_cd_sweep(X, k, ncols, pv, G, 0.0, 0.0, part, st, 1);
            case 2: return launch_hals_sweep(X, k, ncols, pv, G, st);
            default: return launch_reduce_partials(pv, k, 0, ncols, Rsum, 1, st);
        }
    }, ms);
    if (rc) return rc;
    double c = 0.0;
    if (which <= 1) {
        rc = launch_cd_violation(part, nblk, v, nullptr, st);
        if (rc) return rc;
        SMK_HIP(hipMemcpyAsync(&c, v, sizeof(double), hipMemcpyDeviceToHost, st));
        rc = e.sync();
        if (rc) return rc;
    }
    if (checksum) *checksum = c;
    return e.synced(SMK_OK);          // (which > 1: time_launches has waited for the last launch)
}

}  // extern "C"
