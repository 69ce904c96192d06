// smallk_amd/csrc/svd.cpp -- truncated SVD of a resident matrix and the NNDSVD start built from it (include/smallk_amd.h:
// smk_matrix_svd_device, smk_matrix_nndsvd_device, smk_solver_set_factors_nndsvd).  A randomised range finder with
// power iterations: every pass over A is the accurate-form streaming product (dense) or the fp64 gather product (sparse) the
// solver already has, every orthonormalisation is launch_gram + a host eigendecomposition of the l x l Gram matrix (svd_host.h)
// + the tall-skinny apply of svd.hip.  The entries are synchronous; every workspace belongs to the smk::Entry local of the entry
// (entry.h: synchronised before it releases them, on every path); no field of the matrix handle and no buffer of a solver is
// written here (the solver entry hands its finished start to smk_solver_set_factors_device).
#include "entry.h"
#include "factor_product.h"
#include "svd_host.h"

#include <cmath>
#include <string>
#include <vector>

namespace smk {

static const int SVD_MAX_L = 128;
static const bool SVD_FUSED_GRAM = true;      // orth's first apply also forms the Gram partials of its output (measured)

struct SvdRun {
    const smk_matrix* a = nullptr;
    int k = 0, l = 0, KP = 0, q = 0;
    hipStream_t st = nullptr;
    Owned* own = nullptr;
    double *Fm = nullptr, *Fn = nullptr;          // the two factors: KP x m and KP x n
    double *G = nullptr, *gscratch = nullptr, *Md = nullptr;
    double* Gp = nullptr;                         // Gram partials left by the fused apply (null: this padded rank has none)
    FactorProduct fp;                             // the passes over A (factor_product.h)
    std::vector<double> hG, lambda, E, M;
    int host_trips = 0;
    double host_us = 0.0;                         // the host's own work in those trips (eigendecomposition + M), without the copies
    FactorPair pair(bool v_rows) const { return {a->m, a->n, k, KP, st, Fm, Fn, v_rows}; }
};

// the last run of the calling thread, for tools/svd_rate.py (smk_svd_last_profile)
static thread_local int g_last_trips = 0;
static thread_local double g_last_host_us = 0.0;

static int svd_alloc(SvdRun& r)
{
    const smk_matrix* a = r.a;
    Owned& own = *r.own;
    const size_t kk = (size_t)r.KP * r.KP;
    int rc = own.dev(&r.Fm, (size_t)r.KP * a->m);
    if (!rc) rc = own.dev(&r.Fn, (size_t)r.KP * a->n);
    if (!rc) rc = own.dev(&r.G, kk);
    if (!rc) rc = own.dev(&r.Md, kk);
    if (!rc) rc = own.dev(&r.gscratch, gram_scratch_elems(r.l, GRAM_BLOCKS));
    const int fused = svd_apply_gram_blocks(r.KP, a->m > a->n ? a->m : a->n, ctx().cus);
    if (!rc && fused > 0) rc = own.dev(&r.Gp, (size_t)fused * kk);
    if (rc) { set_error("svd: no memory for the factor workspace"); return SMK_DEVICE_ERROR; }
    return factor_product_alloc(r.fp, a, r.l, r.KP, r.st, own, "svd");
}

// over_rows: out (KP x n) = (A' X')' for X = KP x m, the contraction over the rows of A; else out (KP x m) = (A X')' for X = KP x n
// (factor_product.h: the product cd.cpp runs too)
static int svd_product(SvdRun& r, bool over_rows, const double* X, double* out) { return factor_product(r.fp, over_rows, X, out); }

// the Gram matrix of F (KP x N) -> host -> eigendecomposition (r.lambda, r.E).  partials > 0: the fused apply has left that many
// partial sums of it in r.Gp, F is not read.
static int svd_gram_eig(SvdRun& r, const double* F, i64 N, int partials = 0)
{
    int rc = partials > 0 ? launch_gram_reduce(r.Gp, partials, r.l, r.G, r.st) : launch_gram(F, r.l, N, r.G, r.gscratch, GRAM_BLOCKS, r.st);
    if (rc) return rc;
    r.hG.resize((size_t)r.KP * r.KP);
    SMK_HIP(hipMemcpyAsync(r.hG.data(), r.G, r.hG.size() * sizeof(double), hipMemcpyDeviceToHost, r.st));
    SMK_HIP(hipStreamSynchronize(r.st));
    const double t0 = wall_us();
    svdh::jacobi_eigh(r.hG.data(), r.KP, r.l, r.lambda, r.E);
    r.host_us += wall_us() - t0;
    ++r.host_trips;
    g_last_trips = r.host_trips;
    g_last_host_us = r.host_us;
    return 0;
}

// F <- F M for a host M (l x lout, row-major with pitch l).  gram_partials (optional): take the fused kernel where there is one
// and report how many Gram partials of the new F it left in r.Gp (0: none, form the Gram matrix from F)
static int svd_apply_host(SvdRun& r, double* F, i64 N, const std::vector<double>& M, int lout, int* gram_partials = nullptr)
{
    SMK_HIP(hipMemcpyAsync(r.Md, M.data(), (size_t)r.l * r.l * sizeof(double), hipMemcpyHostToDevice, r.st));
    int rc = 1;
    if (gram_partials) {
        *gram_partials = 0;
        if (r.Gp) rc = launch_svd_apply_gram(F, F, r.KP, N, r.Md, r.l, r.l, lout, r.Gp, gram_partials, ctx().cus, r.st);
        if (rc < 0) return rc;
        if (rc == 1) *gram_partials = 0;
    }
    if (rc == 1) rc = launch_svd_apply(F, F, r.KP, N, r.Md, r.l, r.l, lout, ctx().cus, r.st);
    if (rc) return rc;
    SMK_HIP(hipStreamSynchronize(r.st));          // M is a host vector that is rewritten by the next step
    return 0;
}

// orth(F): two rounds of Gram + eigendecomposition + apply.  The first round leaves F'F = I to about 2^40 u, the second to l u.
static int svd_orth(SvdRun& r, double* F, i64 N)
{
    int partials = 0;                 // the first round's apply leaves the Gram partials of its output for the second round
    for (int round = 0; round < 2; ++round) {
        int rc = svd_gram_eig(r, F, N, partials);
        if (rc) return rc;
        svdh::orth_matrix(r.lambda, r.E, r.l, r.M);
        rc = svd_apply_host(r, F, N, r.M, r.l, (round == 0 && SVD_FUSED_GRAM) ? &partials : nullptr);
        if (rc) return rc;
    }
    return 0;
}

// what every entry checks first; fills k-independent parts of the run
static int svd_args(const char* who, const smk_matrix* a, const smk_svd_options* o, int k, SvdRun& r)
{
    const std::string w(who);
    if (int rc = require_init()) return rc;
    if (!a) { set_error(w + ": null matrix"); return SMK_BAD_PARAM; }
    if (k < 1) { set_error(w + ": k < 1"); return SMK_BAD_PARAM; }
    if (k > a->m || k > a->n_global) { set_error(w + ": k exceeds min(m, n)"); return SMK_BAD_PARAM; }
    const int p = (o && o->oversample >= 0) ? o->oversample : 8;
    const int q = (o && o->power_iters >= 0) ? o->power_iters : 2;
    if ((i64)k + p > SVD_MAX_L) { set_error(w + ": k + oversample > 128 is not supported yet"); return SMK_UNSUPPORTED; }
    if (a->n != a->n_global) { set_error(w + ": not available on a column shard"); return SMK_UNSUPPORTED; }
    if (!a->sparse && (a->single || !a->At)) {
        set_error(w + ": a single-copy dense matrix has no stored transpose, and the accurate-form product has no transposed-source kernel");
        return SMK_UNSUPPORTED;
    }
    if (o && o->omega && !is_factor_dtype(o->omega_dtype)) { set_error(w + ": omega is fp64 or fp32"); return SMK_BAD_PARAM; }
    r.a = a;
    r.k = k;
    i64 l = (i64)k + p;
    if (l > a->m) l = a->m;
    if (l > a->n) l = a->n;
    r.l = (int)l;
    r.KP = kp_of(r.l);
    r.q = q;
    if (o && o->omega) {
        const int rc = check_device_view(o->omega, o->omega_dtype, a->n, r.l, o->omega_rs, o->omega_cs, false, (w + "(omega)").c_str());
        if (rc) return rc;
    }
    return SMK_OK;
}

// The SVD proper.  On return r.Fm holds U' (rows < k of a KP x m factor) and r.Fn holds V' (KP x n), both complete, S the k
// singular values.  Synchronises r.st.
static int svd_core(SvdRun& r, const smk_svd_options* o, double* S)
{
    const smk_matrix* a = r.a;
    int rc = svd_alloc(r);
    if (rc) return rc;
    // 1. the test matrix, as the factor Omega' (KP x n), and Y = A Omega
    if (o && o->omega) {
        SMK_HIP(hipMemsetAsync(r.Fn, 0, (size_t)r.KP * a->n * sizeof(double), r.st));
        rc = convert_view(DeviceView::in(o->omega, o->omega_dtype, o->omega_rs, o->omega_cs), DeviceView::rows(r.Fn, r.KP), a->n, r.l, r.st);
    } else {
        rc = launch_svd_fill_centred(r.Fn, r.KP, r.l, a->n, o ? o->seed : 0, r.st);
    }
    if (!rc) rc = svd_product(r, false, r.Fn, r.Fm);
    if (!rc) rc = svd_orth(r, r.Fm, a->m);
    // 3. power iterations
    for (int it = 0; it < r.q && !rc; ++it) {
        rc = svd_product(r, true, r.Fm, r.Fn);
        if (!rc) rc = svd_orth(r, r.Fn, a->n);
        if (!rc) rc = svd_product(r, false, r.Fn, r.Fm);
        if (!rc) rc = svd_orth(r, r.Fm, a->m);
    }
    // 4. B' = A' Q, the eigendecomposition of B B', the k leading triplets
    if (!rc) rc = svd_product(r, true, r.Fm, r.Fn);
    if (!rc) rc = svd_gram_eig(r, r.Fn, a->n);
    if (rc) return rc;
    const double top = r.lambda[0];
    std::vector<double> Eu((size_t)r.l * r.l, 0.0), Ev((size_t)r.l * r.l, 0.0);
    for (int j = 0; j < r.k; ++j) {
        const double lam = r.lambda[(size_t)j];
        const bool live = lam > 0.0 && lam > svdh::RANK_TOL * top;
        S[j] = live ? std::sqrt(lam) : 0.0;
        if (!live) continue;
        for (int i = 0; i < r.l; ++i) {
            Eu[(size_t)i * r.l + j] = r.E[(size_t)i * r.l + j];
            Ev[(size_t)i * r.l + j] = r.E[(size_t)i * r.l + j] / S[j];
        }
    }
    rc = svd_apply_host(r, r.Fm, a->m, Eu, r.k);
    if (!rc) rc = svd_apply_host(r, r.Fn, a->n, Ev, r.k);
    // V = B' E / S keeps V'V = I only to u (sigma_1 / sigma_k)^2: one symmetric re-orthonormalisation V <- V (V'V)^(-1/2) brings it
    // to l u without turning the vectors among themselves (rows >= k of the factor are zero and stay zero)
    if (!rc) rc = svd_gram_eig(r, r.Fn, a->n);
    if (rc) return rc;
    svdh::polish_matrix(r.lambda, r.E, r.l, r.M);
    return svd_apply_host(r, r.Fn, a->n, r.M, r.k);
}

// U' / V' of a finished run -> the NNDSVD start, in place (r.Fm becomes W', r.Fn becomes H)
static int nndsvd_from_svd(SvdRun& r, const double* S, int variant)
{
    const smk_matrix* a = r.a;
    Owned& own = *r.own;
    const int KP = r.KP, k = r.k;
    double *stats = nullptr, *sscratch = nullptr, *prm = nullptr, *part = nullptr, *sum = nullptr;
    const i64 nmax = a->m > a->n ? a->m : a->n;
    int rc = own.dev(&stats, (size_t)8 * KP);
    if (!rc) rc = own.dev(&sscratch, nndsvd_stats_scratch_elems(KP, nmax));
    if (!rc) rc = own.dev(&prm, (size_t)6 * KP);
    if (!rc) rc = own.dev(&part, 2048);
    if (!rc) rc = own.dev(&sum, 1);
    if (rc) { set_error("nndsvd: no memory for the split"); return SMK_DEVICE_ERROR; }
    rc = launch_nndsvd_stats(r.Fm, KP, k, a->m, sscratch, stats, r.st);
    if (!rc) rc = launch_nndsvd_stats(r.Fn, KP, k, a->n, sscratch, stats + 4 * KP, r.st);
    double fill = 0.0;
    if (!rc && variant == SMK_NNDSVDA)
        rc = a->sparse ? launch_sum_entries_sparse(a->val, a->nnz, part, sum, r.st)
                       : launch_sum_entries_dense(a->A, a->storage, a->ldA, a->m, a->n, part, sum, r.st);
    if (rc) return rc;
    std::vector<double> hs((size_t)8 * KP), hp((size_t)6 * KP, 0.0);
    SMK_HIP(hipMemcpyAsync(hs.data(), stats, hs.size() * sizeof(double), hipMemcpyDeviceToHost, r.st));
    if (variant == SMK_NNDSVDA) SMK_HIP(hipMemcpyAsync(&fill, sum, sizeof(double), hipMemcpyDeviceToHost, r.st));
    SMK_HIP(hipStreamSynchronize(r.st));
    if (variant == SMK_NNDSVDA) fill /= (double)a->m * (double)a->n;
    const double* su = hs.data();
    const double* sv = hs.data() + 4 * KP;
    double *pu = hp.data(), *pv = hp.data() + 3 * KP;
    for (int j = 0; j < k; ++j) {
        if (!(S[j] > 0.0)) continue;                  // past the rank of A: the component stays zero (mode 0)
        const double up = su[j], un = su[KP + j], ump = su[2 * KP + j], umn = su[3 * KP + j];
        const double vp = sv[j], vn = sv[KP + j], vmp = sv[2 * KP + j], vmn = sv[3 * KP + j];
        if (j == 0) {
            pu[j] = pv[j] = 2.0;
            pu[KP + j] = pv[KP + j] = std::sqrt(S[0]);
            pu[2 * KP + j] = svdh::RANK_TOL * (ump > umn ? ump : umn);
            pv[2 * KP + j] = svdh::RANK_TOL * (vmp > vmn ? vmp : vmn);
            continue;
        }
        const double nup = std::sqrt(up), nun = std::sqrt(un), nvp = std::sqrt(vp), nvn = std::sqrt(vn);
        const double mpos = nup * nvp, mneg = nun * nvn;
        const bool pos = mpos >= mneg;                // an exact tie keeps the positive pair
        const double mm = pos ? mpos : mneg;
        if (!(mm > 0.0)) continue;
        const double f = std::sqrt(S[j] * mm);
        pu[j] = pv[j] = pos ? 1.0 : -1.0;
        pu[KP + j] = f / (pos ? nup : nun);
        pv[KP + j] = f / (pos ? nvp : nvn);
        pu[2 * KP + j] = svdh::RANK_TOL * (pos ? ump : umn);
        pv[2 * KP + j] = svdh::RANK_TOL * (pos ? vmp : vmn);
    }
    SMK_HIP(hipMemcpyAsync(prm, hp.data(), hp.size() * sizeof(double), hipMemcpyHostToDevice, r.st));
    rc = launch_nndsvd_write(r.Fm, KP, k, a->m, prm, fill, r.st);
    if (!rc) rc = launch_nndsvd_write(r.Fn, KP, k, a->n, prm + 3 * KP, fill, r.st);
    if (rc) return rc;
    SMK_HIP(hipStreamSynchronize(r.st));              // hp leaves scope
    return 0;
}

}  // namespace smk

extern "C" {

int smk_matrix_svd_device(const smk_matrix* a, const smk_svd_options* opts, void* U, int dtypeU, int64_t rsU, int64_t csU, double* S_host,
                          void* V, int dtypeV, int64_t rsV, int64_t csV, void* stream)
{
    const char* who = "smk_matrix_svd_device";
    SvdRun r;
    if (!opts) { set_error("smk_matrix_svd_device: null options"); return SMK_BAD_PARAM; }
    int rc = svd_args(who, a, opts, opts->k, r);
    if (rc) return rc;
    if (!S_host) { set_error("smk_matrix_svd_device: null output"); return SMK_BAD_PARAM; }
    const DeviceView vU{U, dtypeU, rsU, csU}, vV{V, dtypeV, rsV, csV};
    rc = check_factor_dtypes(who, "U and V", dtypeU, dtypeV);
    if (!rc) rc = r.pair(true).check(who, vU, vV, true, true, "U", "V");
    if (rc) return rc;
    Entry e(matrix_stream(a));
    r.own = &e.own;
    r.st = e.st;
    rc = e.join(stream);
    if (!rc) rc = svd_core(r, opts, S_host);
    if (!rc) rc = r.pair(true).store(&vU, &vV);
    return rc ? rc : e.sync();
}

int smk_matrix_nndsvd_device(const smk_matrix* a, const smk_svd_options* opts, int variant, void* W, int dtypeW, int64_t rsW, int64_t csW,
                             void* H, int dtypeH, int64_t rsH, int64_t csH, void* stream)
{
    const char* who = "smk_matrix_nndsvd_device";
    SvdRun r;
    if (!opts) { set_error("smk_matrix_nndsvd_device: null options"); return SMK_BAD_PARAM; }
    int rc = svd_args(who, a, opts, opts->k, r);
    if (rc) return rc;
    if (variant != SMK_NNDSVD && variant != SMK_NNDSVDA) { set_error("smk_matrix_nndsvd_device: unknown variant"); return SMK_BAD_PARAM; }
    const DeviceView vW{W, dtypeW, rsW, csW}, vH{H, dtypeH, rsH, csH};
    rc = check_factor_dtypes(who, "W and H", dtypeW, dtypeH);
    if (!rc) rc = r.pair(false).check(who, vW, vH, true, true);
    if (rc) return rc;
    Entry e(matrix_stream(a));
    r.own = &e.own;
    r.st = e.st;
    std::vector<double> S((size_t)r.k, 0.0);
    rc = e.join(stream);
    if (!rc) rc = svd_core(r, opts, S.data());
    if (!rc) rc = nndsvd_from_svd(r, S.data(), variant);
    if (!rc) rc = r.pair(false).store(&vW, &vH);
    return rc ? rc : e.sync();
}

int smk_svd_last_profile(int* host_trips, double* host_ms)
{
    if (host_trips) *host_trips = g_last_trips;
    if (host_ms) *host_ms = g_last_host_us * 1e-3;
    return SMK_OK;
}

int smk_solver_set_factors_nndsvd(smk_solver* s, const smk_svd_options* opts, int variant)
{
    if (!s) { set_error("smk_solver_set_factors_nndsvd: null solver"); return SMK_BAD_PARAM; }
    if (s->ex.ar || s->ex.comm || s->ex.world > 1) { set_error("smk_solver_set_factors_nndsvd: not available on a solver with a communicator"); return SMK_UNSUPPORTED; }
    if (variant != SMK_NNDSVD && variant != SMK_NNDSVDA) { set_error("smk_solver_set_factors_nndsvd: unknown variant"); return SMK_BAD_PARAM; }
    SvdRun r;
    int rc = svd_args("smk_solver_set_factors_nndsvd", s->a, opts, s->k, r);
    if (rc) return rc;
    Entry e(s->st);
    r.own = &e.own;
    r.st = e.st;
    std::vector<double> S((size_t)r.k, 0.0);
    rc = svd_core(r, opts, S.data());
    if (!rc) rc = nndsvd_from_svd(r, S.data(), variant);
    if (rc) return rc;
    // the finished start lies in this call's workspace as W' (KP x m) and H (KP x n): hand it over as any caller would
    const FactorPair f = r.pair(false);
    const DeviceView vW = f.first(), vH = f.second();
    return e.synced(smk_solver_set_factors_device(s, vW.p, vW.dtype, vW.rs, vW.cs, vH.p, vH.dtype, vH.rs, vH.cs, (void*)s->st));
}

}  // extern "C"
