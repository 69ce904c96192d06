// smallk_amd/csrc/guard.cpp -- the run-time guard of the product form: every SMK_GUARD_EVERY iterations of a BPP run the fast form's
// W'A is compared with the accurate form's on a column sample, and the run changes to the accurate form when the discrepancy
// times the condition of the Gram matrices passes SMK_GUARD_TAU.  Its state is the solver's ProductGuard (state.h); solver.cpp
// calls guard_step behind every iteration and lends it the planning functions and solver_init for the re-plan.
#include "solver_internal.h"

#include <algorithm>
#include <cmath>
#include <cstdio>
#include <vector>

namespace smk {

// ---- run-time guard of the product form ------------------------------------------------------------------------------
// Which product form a run takes is decided when the solver is created (rank, algorithm, the spread of the column scales:
// thresholds found by sweeps).  A matrix outside the swept families must not leave the 1e-4 bar silently, so the choice is
// can be re-examined while the run goes on (OPT-IN: SMK_GUARD_EVERY=16; default 0 = off, see the note at the end).  Every
// SMK_GUARD_EVERY iterations of a BPP run the solver forms W'A for a sample
// of 64 columns in the ACCURATE form (fp64 factor against the stored data, bigprod_f64_kernel) and compares it with what the
// fast form has just produced for the same columns: delta = ||P_fast - P_acc||_F / ||P_acc||_F, the product error ON THIS
// DATA (4e-8 for well-scaled data; much more when small entries sit next to large ones).  To first order an error delta in
// the right-hand sides moves the solution of the k x k normal equations by at most cond(G) delta, G = W'W or HH', and the
// condition numbers are cheap: both Gram matrices come back with the two sums (k <= 256: Cholesky + inverse on the host,
// 1-norm).  When max(cond) * delta exceeds SMK_GUARD_TAU (default 1e-4: ONE iteration could move the factors by the parity
// bar) the solver changes to the accurate form for the rest of the run: plans and buffers are rebuilt and solver.Init is
// repeated on the current factors, exactly what a fresh solver given them would do.  The check is asynchronous -- enqueued
// behind one iteration, read GUARD_EVERY iterations later -- so it never stalls the stream (C4: one 67 MB pass per 16
// iterations of 137 GB each; measured -1.1 % on C4, -8 % on the 0.09 ms iterations of C2 where the host runs at most 16
// iterations ahead).  Not for sharded runs (every rank would have to agree; their form is agreed once, at attach).
// WHY IT IS NOT ON BY DEFAULT (round 4, profiles/r04_guard_cases.txt): cond(G) delta is a worst-case bound, and the
// non-negativity constraints take the ill-conditioned directions out of the problems that are actually solved.  HALS on
// uniform noise at k = 8 shows cond(HH') = 2.3e4, delta = 1.2e-8, product 2.6e-4 > tau, while the run ends 1.7e-6 from the
// oracle after 40 iterations; with the guard on, C3 (HALS, k = 32) changes to the accurate form and runs at 253 instead of
// 1160 iterations/s.  For block pivoting -- where the bound describes the solves that are really done -- the cases measured
// separate cleanly (noise: 2e-6 .. 7e-6 over 40 iterations; a planted factor with nearly collinear columns: > 1e-2), so the
// guard is offered for BPP runs on data outside the swept families, and the static rules of smk_solver_create stay the default.
static bool guard_applies(const smk_solver* s)
{
    const int every = sw::guard_every();
    if (every <= 0 || s->guard.off || s->a->sparse || s->nsplit == NSPLIT_F64 || is_dist(s) || s->ex.comm) return false;
    if (s->o.algorithm != SMK_ALG_BPP) return false;
    return s->k <= 256 && s->n >= 64 && s->iter > 0 && s->iter % every == 0;
}

// 1-norm condition number of the live k x k block of a KP x KP symmetric matrix (inf when it is not positive definite)
static double cond1_spd(const double* G, int KP, int k)
{
    std::vector<double> L((size_t)k * k, 0.0), X((size_t)k * k, 0.0);
    double n1 = 0.0;
    for (int c = 0; c < k; ++c) { double sum = 0.0; for (int r = 0; r < k; ++r) sum += std::fabs(G[(size_t)c * KP + r]); n1 = std::max(n1, sum); }
    for (int j = 0; j < k; ++j) {                                  // G = L L'
        double d = G[(size_t)j * KP + j];
        for (int p = 0; p < j; ++p) d -= L[(size_t)j * k + p] * L[(size_t)j * k + p];
        if (!(d > 0.0)) return INFINITY;
        const double ljj = std::sqrt(d);
        L[(size_t)j * k + j] = ljj;
        for (int i = j + 1; i < k; ++i) {
            double v = G[(size_t)j * KP + i];
            for (int p = 0; p < j; ++p) v -= L[(size_t)i * k + p] * L[(size_t)j * k + p];
            L[(size_t)i * k + j] = v / ljj;
        }
    }
    double ninv = 0.0;
    std::vector<double> y((size_t)k);
    for (int c = 0; c < k; ++c) {                                  // column c of the inverse: L y = e_c, L' x = y
        for (int i = 0; i < k; ++i) {
            double v = i == c ? 1.0 : 0.0;
            for (int p = 0; p < i; ++p) v -= L[(size_t)i * k + p] * y[(size_t)p];
            y[(size_t)i] = v / L[(size_t)i * k + i];
        }
        double sum = 0.0;
        for (int i = k - 1; i >= 0; --i) {
            double v = y[(size_t)i];
            for (int p = i + 1; p < k; ++p) v -= L[(size_t)p * k + i] * X[(size_t)p];
            X[(size_t)i] = v / L[(size_t)i * k + i];
            sum += std::fabs(X[(size_t)i]);
        }
        ninv = std::max(ninv, sum);
    }
    return n1 * ninv;
}

static int guard_resolve(smk_solver* s)
{
    ProductGuard& g = s->guard;
    if (!g.pending) return 0;
    g.pending = false;
    SMK_HIP(hipEventSynchronize(g.ev));
    const double tau = sw::guard_tau();
    const double* p = g.pin;
    const double delta = p[1] > 0.0 ? std::sqrt(p[0] / p[1]) : 0.0;
    const size_t kk = (size_t)s->KP * s->KP;
    const double cond = std::max(cond1_spd(p + 2, s->KP, s->k), cond1_spd(p + 2 + kk, s->KP, s->k));
    g.checks += 1;
    g.last = cond * delta;
    if (sw::guard_verbose()) fprintf(stderr, "[smk guard] iteration %d: delta %.3e, cond %.3e, product %.3e (tau %.1e)\n", s->iter, delta, cond, cond * delta, tau);
    if (!(cond * delta > tau)) return 0;
    // change to the accurate form: new plans and buffers, then solver.Init on the current factors (it forgets every hand-off)
    g.fired += 1;
    s->nsplit = NSPLIT_F64;
    int rc = plan_products(s);
    if (!rc && alloc_product_buffers(s)) rc = SMK_DEVICE_ERROR;
    if (rc) return rc;
    const int iter_keep = s->iter;
    rc = solver_init(s);
    s->iter = iter_keep;
    return rc;
}

static int guard_enqueue(smk_solver* s)
{
    ProductGuard& g = s->guard;
    const size_t kk = (size_t)s->KP * s->KP;
    if (!g.As) {                    // first use: the sample (64 columns, evenly spaced), plans, buffers
        const int nc = 64;
        std::vector<unsigned> cols((size_t)nc);
        for (int i = 0; i < nc; ++i) cols[(size_t)i] = (unsigned)((i64)i * s->n / nc);
        const i64 es = elem_size(s->a->storage);
        int rc = s->own.dev(&g.cols, (size_t)nc);
        rc |= s->own.dev((unsigned char**)&g.As, (size_t)s->a->ldA * COL_PAD * es);
        rc |= s->own.dev(&g.dev, 2 + 2 * kk);
        if (rc) return SMK_DEVICE_ERROR;
        SMK_HIP(hipMemsetAsync(g.As, 0, (size_t)s->a->ldA * COL_PAD * es, s->st));
        SMK_HIP(hipMemcpyAsync(g.cols, cols.data(), (size_t)nc * sizeof(unsigned), hipMemcpyHostToDevice, s->st));
        rc = launch_gather_cols(s->a->A, s->a->ldA * es, g.cols, nc, g.As, s->a->ldA * es, s->a->ldA * es, s->st);
        if (rc) return rc;
        SMK_HIP(hipStreamSynchronize(s->st));              // `cols` leaves scope
        const int ng = plan_bigprod_groups(s->a->storage, s->k, s->m, nc, NSPLIT_F64, ctx().cus, g.pl);
        for (int i = 0; i < ng; ++i) g.pl[i].ldx = s->KP;
        if (s->own.dev(&g.P, g.pl[0].p_elems) || s->own.pinned((void**)&g.pin, (2 + 2 * kk) * sizeof(double)) ||
            s->own.event(&g.ev, hipEventDisableTiming))
            return SMK_DEVICE_ERROR;
        g.ncols = nc;
    }
    // the full fp64 W (s->Wt) against the sampled columns, one launch per group of 64 factor rows
    for (int i = 0; i < s->ng; ++i) {
        const int rc = launch_bigprod(g.pl[i], g.As, s->a->ldA, s->Wt + g.pl[i].k0, g.P + g.pl[i].k0, s->st);
        if (rc) return rc;
    }
    const BigProdPlan& gp = g.pl[0];
    int rc = launch_guard_compare(view1(s), g.cols, g.ncols, g.P, gp.S, (i64)gp.ncols_pad * gp.pstride, gp.pstride, s->k, g.dev, s->st);
    if (rc) return rc;
    SMK_HIP(hipMemcpyAsync(g.dev + 2, s->Gw, kk * sizeof(double), hipMemcpyDeviceToDevice, s->st));
    SMK_HIP(hipMemcpyAsync(g.dev + 2 + kk, s->Gh, kk * sizeof(double), hipMemcpyDeviceToDevice, s->st));
    SMK_HIP(hipMemcpyAsync(g.pin, g.dev, (2 + 2 * kk) * sizeof(double), hipMemcpyDeviceToHost, s->st));
    SMK_HIP(hipEventRecord(g.ev, s->st));
    g.pending = true;
    return 0;
}

// after every iteration: read the check enqueued GUARD_EVERY iterations ago, enqueue the next one
int guard_step(smk_solver* s)
{
    if (!guard_applies(s)) return 0;
    int rc = guard_resolve(s);
    if (rc || s->nsplit == NSPLIT_F64) return rc;
    rc = wait_r2(s);                      // HH' / the stored products are final
    if (rc) return rc;
    return guard_enqueue(s);
}

}  // namespace smk
