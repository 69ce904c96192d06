// smallk_amd/csrc/solver.cpp -- the solver handle of the C ABI (include/smallk_amd.h): planning and
// allocation, the NmfSolve<> driver loop and the per-iteration schedules (MU / HALS / BPP / RANK2)
// expressed as launches of the kernels in kernels.hip, with everything an iteration calls -- the
// exchange with the other ranks included -- in this one translation unit.  Beside it: attach.cpp
// (giving the handle a communicator), factors.cpp (factors in and out), guard.cpp (the run-time guard
// of the product form), timing.cpp (what a caller reads about the passes), progress.cpp (the stopping
// rule's check), standalone.cpp (the entries without a handle).
//
// Device data layout (all in HBM, fp64 unless noted):
//   A   : m_pad x n_pad   bf16|f32, column-major, zero padded (rows to 128, cols to 128)
//   At  : n_pad x m_pad   same dtype: the explicit transpose (the reference's BPP keeps one
//         too, nmf_solver_bpp.hpp:319) so BOTH streaming products contract down the
//         contiguous dimension
//   H   : KP x n (ld KP)    Wt : KP x m (ld KP) -- W is kept transposed on the device; KP = k padded
//         to 8/16/32/64, pad rows are zero
//   Gw = W'W, Gh = HH' : KP x KP (KP = 8/16/32/64 padded)
//   P1 : S1 slabs of n_pad x kpp fp64 = W'A partials,   P2 : S2 slabs of m_pad x kpp = (AH')' partials
//   packW / packH : MFMA operand fragments of W' / H
#include "solver_internal.h"
#include "entry.h"
#include "check_ring.h"
#include "comm.h"
#include "switches.h"

#include <climits>
#include <cmath>
#include <cstdio>
#include <cstring>
#include <functional>
#include <algorithm>
#include <thread>

extern "C" {

// BPP with a native communicator: every rank solves only its own blocks of W, so it needs only those rows of the summed
// (AH')' -- a reduce-scatter instead of an all-reduce (half the bytes on the wire) -- and the other ranks receive the
// packed streaming operand of those rows (4 B per entry in the fp16 form) instead of the fp64 values
static inline bool w_rows_sharded(const smk_solver* s) { return s->ex.w_sharded; }

// rows [r0, r1) of chunk j (clipped to the padded row count of the H*At pass; this rank's block of it: own_block, solver_internal.h)
static inline void chunk_rows(const smk_solver* s, int j, i64* r0, i64* r1)
{
    *r0 = (i64)j * s->ex.world * s->ex.blk;
    *r1 = std::min<i64>(*r0 + (i64)s->ex.world * s->ex.blk, s->pl2.ncols_pad);
}

// What the transposed-source kernels cover: MU, HALS and BPP with the 16-bit product forms (the reference's BPP keeps a transpose
// itself, nmf_solver_bpp.hpp:319 -- its W-side right-hand side H A' is the same product as MU's and HALS's, so it does not have
// to; RANK2 and the accurate form contract down the contiguous direction of A' on the vector ALUs / fp64 matrix cores).
static bool single_copy_serves(const smk_solver* s)
{
    const int alg = s->o.algorithm;
    const bool ok_alg = alg == SMK_ALG_MU || alg == SMK_ALG_HALS || alg == SMK_ALG_BPP;
    const bool ok_form = s->a->storage == SMK_STORE_BF16 ? (s->nsplit >= 1 && s->nsplit <= 3) : (s->nsplit == 3 || s->nsplit == NSPLIT_F16X2);
    return ok_alg && ok_form;
}

// Everything that depends on the product form (s->nsplit): the launch plans of both passes and the fp16 row scales ...
// (extern "C++": attach.cpp and guard.cpp re-plan through these two, solver_internal.h)
extern "C++" int smk::plan_products(smk_solver* s)
{
    const smk_matrix* a = s->a;
    if (s->nsplit == NSPLIT_F16X2 && a->ascale == 0.f) {
        const int rc0 = matrix_measure_scale(a, s->st);
        if (rc0) return rc0;
    }
    if (a->single && !a->sparse && !single_copy_serves(s)) {
        // every (re-)plan passes here -- smk_solver_create, the form agreement of attach_comm, guard_resolve, smk_solver_nnls_hals:
        // a single-copy matrix whose run leaves what the transposed-source kernels cover gets its stored transpose NOW, once
        // (the matrix is an ordinary one afterwards; solvers already planned on the transposed source keep reading A)
        const int trc = matrix_materialize_transpose(a);
        if (trc) return trc;
    }
    s->ng = plan_bigprod_groups(a->storage, s->k, s->m, s->n, s->nsplit, ctx().cus, s->pg1);
    if (a->single) {                                                                                        // H*A' from A itself
        if (plan_bigprod_groups_tr(a->storage, s->k, s->n, s->m, s->nsplit, ctx().cus, s->pg2) < 0) {
            set_error("no transposed-source kernel for this product form");
            return SMK_UNSUPPORTED;
        }
    } else (void)plan_bigprod_groups(a->storage, s->k, s->n, s->m, s->nsplit, ctx().cus, s->pg2);
    if (s->nsplit == NSPLIT_F64)
        for (int g = 0; g < s->ng; ++g) { s->pg1[g].ldx = s->KP; s->pg2[g].ldx = s->KP; }
    {
        // Cache policy of the streamed loads (BigProdPlan::temporal): what one iteration streams -- A and, unless the matrix is a
        // single copy, A' -- either stays in the 256 MB Infinity Cache between the passes or it does not.  Measured crossover:
        // profiles/r05_cache_policy_ab.txt.  SMK_BP_TEMPORAL=0/1 forces a policy.
        const double streamed = (double)s->m * (double)s->n * elem_size(a->storage) * (a->single ? 1.0 : 2.0) * s->ng;
        const int forced = sw::bp_temporal();
        const int temporal = forced >= 0 ? (forced ? 1 : 0) : (streamed <= 300.0e6 ? 1 : 0);
        for (int g = 0; g < s->ng; ++g) { s->pg1[g].temporal = temporal; s->pg2[g].temporal = temporal; }
    }
    s->pl1 = s->pg1[0];
    s->pl2 = s->pg2[0];
    if (s->nsplit == NSPLIT_F16X2) {
        int rc = 0;
        for (int side = 0; side < 2 && !rc; ++side) {
            if (!s->xscale[side]) rc |= s->own.dev(&s->xscale[side], (size_t)MAX_K);
            if (!s->oscale[side]) rc |= s->own.dev(&s->oscale[side], (size_t)MAX_K);
        }
        if (rc) return SMK_DEVICE_ERROR;
        for (int g = 0; g < s->ng; ++g) {
            s->pg1[g].oscale = s->oscale[0] + s->pg1[g].k0;  s->pg1[g].ascale = a->ascale;
            s->pg2[g].oscale = s->oscale[1] + s->pg2[g].k0;  s->pg2[g].ascale = a->ascale;
        }
        s->pl1 = s->pg1[0];
        s->pl2 = s->pg2[0];
    }
    const bool pack_env = sw::nnls_pack();                          // read per plan, like SMK_NSPLIT (0 = the separate reduce-and-pack launch)
    s->pack_in_solve = pack_env && !s->pack_in_solve_off && s->o.algorithm == SMK_ALG_BPP && s->KP == 16 && s->nsplit == NSPLIT_F16X2 &&
                       !a->sparse && !a->single && s->ng == 1 && !is_dist(s) && !s->ex.comm && bigprod_supports_tail(s->pl1) && bigprod_supports_tail(s->pl2);
    if (s->pack_in_solve && (a->colnorm_max < 0.0 || a->rownorm_max < 0.0)) {
        const int rc0 = matrix_measure_norms(a, s->st);
        if (rc0) return rc0;
    }
    return 0;
}
// ... and the buffers sized by those plans: the packed operands and the partial products (dense A)
extern "C++" int smk::alloc_product_buffers(smk_solver* s)
{
    int rc = 0;
    s->own.drop(&s->packW); s->own.drop(&s->packH); s->own.drop(&s->P1); s->own.drop(&s->P2);      // a re-plan sizes them anew
    if (!s->a->sparse) {
        rc |= s->own.dev((unsigned char**)&s->packW, packed_bytes(s->a->storage, s->k, s->m, s->nsplit));
        rc |= s->own.dev((unsigned char**)&s->packH, packed_bytes(s->a->storage, s->k, s->n, s->nsplit));
    }
    rc |= s->own.dev(&s->P1, s->pl1.p_elems);
    rc |= s->own.dev(&s->P2, s->pl2.p_elems);
    return rc;
}

int smk_solver_create(smk_solver** out, const smk_options* opts, const smk_matrix* a)
{
    if (!out) return SMK_BAD_PARAM;
    *out = nullptr;
    if (int rc = require_init()) return rc;
    if (!opts || !a) return SMK_BAD_PARAM;
    if (!smk_is_valid(opts, 1)) return SMK_BAD_PARAM;
    if (opts->height != a->m || opts->width != a->n_global) { set_error("options/matrix dimension mismatch"); return SMK_BAD_PARAM; }
    if (opts->k > MAX_K || (opts->algorithm == SMK_ALG_BPP && opts->k > MAX_K_BPP)) { set_error("device path supports k <= 2048"); return SMK_UNSUPPORTED; }
    // W and H element counts must fit the reference's 32-bit index (nmf.cpp:194-210)
    if ((uint64_t)a->m * (uint64_t)opts->k > 0x7FFFFFFFull) { fprintf(stderr, "W matrix size too large\n"); return SMK_SIZE_TOO_LARGE; }
    if ((uint64_t)a->n_global * (uint64_t)opts->k > 0x7FFFFFFFull) { fprintf(stderr, "H matrix size too large\n"); return SMK_SIZE_TOO_LARGE; }

    smk_solver* s = new smk_solver;
    ++ctx().live_solvers;
    s->o = *opts;
    s->a = a;
    s->k = opts->k;
    s->KP = kp_of(s->k);
    s->kpp = kpp_of(s->k);
    s->m = a->m;
    s->n = a->n;
    s->st = matrix_stream(a);
    const sw::Maybe<int> env = sw::nsplit();
    static_assert(ALG_MU == SMK_ALG_MU && ALG_HALS == SMK_ALG_HALS && ALG_RANK2 == SMK_ALG_RANK2 && ALG_BPP == SMK_ALG_BPP, "bigprod_plan.h");
    // the product form (bigprod_plan.h: default_product_form).  Its last rule needs the spread of A's column scales, measured once
    // per matrix where the rule can apply
    if (!env.set && !a->sparse && opts->algorithm != SMK_ALG_RANK2 && a->col_spread_log2 < 0) {
        const int rc0 = matrix_measure_scale(a, matrix_stream(a));
        if (rc0) { --ctx().live_solvers; delete s; return rc0; }
    }
    s->nsplit = resolve_product_form(opts->algorithm, opts->k, a->storage, a->sparse, a->m * a->n_global, a->col_spread_log2,
                                     sw::bpp_small_accurate() /* read per solver, like SMK_NSPLIT */, {env.set, env.v});
    // (a single-copy matrix outside what the transposed-source kernels cover gets its stored transpose inside plan_products)
    int rc = plan_products(s);
    if (rc) { smk_solver_destroy(s); return rc; }
    if (a->sparse) {   // gather products write one slab, as dense as the factor layout (KP values per column; RANK2: the 2 live ones)
        s->kpp = (opts->algorithm == SMK_ALG_RANK2) ? 2 : s->KP;
        int nb1 = 1, nb2 = 1;
        if (opts->algorithm == SMK_ALG_RANK2) {
            // a factor that does not fit an XCD's L2 is gathered block by block (one partial slab per row block)
            if (!a->blocked_tried) {
                a->blocked_tried = true;
                const int b1 = blocked_csc_blocks(a->m), b2 = blocked_csc_blocks(a->n);
                hipStream_t bst = matrix_stream(a);
                if (b1 > 1) (void)build_blocked_csc(a->m, a->n, a->nnz, a->colptr, a->rowidx, a->val, b1, &a->bA, bst);
                if (b2 > 1) (void)build_blocked_csc(a->n, a->m, a->nnz, a->colptr_t, a->rowidx_t, a->val_t, b2, &a->bAt, bst);
            }
            nb1 = a->bA.nb > 1 ? a->bA.nb : 1;
            nb2 = a->bAt.nb > 1 ? a->bAt.nb : 1;
        } else if (!is_wide(opts->k)) {
            // MU / HALS / BPP at ranks up to 128: the gather products work on entry-balanced segments (spmm_seg.hip);
            // SMK_SPMM_SEG=0 keeps the column-per-lane-group kernel of round 4
            ensure_seg_plans(a);
        }
        s->pl1.S = nb1; s->pl1.p_elems = (size_t)nb1 * s->pl1.ncols_pad * s->kpp;
        s->pl2.S = nb2; s->pl2.p_elems = (size_t)nb2 * s->pl2.ncols_pad * s->kpp;
    }

    const size_t kk = (size_t)s->KP * s->KP;
    rc |= s->own.dev(&s->H, (size_t)s->KP * s->n);
    rc |= s->own.dev(&s->Wt, (size_t)s->KP * s->m);
    rc |= s->own.dev(&s->Gw, kk);
    rc |= s->own.dev(&s->Gh, kk);
    {
        size_t gs = gram_scratch_elems(s->k, GRAM_BLOCKS);
        if (opts->algorithm == SMK_ALG_HALS && !a->sparse && (s->KP == 16 || s->KP == 32)) {
            // the sweeps' own Gram partials (HalsEpilogue): one per workgroup -- 1024 / KP columns of H, 256 rows of W
            const i64 need = std::max<i64>((s->n * s->KP + 1023) / 1024, (s->m + 255) / 256);
            if (need <= 4096) { s->hals_ep_blocks = (int)std::max<i64>(need, 1); gs = std::max(gs, gram_scratch_elems(s->k, s->hals_ep_blocks)); }
        }
        if (s->KP == 16 && opts->algorithm == SMK_ALG_BPP) gs = std::max(gs, (size_t)NNLS_GRAM_MAX * (256 + 16) + 8);   // partials from the NNLS launch
        rc |= s->own.dev(&s->gram_scratch, gs);
        if (s->o.algorithm == SMK_ALG_RANK2) {
            const size_t e1 = rank2_gram_scratch_elems(std::max(s->m, s->n)), e2 = rank2_progress_scratch_elems(s->m, s->n);
            rc |= s->own.dev(&s->r2_scratch, e1);
            rc |= s->own.dev(&s->r2_prog, e2);
            rc |= s->own.dev(&s->Graw, (size_t)s->KP * s->KP);
            if (a->sparse) { rc |= s->own.dev(&s->Hc, (size_t)2 * s->n); rc |= s->own.dev(&s->Wc, (size_t)2 * s->m); }

        }
        if (!rc && hipMemsetAsync(s->gram_scratch, 0, gs * sizeof(double), s->st) != hipSuccess) rc |= 1;   // incl. the ticket word
    }
    rc |= s->own.dev(&s->tmpW, (size_t)s->KP * s->m);
    if (is_wide(s->k)) rc |= s->own.dev(&s->wide_tmp, (size_t)s->KP * std::max(s->m, s->n));
    // one partial per workgroup of the column-tile kernels (grid = N*(KP/4)/256 blocks) and at most
    // 2 x 512 for delta_fnorm
    s->pg_half = (size_t)((std::max(s->m, s->n) * (s->KP / 4) + 255) / 256) + 1024;
    if (is_wide(s->k)) s->pg_half = std::max(s->pg_half, (size_t)((std::max(s->m, s->n) + 3) / 4) + 1024);   // one partial per 4 columns
    rc |= s->own.dev(&s->pg_partials, 2 * s->pg_half);
    rc |= s->own.dev(&s->scal, (size_t)8);
    rc |= s->own.dev(&s->fail_flag, (size_t)1);
    rc |= alloc_product_buffers(s);
    if (opts->algorithm == SMK_ALG_HALS) {
        rc |= s->own.dev(&s->hals_scratch, hals_w_scratch_elems(s->k, s->m));
        rc |= s->own.dev(&s->W0c, (size_t)s->KP * s->m);
        rc |= s->own.dev(&s->H0c, (size_t)s->KP * s->n);
        if (!rc) rc = hals_w_scratch_init(s->hals_scratch, s->k, s->m, s->st);
    }
    if (s->pack_in_solve && !s->W0c) {      // pack_fail_soft goes back to the initial factors
        rc |= s->own.dev(&s->W0c, (size_t)s->KP * s->m);
        rc |= s->own.dev(&s->H0c, (size_t)s->KP * s->n);
    }
    if (opts->algorithm == SMK_ALG_BPP) {
        // k <= 64: two (inverse + selector) halves; above: one Cholesky panel per resident workgroup (wide.hip)
        rc |= s->own.dev(&s->nnls_scratch, nnls_uses_tiles(s->k) ? nnls_wide_scratch_elems(s->k, ctx().cus, std::max(s->m, s->n)) : 2 * nnls_scratch_elems(s->k));
        // (above k = 64 the inverse stays in stream order: beside the product it gained 1-2 % -- measured -- and the two sides
        // share one scratch there)
        // The second stream pays two event hops per solve (~8 us each way on the main stream): worth it where it hides the 47 us
        // inversion of k in (32, 64] behind a dense pass; at k in (16, 32] (13 us) stream order is as fast or faster (4096 x 2048,
        // k = 32: 115 -> 92 us per iteration; 8192 x 4096: 131 -> 125; 32768 x 8192: equal), and with a sparse matrix the inverse
        // rides in the gather product's launch (start_inverse).  SMK_INV_STREAM=1: the second stream everywhere, =0: nowhere.
        const int inv_env = sw::inv_stream();
        const bool inv_beside = inv_env >= 0 ? inv_env != 0 : (!a->sparse && s->KP >= 64);
        if (inv_beside && (s->KP == 64 || (s->KP == 32 && nnls_inverse_at_32()))) {
            rc |= s->own.stream(&s->st_inv, hipStreamNonBlocking);
            for (int i = 0; i < 2 && !rc; ++i) {
                rc |= s->own.event(&s->ev_g[i], hipEventDisableTiming);
                rc |= s->own.event(&s->ev_inv[i], hipEventDisableTiming);
            }
        }
    }
    if (opts->prog_est_algorithm == SMK_PROG_DELTA_FNORM) rc |= s->own.dev(&s->Wprev, (size_t)s->KP * s->m);
    if (rc) { smk_solver_destroy(s); return SMK_DEVICE_ERROR; }
    *out = s;
    return SMK_OK;
}

void smk_solver_destroy(smk_solver* s)
{
    if (!s) return;
    s->own.release();
    --ctx().live_solvers;
    delete s;
}

// ---- collectives -------------------------------------------------------------------------------
// callback hook: one host call per buffer, in stream order on the main stream
static int dist_allreduce_cb(smk_solver* s, void* ptr, i64 count, int f64)
{
    if (s->ex.ar && s->ex.ar(s->ex.ar_user, ptr, (int64_t)count, f64)) { set_error("all-reduce callback failed"); return SMK_DEVICE_ERROR; }
    return 0;
}

// A pair of timing events for one span of smk_solver_kernel_time: a pair whose times resolve_events has read, else a new one
// from the owner.  The caller records both and pushes the span onto s->timing.ev[slot], or hands it back to s->timing.span_pool.
static int span_open(smk_solver* s, Timing::TimedSpan* sp, int counts = 1)
{
    if (!s->timing.span_pool.empty()) { *sp = s->timing.span_pool.back(); s->timing.span_pool.pop_back(); }
    else if (s->own.event(&sp->e0, hipEventDefault) || s->own.event(&sp->e1, hipEventDefault)) return SMK_DEVICE_ERROR;
    sp->counts = counts;
    return 0;
}

// native communicator: st2 picks up after everything enqueued on the main stream so far
static int comm_fork(smk_solver* s, hipEvent_t ev)
{
    SMK_HIP(hipEventRecord(ev, s->st));
    SMK_HIP(hipStreamWaitEvent(s->ex.st2, ev, 0));
    return 0;
}
// The main stream waits for `n` events of the collective stream.  On a timed pass the wait is bracketed by two events on the
// main stream: their distance is the time the main stream stood still for the exchange -- measured exposure instead of the
// "step time minus products" subtraction (slot 3 of smk_solver_kernel_time; the two records themselves cost a few us of idle
// time, so an exchange that is hidden completely still reads ~5 us per wait).
static int main_waits_for_comm(smk_solver* s, const hipEvent_t* evs, int n)
{
    const bool timed = s->timing.on && (s->timing.pass_timed[0] || s->timing.pass_timed[1]);
    Timing::TimedSpan sp{};
    if (timed && (s->timing.cal_counter++ & 3u) == 0 && s->ex.st2) {        // every fourth bracket is preceded by a calibration bracket
        if (!s->timing.ev_cal) {
            if (s->own.event(&s->timing.ev_cal, hipEventDisableTiming)) return SMK_DEVICE_ERROR;
            SMK_HIP(hipEventRecord(s->timing.ev_cal, s->ex.st2));
        } else {
            Timing::TimedSpan cal{};
            if (span_open(s, &cal)) return SMK_DEVICE_ERROR;
            (void)hipEventRecord(cal.e0, s->st);
            (void)hipStreamWaitEvent(s->st, s->timing.ev_cal, 0);
            (void)hipEventRecord(cal.e1, s->st);
            s->timing.ev[4].push_back(cal);
        }
    }
    if (timed) {
        if (span_open(s, &sp)) return SMK_DEVICE_ERROR;
        (void)hipEventRecord(sp.e0, s->st);
    }
    for (int i = 0; i < n; ++i)
        if (hipStreamWaitEvent(s->st, evs[i], 0) != hipSuccess) {
            if (timed) s->timing.span_pool.push_back(sp);
            set_error("hipStreamWaitEvent failed");
            return SMK_DEVICE_ERROR;
        }
    if (timed) {
        (void)hipEventRecord(sp.e1, s->st);
        s->timing.ev[3].push_back(sp);
    }
    return 0;
}
// ... and the main stream waits for what st2 has been given so far
static int comm_join(smk_solver* s, hipEvent_t ev)
{
    SMK_HIP(hipEventRecord(ev, s->ex.st2));
    return main_waits_for_comm(s, &ev, 1);
}

// a collective on st2 bracketed by events when timing is on (slot 2 of smk_solver_kernel_time)
static int timed_collective(smk_solver* s, int pass, const std::function<int()>& issue)
{
    if (!s->timing.on || !s->timing.pass_timed[pass]) return issue();
    Timing::TimedSpan sp{};
    if (span_open(s, &sp)) return SMK_DEVICE_ERROR;
    (void)hipEventRecord(sp.e0, s->ex.st2);
    const int rc = issue();
    if (rc) { s->timing.span_pool.push_back(sp); return rc; }
    (void)hipEventRecord(sp.e1, s->ex.st2);
    s->timing.ev[2].push_back(sp);
    return 0;
}

// a small in-place sum that the main stream needs right away (scalars of the stopping rule, W'W of a row-sharded W)
static int dist_allreduce_now(smk_solver* s, void* ptr, i64 count, int f64)
{
    if (!s->ex.comm) return dist_allreduce_cb(s, ptr, count, f64);
    int rc = comm_fork(s, s->ex.ev_x);
    if (rc) return rc;
    rc = comm_allreduce(s->ex.comm, ptr, count, f64, s->ex.st2);
    if (rc) return rc;
    return comm_join(s, s->ex.ev_y);
}

// HH' is needed only after the H*At pass: with a native communicator its all-reduce runs on the second stream
// beside that pass; wait_gh() joins it back.
static int allreduce_gh(smk_solver* s)
{
    if (!is_dist(s)) return 0;
    if (!s->ex.comm) return dist_allreduce_cb(s, s->Gh, (i64)s->KP * s->KP, 1);
    int rc = comm_fork(s, s->ex.ev_gram);
    if (rc) return rc;
    rc = comm_allreduce(s->ex.comm, s->Gh, (i64)s->KP * s->KP, 1, s->ex.st2);
    if (rc) return rc;
    SMK_HIP(hipEventRecord(s->ex.ev_gh, s->ex.st2));
    s->ex.gh_pending = true;
    return 0;
}
static int wait_gh(smk_solver* s)
{
    if (!s->ex.gh_pending) return 0;
    const int rc = main_waits_for_comm(s, &s->ex.ev_gh, 1);
    if (rc) return rc;
    s->ex.gh_pending = false;
    return 0;
}
// the main stream joins the chunk exchanges of the last H*At pass (every consumer of the summed (AH')' calls this)
// (extern "C++": progress.cpp calls it too, solver_internal.h -- as gather_w, sync_and_check and dist_agree below)
extern "C++" int smk::wait_r2(smk_solver* s)
{
    if (!s->ex.r2_pending) return 0;
    // (the chunk exchanges were recorded on ONE in-order stream: the last event covers the others -- one barrier packet on the
    // main stream instead of nchunk; tools/mb/mb_event_hop.hip prices them)
    const int rc = main_waits_for_comm(s, &s->ex.ev_r[s->ex.nchunk - 1], 1);
    if (rc) return rc;
    s->ex.r2_pending = false;
    return 0;
}

// BPP, k > 32: the inverse of a Gram matrix (side 0: W'W for the H solve, side 1: HH' for the W solve) is taken on a
// side stream as soon as the matrix exists; the streaming product that follows on the main stream hides it.
static inline double* inv_scratch(smk_solver* s, int side)
{
    return nnls_uses_tiles(s->k) ? s->nnls_scratch : s->nnls_scratch + (size_t)side * nnls_scratch_elems(s->k);
}
// `after`: the event that makes G final when that is not the main stream's current position (the HH' all-reduce of a
// sharded run finishes on the second stream)
static int start_inverse(smk_solver* s, int side, const double* G, hipEvent_t after = nullptr)
{
    Handoff& h = s->hand[side];
    h.forget_inverse();                 // G is new: whatever rode, ran beside or was done belonged to the matrix before it
    if (s->o.algorithm != SMK_ALG_BPP) return 0;
    {
        // The inverse is formed by one more workgroup of the product launch that follows this Gram matrix in every BPP schedule
        // (spmm_seg.hip / kernels.hip / bigprod.hip: InvRide) where that launch can carry it: a second stream pays two event hops
        // per solve, ~8 us each way on the main stream -- more than the 13 us inversion of k <= 32 they hide (the Reuters shape: 125
        // us per iteration beside the product, 118 in stream order, 91 riding; dense 4096 x 2048, k = 32: 115 / 92 / 70).  A launch
        // that cannot carry it leaves it to launch_nnls_bpp, in stream order, or to the second stream.  SMK_INV_RIDE=0: never rides.
        const bool ride = sw::inv_ride();
        const bool route = s->KP == 64 || (s->KP == 32 && nnls_inverse_at_32());
        const bool carrier = s->a->sparse ? true : (s->ng == 1 && bigprod_supports_ride(side == 0 ? s->pg1[0] : s->pg2[0]));
        if (ride && route && carrier && !after && !is_dist(s) && !s->ex.comm && !s->ex.w_sharded) { h.inverse_will_ride(); return 0; }
    }
    if (!s->st_inv) return 0;
    if (after) {
        SMK_HIP(hipStreamWaitEvent(s->st_inv, after, 0));
    } else {
        SMK_HIP(hipEventRecord(s->ev_g[side], s->st));
        SMK_HIP(hipStreamWaitEvent(s->st_inv, s->ev_g[side], 0));
    }
    int rc = launch_gram_inverse(G, s->k, inv_scratch(s, side), s->st_inv);
    if (rc) return rc;
    SMK_HIP(hipEventRecord(s->ev_inv[side], s->st_inv));
    h.inverse_sent_to_side_stream();
    return 0;
}
// `side` names the factor whose Gram matrix G is (0: W'W, the solve writes H; 1: HH', the solve writes W): hs is the hand-off
// record of that factor, hx the one of the factor being solved
static int nnls_side(smk_solver* s, int side, double* X, i64 c0, i64 c1, PartialView R, const double* G)
{
    const int fx = side == 0 ? 1 : 0;                // the factor being solved (0 = W, 1 = H); the other one is `side`
    Handoff &hs = s->hand[side], &hx = s->hand[fx];
    if (hs.inverse_on_side_stream()) {
        SMK_HIP(hipStreamWaitEvent(s->st, s->ev_inv[side], 0));
        hs.inverse_joined();
    }
    // k in (8, 16], fp16 form, one GPU: the launch that solves ALL columns of a factor also leaves its Gram partials (the
    // gram_x that follows in every BPP schedule then only reduces them)
    const bool fuse = sw::nnls_gram();
    const i64 N = side == 0 ? s->n : s->m;
    const bool want = fuse && s->KP == 16 && s->nsplit == NSPLIT_F16X2 && !is_dist(s) && c0 == 0 && c1 == N && (X == s->H || X == s->Wt);
    hx.gram_partials = 0;
    // ... and packs it, when the system matrix is the Gram matrix of a factor that an NNLS launch of this run produced (>= 0:
    // the bound behind the row scales needs that; the first solve of a run works from the caller's factor and packs the old way)
    NnlsPack pk;
    const bool pack = want && s->pack_in_solve && !s->pack_in_solve_off && !s->ex.comm && hs.from_nnls && s->a->colnorm_max >= 0.0 && s->a->rownorm_max >= 0.0;
    if (pack) {
        pk.out = (unsigned char*)(fx == 0 ? s->packW : s->packH);
        pk.xscale = s->xscale[fx];
        pk.oscale = s->oscale[fx];
        pk.anorm = side == 0 ? s->a->colnorm_max : s->a->rownorm_max;     // H's columns solve for columns of A, W's rows for rows
        pk.ascale = (double)s->a->ascale;
        pk.nq = packed_chunk_pairs_f16x2(s->a->storage, N);
        // TEST HOOK: shrink the bound so that the scaled entries leave fp16's range (the launch must flag it, the run must be
        // repeated without the packing: pack_fail_soft)
        pk.anorm *= sw::nnls_pack_test_anorm();
    }
    hx.packed_by_solve = false;
    // slot 5 of smk_solver_kernel_time: the block-pivoting launches (both kernels of a k > 16 solve), sampled with the pass that fed them
    Timing::TimedSpan tsp{};
    if (s->timing.on && s->timing.pass_timed[side] && c1 > c0 && span_open(s, &tsp) == 0) (void)hipEventRecord(tsp.e0, s->st);
    else tsp.e1 = nullptr;                      // (a launch that cannot be timed still runs)
    struct Stamp { smk_solver* s; Timing::TimedSpan sp; ~Stamp() { if (sp.e1) { (void)hipEventRecord(sp.e1, s->st); s->timing.ev[5].push_back(sp); } } } stamp{s, tsp};
    // riders of the checked loop (check_rides_in_nnls): the previous iteration's projected-gradient sum, this iteration's snapshot
    NnlsRiders rd;
    bool riders = false;
    const int k2 = (s->k + 1) / 2 * 2;
    ProgressCheck& pc = s->pc;
    if (c0 == 0 && c1 == N && (X == s->H || X == s->Wt) && (pc.pg_defer_slot >= 0 || pc.iter_snap_slot >= 0) && check_rides_in_nnls(s)) {
        if (side == 0 && pc.pg_defer_slot >= 0) { rd.pg_part = s->pg_partials + s->pg_half; rd.pg_nblk = &pc.pg_defer_nblk; riders = true; }
        if (pc.iter_snap_slot >= 0) {
            const int b = pc.iter_snap_slot;
            const int arc = ensure_snapshot(s, b); if (arc) return arc;
            rd.snap_x = pc.snap[b] + (side == 0 ? (size_t)s->m * k2 : 0);        // snapshot_kernel's layout: [W'][H][W'W]
            rd.k2 = k2;
            riders = true;
        }
    }
    const int rc = launch_nnls_bpp(X, nullptr, s->k, c0, c1, R, G, s->fail_flag, s->iter, inv_scratch(s, side), hs.inverse_ready() ? 1 : 0, ctx().cus, s->st,
                                   want ? s->gram_scratch : nullptr, want ? &hx.gram_partials : nullptr, pack ? &pk : nullptr,
                                   riders ? &rd : nullptr);
    if (!rc && rd.pg_part) {
        // the totals of the deferred check are due: they ride in the tail of the pass that follows (prod2), or go out as a launch
        // of their own right in front of it (check_totals)
        if (pc.pg_defer_nblk <= 0) { set_error("the deferred progress check was not carried by the NNLS launch"); return SMK_FAILURE; }
        pc.pg_totals_slot = pc.pg_defer_slot;
        pc.pg_defer_slot = -1;
    }
    if (!rc && (X == s->H || X == s->Wt)) {
        hx.from_nnls = c0 == 0 && c1 == N;
        hx.packed_by_solve = pack && hx.gram_partials > 0;
    }
    // without the side stream (k <= 32) a first launch at k > 32 computes the inverse itself, in stream order
    if (!rc && c1 > c0 && (s->KP >= 64 || (s->KP == 32 && nnls_inverse_at_32()))) hs.inverse_formed_by_solve();
    return rc;
}

// ---- building blocks -----------------------------------------------------------------------
// every pass starts here: is it one of the timed samples?
static inline void begin_pass(smk_solver* s, int which)
{
    if (!s->timing.on) { s->timing.pass_timed[which] = false; return; }
    const unsigned c = s->timing.pass_counter[which]++;
    s->timing.pass_timed[which] = s->timing.stride <= 1 || (c % (unsigned)s->timing.stride) == 0;
    if (s->timing.pass_timed[which]) ++s->timing.pass_sampled[which];
}

// one launch of the streaming product, bracketed by events when timing is on; `counts`: this launch completes a pass
static int timed_bigprod(smk_solver* s, int which, const BigProdPlan& pl_in, const void* B, i64 ldb, const void* Xp,
                         double* P, int counts = 1)
{
    BigProdPlan pl = pl_in;
    Handoff& h = s->hand[which];
    if (h.take_inverse_ride() && bigprod_supports_ride(pl)) {       // start_inverse: this factor's Gram inverse rides in the launch
        pl.inv_ride.G = which == 0 ? s->Gw : s->Gh;
        pl.inv_ride.k = s->k;
        pl.inv_ride.Ginv = inv_scratch(s, which);
    }
    const bool timed = s->timing.on && s->timing.pass_timed[which];
    Timing::TimedSpan sp{};
    if (timed) {
        if (span_open(s, &sp, counts)) return SMK_DEVICE_ERROR;
        s->timing.ev[which].push_back(sp);
        SMK_HIP(hipEventRecord(sp.e0, s->st));
    }
    int rc = launch_bigprod(pl, B, ldb, Xp, P, s->st);
    if (rc == 1) { h.inverse_carried(); rc = 0; }
    if (timed) {
        if (rc) { s->timing.ev[which].pop_back(); s->timing.span_pool.push_back(sp); return rc; }
        SMK_HIP(hipEventRecord(sp.e1, s->st));
    }
    return rc;
}

// R1 = W'A  (k x n, local columns)
static int timed_spmm(smk_solver* s, int which, const i64* colptr, const unsigned* rowidx, const double* val, i64 ncols,
                      const double* X, int ldx, double* P)
{
    Timing::TimedSpan sp{};
    const bool timed = s->timing.on && s->timing.pass_timed[which];
    if (timed) {
        if (span_open(s, &sp)) return SMK_DEVICE_ERROR;
        (void)hipEventRecord(sp.e0, s->st);
    }
    int rc = 0;
    const BlockedCsc& blk = (which == 0) ? s->a->bA : s->a->bAt;
    const SegPlan& seg = (which == 0) ? s->a->segA : s->a->segAt;
    Handoff& h = s->hand[which];
    InvRide ride;                                                   // start_inverse: this factor's Gram inverse rides in the launch
    if (h.take_inverse_ride()) { ride.G = which == 0 ? s->Gw : s->Gh; ride.k = s->k; ride.Ginv = inv_scratch(s, which); }
    GramRide gram;                                                  // gram_factor: this factor's Gram matrix is due
    const bool by_seg = seg_route(s, which, ldx, ncols);
    if (h.take_gram_ride()) {
        const double* F = which == 0 ? s->Wt : s->H;
        const i64 FN = which == 0 ? s->m : s->n;
        double* G = which == 0 ? s->Gw : s->Gh;
        if (by_seg) { gram.X = F; gram.N = FN; gram.max_blocks = GRAM_BLOCKS; gram.Gp = s->gram_scratch; gram.G = G; }
        else rc = launch_gram(F, s->k, FN, G, s->gram_scratch, GRAM_BLOCKS, s->st);
    }
    if (!rc) {        // a failure, the Gram launch's or one below, launches nothing more and reaches the span's clean-up, not a return
        if (blocked2_route(s, which, ldx)) rc = launch_spmm_blocked2(blk, X, P, which == 0 ? s->pl1.ncols_pad : s->pl2.ncols_pad, s->st);
        else if (by_seg) {
            // the partial sums of long columns live in the SOLVER (two solvers on one sparse matrix run on their own streams)
            if (seg.npieces > 0 && !s->seg_pieces[which] && s->own.dev(&s->seg_pieces[which], (size_t)seg.npieces * 128)) {
                set_error("no memory for the long-column partial sums");
                rc = SMK_DEVICE_ERROR;
            }
            if (!rc) rc = launch_spmm_seg(seg, colptr, val, X, s->k, P, s->kpp, s->st, s->seg_pieces[which], &ride, &gram);
            if (rc > 0 && (rc & 2)) rc &= ~2;                           // ... and the Gram matrix
            else if (rc >= 0 && gram.X) {                               // nothing was launched (a matrix without stored entries): the matrix by itself
                const int grc = launch_gram(gram.X, s->k, gram.N, gram.G, s->gram_scratch, GRAM_BLOCKS, s->st);
                if (grc) rc = grc;
            }
        }
        else rc = launch_spmm_gather(colptr, rowidx, val, ncols, s->a->nnz, X, ldx, s->k, P, s->kpp, s->st, &ride);
    }
    if (rc == 1) { h.inverse_carried(); rc = 0; }
    if (timed) {
        if (rc) { s->timing.span_pool.push_back(sp); return rc; }
        (void)hipEventRecord(sp.e1, s->st);
        s->timing.ev[which].push_back(sp);
    }
    return rc;
}

// W'A with a row-sharded W (BPP, native communicator): every rank packs its own blocks, the blocks of chunk j are
// all-gathered on st2 (packed operand: 4 B per entry in the fp16 form, half of the fp64 values) and the product is
// taken chunk by chunk down the contraction, each launch adding to P1, as soon as its chunk of the operand has landed.
static int prod1_sharded(smk_solver* s)
{
    begin_pass(s, 0);
    const int storage = s->a->storage;
    const size_t es = (size_t)elem_size(storage);
    const bool f64 = s->nsplit == NSPLIT_F64;       // the accurate form reads the fp64 factor: gather the fp64 own blocks into W itself
    int rc = 0;
    // one launch per group of 64 factor rows: this rank's blocks into their places in the operand (padding rows as zeros)
    for (int g = 0; g < s->ng && !rc && !f64; ++g)
        rc = launch_pack_own_blocks(s->ex.Wown, s->KP, s->pg1[g].k0, s->pg1[g].kg, s->ex.n_own, s->ex.blk, s->ex.nchunk, s->ex.world, s->ex.rank, storage,
                                    s->nsplit, (unsigned char*)s->packW + s->pg1[g].pack_offset, s->st, s->xscale[0]);
    if (rc) return rc;
    rc = comm_fork(s, s->ex.ev_x);
    if (rc) return rc;
    for (int j = 0; j < s->ex.nchunk; ++j) {
        i64 r0, r1;
        chunk_rows(s, j, &r0, &r1);
        rc = timed_collective(s, 0, [&] {
            if (f64)        // block r of chunk j from every rank, straight into its rows of the full fp64 W
                return comm_allgather_to(s->ex.comm, s->ex.Wown + (i64)j * s->ex.blk * s->KP, s->Wt + r0 * s->KP, s->ex.blk * s->KP, 1, s->ex.st2);
            for (int g = 0; g < s->ng; ++g) {
                const size_t per = packed_row_offset(storage, s->pg1[g].kg, s->nsplit, s->ex.blk);          // bytes per block
                unsigned char* base = (unsigned char*)s->packW + s->pg1[g].pack_offset + packed_row_offset(storage, s->pg1[g].kg, s->nsplit, r0);
                const int grc = comm_allgather(s->ex.comm, base, (i64)(per / 4), 0, s->ex.st2);
                if (grc) return grc;
            }
            return 0;
        });
        if (rc) return rc;
        SMK_HIP(hipEventRecord(s->ex.ev_a[j], s->ex.st2));
    }
    bool first = true;
    for (int j = 0; j < s->ex.nchunk; ++j) {
        i64 r0, r1;
        chunk_rows(s, j, &r0, &r1);
        { const int wrc = main_waits_for_comm(s, &s->ex.ev_a[j], 1); if (wrc) return wrc; }
        const i64 rows = std::min<i64>(r1, s->m) - r0;
        if (rows <= 0) continue;
        const bool last = (j == s->ex.nchunk - 1) || (std::min<i64>(r1, s->m) >= s->m);
        for (int g = 0; g < s->ng; ++g) {
            BigProdPlan pl = s->pg1[g];
            pl.stages = (rows + pl.mb - 1) / pl.mb;
            pl.nst = (pl.stages + pl.S - 1) / pl.S;
            pl.accum = first ? 0 : 1;
            const void* Xp = (const unsigned char*)s->packW + pl.pack_offset + packed_row_offset(storage, pl.kg, s->nsplit, r0);
            if (f64) { pl.len = rows; Xp = s->Wt + r0 * s->KP + pl.k0; }     // rows [r0, r0 + rows) of the gathered W, this group's factor rows
            rc = timed_bigprod(s, 0, pl, (const unsigned char*)s->a->A + (size_t)r0 * es, s->a->ldA, Xp, s->P1 + pl.k0, last ? 1 : 0);
            if (rc) return rc;
        }
        first = false;
    }
    if (f64) s->ex.w_full = true;       // every row of the fp64 W is current again (a by-product of the accurate form's gather)
    return 0;
}

// the product of factor `side` (0 = W, 1 = H) takes the pending reduction of that factor's Gram partials along (gram_factor)
static inline void take_tail(smk_solver* s, int side, BigProdPlan* pl)
{
    Handoff& h = s->hand[side];
    if (h.tail_nblk <= 0) return;
    pl->tail_gp = s->gram_scratch;
    pl->tail_nblk = h.tail_nblk;
    pl->tail_g = side == 0 ? s->Gw : s->Gh;
    h.tail_nblk = 0;
}

static int prod1(smk_solver* s)
{
    if (s->ex.w_sharded) return prod1_sharded(s);
    begin_pass(s, 0);
    if (s->a->sparse) {
        if (s->Wc) {        // RANK2: gather from the compact copy of W (16 B per row)
            if (!s->wc_valid) { const int crc = launch_rank2_compact(s->Wt, s->Wc, s->m, s->st); if (crc) return crc; s->wc_valid = true; }
            return timed_spmm(s, 0, s->a->colptr, s->a->rowidx, s->a->val, s->n, s->Wc, 2, s->P1);
        }
        return timed_spmm(s, 0, s->a->colptr, s->a->rowidx, s->a->val, s->n, s->Wt, s->KP, s->P1);
    }
    int rc = 0;
    const bool f64 = s->nsplit == NSPLIT_F64;                 // the accurate form reads the fp64 factor itself
    if (!s->hand[0].packed_fresh && !f64) rc = launch_pack(s->Wt, s->k, s->m, s->a->storage, s->nsplit, s->packW, s->st, s->xscale[0]);
    s->hand[0].packed_fresh = false;
    if (rc) return rc;
    for (int g = 0; g < s->ng; ++g) {
        const void* Xp = f64 ? (const void*)(s->Wt + s->pg1[g].k0) : (const void*)((const unsigned char*)s->packW + s->pg1[g].pack_offset);
        BigProdPlan pl = s->pg1[g];
        take_tail(s, 0, &pl);
        rc = timed_bigprod(s, 0, pl, s->a->A, s->a->ldA, Xp, s->P1 + s->pg1[g].k0);
        if (rc) return rc;
    }
    return 0;
}

// R2 = H At = (A H')'  (k x m), summed over ranks when sharded.  With a native communicator the pass runs chunk by
// chunk over the rows of A and the sum of chunk j (reduce-scatter for the row-sharded BPP solve, all-reduce otherwise)
// travels on st2 while the product streams chunk j + 1; consumers call wait_r2().
static int prod2(smk_solver* s)
{
    begin_pass(s, 1);
    int rc = 0;
    const PartialView pv{s->P2, s->pl2.S, (i64)s->pl2.ncols_pad * s->kpp, s->kpp, 1};
    if (s->pc.pg_totals_slot >= 0 && (s->a->sparse || s->ex.comm || s->ng != 1 || s->hand[1].tail_nblk <= 0)) {
        rc = check_totals(s, nullptr);                  // no tail to ride in
        if (rc) return rc;
    }
    if (s->a->sparse) {
        rc = s->Hc ? timed_spmm(s, 1, s->a->colptr_t, s->a->rowidx_t, s->a->val_t, s->m, s->Hc, 2, s->P2)
                   : timed_spmm(s, 1, s->a->colptr_t, s->a->rowidx_t, s->a->val_t, s->m, s->H, s->KP, s->P2);
        if (rc) return rc;
        rc = wait_gh(s);
        if (rc || !is_dist(s)) return rc;
        rc = launch_reduce_partials(pv, s->k, 0, s->pl2.ncols_pad, s->R2red, s->ex.red_f64 ? 1 : 0, s->st);
        if (rc) return rc;
        if (!s->ex.comm) return dist_allreduce_cb(s, s->R2red, (i64)s->pl2.ncols_pad * s->kpp, 0);
        rc = comm_fork(s, s->ex.ev_c[0]);
        if (rc) return rc;
        rc = timed_collective(s, 1, [&] { return comm_allreduce(s->ex.comm, s->R2red, (i64)s->pl2.ncols_pad * s->kpp, s->ex.red_f64 ? 1 : 0, s->ex.st2); });
        if (rc) return rc;
        return comm_join(s, s->ex.ev_r[0]);
    }
    const bool f64 = s->nsplit == NSPLIT_F64;
    if (!s->hand[1].packed_fresh && !f64) rc = launch_pack(s->H, s->k, s->n, s->a->storage, s->nsplit, s->packH, s->st, s->xscale[1]);
    s->hand[1].packed_fresh = false;
    if (rc) return rc;
    auto xh = [&](const BigProdPlan& pl) -> const void* {
        return f64 ? (const void*)(s->H + pl.k0) : (const void*)((const unsigned char*)s->packH + pl.pack_offset);
    };
    if (!s->ex.comm) {
        for (int g = 0; g < s->ng && !rc; ++g) {
            BigProdPlan pl = s->pg2[g];
            take_tail(s, 1, &pl);
            const int ride = check_totals(s, &pl);
            if (ride < 0 || ride > 1) return ride;
            rc = pl.tr ? timed_bigprod(s, 1, pl, s->a->A, s->a->ldA, xh(s->pg2[g]), s->P2 + s->pg2[g].k0)
                       : timed_bigprod(s, 1, pl, s->a->At, s->a->ldAt, xh(s->pg2[g]), s->P2 + s->pg2[g].k0);
            if (ride == 1 && !rc) {
                if (s->pc.poll_tag[s->pc.pg_totals_slot] == 0.0) SMK_HIP(hipEventRecord(s->pc.pev[s->pc.pg_totals_slot], s->st));
                s->pc.pg_totals_slot = -1;
            }
        }
        if (rc) return rc;
        rc = wait_gh(s);
        if (rc || !is_dist(s)) return rc;
        rc = launch_reduce_partials(pv, s->k, 0, s->pl2.ncols_pad, s->R2red, 0, s->st);
        if (rc) return rc;
        return dist_allreduce_cb(s, s->R2red, (i64)s->pl2.ncols_pad * s->kpp, 0);
    }
    const size_t es = (size_t)elem_size(s->a->storage), rb = s->ex.red_f64 ? sizeof(double) : sizeof(float);
    for (int j = 0; j < s->ex.nchunk; ++j) {
        i64 r0, r1;
        chunk_rows(s, j, &r0, &r1);
        for (int g = 0; g < s->ng; ++g) {
            BigProdPlan pl = s->pg2[g];
            pl.tiles = (r1 - r0 + pl.nb - 1) / pl.nb;
            if (pl.tr && r0 + pl.tiles * pl.nb > s->a->ldA) { set_error("transposed-source chunk runs past the padded rows of A"); return SMK_FAILURE; }
            // rows [r0, r1) of A: columns of the stored transpose, or -- single copy -- a row offset into A itself
            const unsigned char* Bsrc = pl.tr ? (const unsigned char*)s->a->A + (size_t)r0 * es
                                              : (const unsigned char*)s->a->At + (size_t)r0 * s->a->ldAt * es;
            rc = timed_bigprod(s, 1, pl, Bsrc, pl.tr ? s->a->ldA : s->a->ldAt,
                               xh(pl), s->P2 + pl.k0 + r0 * pl.pstride, j == s->ex.nchunk - 1 ? 1 : 0);
            if (rc) return rc;
        }
        rc = comm_fork(s, s->ex.ev_c[j]);
        if (rc) return rc;
        // off the main stream: the row splits of the chunk summed (and rounded to the wire type), then its exchange
        if (!s->ex.r2_alias) { rc = launch_reduce_partials(pv, s->k, r0, r1 - r0, s->R2red, s->ex.red_f64 ? 1 : 0, s->ex.st2); if (rc) return rc; }
        unsigned char* base = (unsigned char*)s->R2red + (size_t)r0 * s->kpp * rb;
        rc = timed_collective(s, 1, [&] {
            if (s->ex.w_sharded)       // every rank receives the sum of ITS block, next to its other blocks
                return comm_reduce_scatter_to(s->ex.comm, base, (unsigned char*)s->ex.R2own + (size_t)j * s->ex.blk * s->kpp * rb, s->ex.blk * s->kpp,
                                              s->ex.red_f64 ? 1 : 0, s->ex.st2);
            return comm_allreduce(s->ex.comm, base, (r1 - r0) * s->kpp, s->ex.red_f64 ? 1 : 0, s->ex.st2);
        });
        if (rc) return rc;
        SMK_HIP(hipEventRecord(s->ex.ev_r[j], s->ex.st2));
    }
    s->ex.r2_pending = true;
    return wait_gh(s);
}

// Gram matrix of a factor; for dense A the same launch also writes the packed operand of the product that follows
// (every schedule calls gram_x and prod_x back to back)
static int gram_factor(smk_solver* s, int side)
{
    const double* X = side == 0 ? s->Wt : s->H;
    const i64 N = side == 0 ? s->m : s->n;
    double* G = side == 0 ? s->Gw : s->Gh;
    Handoff& h = s->hand[side];
    h.packed_fresh = false;
    h.gram_ride = false;
    {
        // Sparse A: the gather product that follows in every schedule reads the same factor, and its two launches (segments, long-column
        // fix-up) carry the Gram matrix along -- partial sums as extra workgroups of the first, their reduction as extra workgroups of
        // the second (spmm_seg.hip, gram_body.h): four launches become two (the Reuters shape under HALS: 102 -> 84 us per iteration).
        // Not where block pivoting needs the inverse of this matrix in the SAME launch (k in (16, 32]: that one rides, start_inverse).
        // A product that takes another route forms the matrix first, as before (timed_spmm).  SMK_GRAM_RIDE=0: never rides.
        const bool ride = sw::gram_ride();
        const bool inverse_next = s->o.algorithm == SMK_ALG_BPP && (s->KP == 64 || (s->KP == 32 && nnls_inverse_at_32()));
        if (ride && s->a->sparse && !is_dist(s) && !s->ex.comm && !s->ex.w_sharded && (s->KP == 16 || s->KP == 32) && s->k > 2 && !inverse_next &&
            s->o.algorithm != SMK_ALG_RANK2) {
            h.gram_ride = true;
            return 0;
        }
    }
    if (side == 0 && s->ex.w_sharded) {
        // W'W from this rank's own rows, summed over the ranks; the fp16 row scales follow the finished matrix
        int rc = s->ex.n_own > 0 ? launch_gram(s->ex.Wown, s->k, s->ex.n_own, G, s->gram_scratch, GRAM_BLOCKS, s->st)
                              : launch_zero_f64(G, (i64)s->KP * s->KP, s->st);
        if (rc) return rc;
        rc = dist_allreduce_now(s, G, (i64)s->KP * s->KP, 1);
        if (rc) return rc;
        if (s->nsplit == NSPLIT_F16X2) return launch_gram_scales(G, s->k, s->xscale[0], s->oscale[0], (double)s->a->ascale, s->st);
        return 0;
    }
    if (s->nsplit == NSPLIT_F16X2) {     // the reduce launch also derives the row scales of the operand packed next
        if (h.gram_partials > 0) {                   // the NNLS launch that solved THIS factor left them
            const int nb = h.gram_partials;
            h.gram_partials = 0;
            // the solve packed the operand itself: nothing is needed before the product, which takes the reduction along
            if (h.packed_by_solve) {
                h.packed_by_solve = false;
                h.packed_fresh = true;
                h.tail_nblk = nb;
                return 0;
            }
            // ... and packs it in the same launch (the packing workgroups add up the 16 diagonal entries themselves)
            const bool fuse_pack = sw::reduce_pack();
            if (fuse_pack && !s->a->sparse) {
                const int rc = launch_reduce_pack_f16x2(s->gram_scratch, nb, s->k, G, s->xscale[side], s->oscale[side], (double)s->a->ascale, X, N,
                                                        s->a->storage, side == 0 ? s->packW : s->packH, s->st);
                if (rc == 0) { h.packed_fresh = true; return 0; }
                if (rc != 1) return rc;
            }
            return launch_gram_reduce(s->gram_scratch, nb, s->k, G, s->st, s->xscale[side], s->oscale[side], (double)s->a->ascale);
        }
        return launch_gram(X, s->k, N, G, s->gram_scratch, GRAM_BLOCKS, s->st, s->xscale[side], s->oscale[side], (double)s->a->ascale);
    }
    // (k > 16.  Leaving the partial sums to the pack launch -- every pack thread adding up its diagonal entry, workgroup 0
    // finishing the matrix -- costs 12 us where reduce + pack cost 9.5; what works, at k <= 16 above, is separate reducer
    // workgroups in the same launch and packers that read a compact copy of the diagonal partials.)
    if (!s->a->sparse && s->o.algorithm != SMK_ALG_RANK2 && s->nsplit != NSPLIT_F64) {
        const int rc = launch_gram_pack(X, s->k, N, G, s->gram_scratch, GRAM_BLOCKS, s->a->storage, s->nsplit,
                                        side == 0 ? s->packW : s->packH, s->st);
        if (rc == 0) { h.packed_fresh = true; return 0; }
        if (rc != 1) return rc;
    }
    return launch_gram(X, s->k, N, G, s->gram_scratch, GRAM_BLOCKS, s->st);
}

static int gram_w(smk_solver* s)
{
    int rc = gram_factor(s, 0);
    if (rc) return rc;
    return start_inverse(s, 0, s->Gw);
}

static int gram_h(smk_solver* s)
{
    int rc = gram_factor(s, 1);
    if (rc) return rc;
    rc = allreduce_gh(s);
    if (rc) return rc;
    // sharded: HH' is final only after its all-reduce -- in stream order with the callback hook, on the second stream
    // (event ev_gh) with a native communicator; either way the inversion runs beside the H*At pass
    return start_inverse(s, 1, s->Gh, (is_dist(s) && s->ex.gh_pending) ? s->ex.ev_gh : nullptr);
}

// row-sharded W: bring every row of the fp64 W to every rank (results, DELTA_FNORM); one in-place all-gather per chunk
extern "C++" int smk::gather_w(smk_solver* s)
{
    if (!s->ex.w_sharded || s->ex.w_full) return 0;
    int rc = comm_fork(s, s->ex.ev_x);
    if (rc) return rc;
    for (int j = 0; j < s->ex.nchunk && !rc; ++j)
        rc = comm_allgather_to(s->ex.comm, s->ex.Wown + (i64)j * s->ex.blk * s->KP, s->Wt + (i64)j * s->ex.world * s->ex.blk * s->KP, s->ex.blk * s->KP, 1, s->ex.st2);
    if (rc) return rc;
    s->ex.w_full = true;
    return comm_join(s, s->ex.ev_y);
}

// solver.Init (mu :98-114, hals :142-159, bpp :310-335) + progress_est->Init
extern "C++" int smk::solver_init(smk_solver* s)
{
    int rc = 0;
    // the factors are the caller's (or a restored snapshot): nothing is known to come from an NNLS launch, nothing is pending
    s->forget_handoffs();
    s->pc.reset();
    if (s->o.algorithm == SMK_ALG_HALS) {
        rc = gram_h(s);  if (rc) return rc;
        rc = prod2(s);   if (rc) return rc;
    } else {   // MU, BPP, RANK2: WtA and WtW from W0
        rc = gram_w(s);  if (rc) return rc;
        rc = prod1(s);   if (rc) return rc;
    }
    if (s->o.prog_est_algorithm == SMK_PROG_DELTA_FNORM) {
        rc = gather_w(s); if (rc) return rc;
        SMK_HIP(hipMemcpyAsync(s->Wprev, s->Wt, (size_t)s->KP * s->m * sizeof(double), hipMemcpyDeviceToDevice, s->st));
    }
    s->inited = true;
    return 0;
}

// one solver iteration (the body of `solver(A,W,H,gradW,gradH)`); gradients are formed on
// demand by update_progress() from the same R1/R2/Gw/Gh the reference uses.
static int solver_iteration(smk_solver* s)
{
    int rc = 0;
    s->normalized = false;          // the factors are about to change
    const PartialView r1 = view1(s), r2 = view2(s);
    switch (s->o.algorithm) {
        case SMK_ALG_MU:   // nmf_solver_mu.hpp:121-164
            rc = launch_mu_update(s->H, s->k, s->n, r1, s->Gw, s->st, s->wide_tmp);  if (rc) return rc;
            rc = gram_h(s);   if (rc) return rc;
            rc = prod2(s);    if (rc) return rc;
            rc = wait_r2(s);  if (rc) return rc;
            if (s->ex.w_sharded) {       // own blocks only (back to back in Wown, their rows of the summed (AH')' in R2own)
                if (s->ex.n_own > 0) { rc = launch_mu_update(s->ex.Wown, s->k, s->ex.n_own, view_own(s), s->Gh, s->st, s->wide_tmp); if (rc) return rc; }
                s->ex.w_full = false;
            } else {
                rc = launch_mu_update(s->Wt, s->k, s->m, r2, s->Gh, s->st, s->wide_tmp); if (rc) return rc;
            }
            rc = gram_w(s);   if (rc) return rc;
            rc = prod1(s);    if (rc) return rc;
            break;
        case SMK_ALG_HALS: { // nmf_solver_hals.hpp:166-199
            // round 6: at k <= 32 on one GPU both sweeps also leave the packed operand of the product that follows and their Gram
            // partials (kernels.hip: tile_pack_gram) -- the separate gram_pack launches (11 us each at C3) go, only the 5 us
            // reductions stay.  SMK_HALS_EPILOGUE=0: the launches of before.
            const bool ep_on = sw::hals_epilogue();
            const bool bf16_frag = s->a->storage == SMK_STORE_BF16 || s->nsplit >= 2;
            const bool ep_ok = ep_on && !s->a->sparse && !is_dist(s) && !s->ex.comm && (s->KP == 16 || s->KP == 32) && bf16_frag && s->nsplit >= 1 && s->nsplit <= 3 &&
                               s->ng == 1 && s->hals_ep_blocks > 0;
            HalsEpilogue epw, eph;
            if (ep_ok) {
                epw.pack_out = (unsigned char*)s->packW; epw.Gp = s->gram_scratch; epw.KT = kt_of(s->k); epw.nsplit = s->nsplit;
                epw.max_blocks = s->hals_ep_blocks; epw.nq = round_up(s->m, 128) / 16;
                eph = epw;
                eph.pack_out = (unsigned char*)s->packH; eph.nq = round_up(s->n, 128) / 16;
            }
            rc = wait_r2(s);  if (rc) return rc;
            rc = launch_hals_w_update(s->Wt, s->k, s->m, r2, s->Gh, s->hals_scratch, ctx().cus, s->fail_flag, s->hals_calls++, s->hals_multi ? 1 : 0, s->st,
                                      ep_ok ? &epw : nullptr); if (rc) return rc;
            if (epw.done) { rc = launch_gram_reduce(s->gram_scratch, epw.nblk, s->k, s->Gw, s->st, nullptr, nullptr, 1.0); s->hand[0].packed_fresh = true; }
            else rc = gram_w(s);
            if (rc) return rc;
            rc = prod1(s);    if (rc) return rc;
            rc = launch_hals_sweep(s->H, s->k, s->n, r1, s->Gw, s->st, ep_ok ? &eph : nullptr); if (rc) return rc;
            if (eph.done) { rc = launch_gram_reduce(s->gram_scratch, eph.nblk, s->k, s->Gh, s->st, nullptr, nullptr, 1.0); s->hand[1].packed_fresh = true; }
            else rc = gram_h(s);
            if (rc) return rc;
            rc = prod2(s);    if (rc) return rc;
            break;
        }
        case SMK_ALG_BPP:  // nmf_solver_bpp.hpp:342-377
            rc = nnls_side(s, 0, s->H, 0, s->n, r1, s->Gw); if (rc) return rc;
            rc = gram_h(s);   if (rc) return rc;
            rc = prod2(s);    if (rc) return rc;
            if (s->ex.w_sharded) {
                // W is replicated in the algorithm but its rows are independent NNLS problems: every rank solves its own
                // blocks (held back to back, one launch) once the last slice of the reduce-scatter has landed
                rc = wait_r2(s);  if (rc) return rc;
                rc = nnls_side(s, 1, s->ex.Wown, 0, s->ex.n_own, view_own(s), s->Gh); if (rc) return rc;
                s->ex.w_full = false;
            } else if (s->ex.ar && s->ex.world > 1) {
                // callback hook (one primitive only): every rank solves a row range, zeroes the rest and sum-all-reduces
                const i64 base = s->m / s->ex.world, extra = s->m % s->ex.world;
                const i64 i0 = s->ex.rank * base + (s->ex.rank < extra ? s->ex.rank : extra);
                const i64 i1 = i0 + base + (s->ex.rank < extra ? 1 : 0);
                rc = nnls_side(s, 1, s->Wt, i0, i1, r2, s->Gh); if (rc) return rc;
                if (i0 > 0) SMK_HIP(hipMemsetAsync(s->Wt, 0, (size_t)i0 * s->KP * sizeof(double), s->st));
                if (i1 < s->m) SMK_HIP(hipMemsetAsync(s->Wt + i1 * s->KP, 0, (size_t)(s->m - i1) * s->KP * sizeof(double), s->st));
                rc = dist_allreduce_cb(s, s->Wt, (i64)s->KP * s->m, 1); if (rc) return rc;
            } else {
                rc = wait_r2(s);  if (rc) return rc;
                rc = nnls_side(s, 1, s->Wt, 0, s->m, r2, s->Gh); if (rc) return rc;
            }
            rc = gram_w(s);   if (rc) return rc;
            rc = prod1(s);    if (rc) return rc;
            break;
        case SMK_ALG_RANK2:  // nmf_solver_rank2.hpp:353-455
            // each closed-form solve also emits partial sums of the Gram matrix of its result (no second pass over H / W),
            // which the kernel that needs the matrix adds up itself (rank2.hip)
            {
                double *GpH = s->r2_scratch, *GpW = s->r2_scratch + rank2_gram_scratch_elems(std::max(s->m, s->n)) / 2;
                int nbh = 0, nbw = 0;
                rc = launch_rank2_solve(s->H, s->Hc, s->n, r1, s->Gw, nullptr, 0, 0, s->fail_flag, s->iter, GpH, &nbh, s->Gh,
                                        is_dist(s) ? 1 : 0, s->st); if (rc) return rc;       // sharded: HH' is finished here and summed over the ranks
                rc = allreduce_gh(s); if (rc) return rc;
                rc = prod2(s);    if (rc) return rc;
                rc = wait_r2(s);  if (rc) return rc;
                rc = launch_rank2_solve(s->Wt, nullptr, s->m, r2, s->Gh, GpH, nbh, 1, s->fail_flag, s->iter, GpW, &nbw, s->Graw, 0, s->st); if (rc) return rc;
                // NormalizeAndScale(W, H, ScaleFactors) every iteration, norms from the Gram matrix of the new W;
                // also rescales HH' and AH', leaves Gw = W'W of the normalised W (D^-1 Graw D^-1) and the compact copy of W
                rc = launch_rank2_normalize(s->H, s->n, s->Wt, s->Wc, s->m, r2, s->Gh, s->Graw, GpW, nbw, s->Gw, s->fail_flag, s->st); if (rc) return rc;
                s->wc_valid = s->Wc != nullptr;
            }
            rc = prod1(s);    if (rc) return rc;
            break;
        default:
            return SMK_UNSUPPORTED;
    }
    s->iter += 1;
    return 0;
}

// wait for the stream; translate device-side failure flags into Result codes
extern "C++" int smk::sync_and_check(smk_solver* s, int* fail_iter)
{
    int flag = INT_MAX;
    int rc = wait_r2(s);                 // chunk exchanges still on the second stream
    if (rc) return rc;
    SMK_HIP(hipMemcpyAsync(&flag, s->fail_flag, sizeof(int), hipMemcpyDeviceToHost, s->st));
    SMK_HIP(hipStreamSynchronize(s->st));
    rc = resolve_events(s);
    if (rc) return rc;
    if (fail_iter) *fail_iter = flag;
    if (flag != INT_MAX) return SMK_FAILURE;
    return SMK_OK;
}

// sharded: sum the H-side scalar over the ranks and make the failure flag the same everywhere, so that every
// rank takes the same branch of the driver loop (a rank that stopped alone would strand the others in a collective)
extern "C++" int smk::dist_agree(smk_solver* s)
{
    const int wpart = w_rows_sharded(s) ? 1 : 0;      // the W-side sum covers this rank's rows only
    int rc = launch_dist_scalars(s->scal, s->fail_flag, s->iter > 0 ? s->iter - 1 : 0, 0, wpart, s->st);
    if (rc) return rc;
    rc = dist_allreduce_now(s, s->scal + 5, 3, 1);
    if (rc) return rc;
    return launch_dist_scalars(s->scal, s->fail_flag, s->iter > 0 ? s->iter - 1 : 0, 1, wpart, s->st);
}

extern "C++" int smk::normalize_device(smk_solver* s)
{
    if (s->normalized) return 0;
    { const int grc = gather_w(s); if (grc) return grc; }
    // nu_c^2 = (W'W)[c][c]; Gw is current in all three schedules after the last W update
    int rc = launch_scale_rows(s->H, s->k, s->n, s->Gw, 0, s->fail_flag, s->st);
    if (rc) return rc;
    rc = launch_scale_rows(s->Wt, s->k, s->m, s->Gw, 1, s->fail_flag, s->st);
    if (rc) return rc;
    if (s->ex.w_sharded) { rc = scatter_own(s); if (rc) return rc; }      // the own rows follow the scaled full copy
    s->wc_valid = false;
    s->normalized = true;
    // Gw/Gh and the stored products describe the un-normalised factors: a later iterate()/run() on this
    // handle starts from solver.Init on the scaled (W, H), exactly like a fresh solver given them
    s->inited = false;
    return 0;
}

// what both fail-soft paths below end with: the initial factors again, a clean failure flag, a run from the start (returns 1)
static int restart_from_initial_factors(smk_solver* s)
{
    const int big = INT_MAX;
    (void)hipMemcpyAsync(s->Wt, s->W0c, (size_t)s->KP * s->m * sizeof(double), hipMemcpyDeviceToDevice, s->st);
    (void)hipMemcpyAsync(s->H, s->H0c, (size_t)s->KP * s->n * sizeof(double), hipMemcpyDeviceToDevice, s->st);
    (void)hipMemcpyAsync(s->fail_flag, &big, sizeof(int), hipMemcpyHostToDevice, s->st);
    (void)hipStreamSynchronize(s->st);
    s->inited = false;
    s->normalized = false;
    s->iter = 0;
    s->pc.reset_estimator();
    return 1;
}

// The fused HALS W sweep reported expired polls (-3: some workgroup was not resident): go back to the initial
// factors and latch the one-launch-per-column path.  Returns 1 when the caller should repeat its work.
static int hals_fail_soft(smk_solver* s)
{
    if (s->o.algorithm != SMK_ALG_HALS || s->hals_multi || !s->W0c) return 0;
    int flag = INT_MAX;
    if (hipMemcpy(&flag, s->fail_flag, sizeof(int), hipMemcpyDeviceToHost) != hipSuccess || flag != -3) return 0;
    fprintf(stderr, "smallk_amd: fused HALS W sweep could not keep its workgroups resident; repeating the run on the per-column path\n");
    s->hals_multi = true;
    (void)hals_w_scratch_init(s->hals_scratch, s->k, s->m, s->st);
    return restart_from_initial_factors(s);
}

// An NNLS launch that packs its own result (NnlsPack) met an entry beyond fp16's range after scaling (flag -4): the a-priori
// bound behind its row scales did not hold -- it cannot while the other factor is non-negative and the solve reaches a KKT
// point, so this is a safety net.  Back to the initial factors with the packing latched off for the life of the handle.
// Returns 1 when the caller should repeat its work.
static int pack_fail_soft(smk_solver* s)
{
    if (!s->pack_in_solve || s->pack_in_solve_off || !s->W0c) return 0;
    int flag = INT_MAX;
    if (hipMemcpy(&flag, s->fail_flag, sizeof(int), hipMemcpyDeviceToHost) != hipSuccess || flag != NNLS_PACK_OVERFLOW) return 0;
    fprintf(stderr, "smallk_amd: an NNLS launch could not pack its result inside fp16's range; repeating the run with the separate pack launch\n");
    s->pack_in_solve_off = true;
    return restart_from_initial_factors(s);
}

int smk_solver_iterate(smk_solver* s, int iters)
{
    if (!s || iters < 0) return SMK_BAD_PARAM;
    if (!s->have_factors) { set_error("set_factors() first"); return SMK_BAD_PARAM; }
    int rc = 0;
    if (!s->inited) { rc = solver_init(s); if (rc) return rc; }
    for (int i = 0; i < iters; ++i) {
        rc = solver_iteration(s);
        if (rc) return rc;
        rc = guard_step(s);
        if (rc) return rc;
    }
    return SMK_OK;
}

// One iteration of a checked loop (the "run one iteration" operation of check_ring.h).  snap_slot >= 0: the check that follows wants
// a snapshot in that slot, and where the check rides in the NNLS launches (check_rides_in_nnls) those launches write it themselves;
// progress_begin takes the promise back.
static int checked_iteration(smk_solver* s, int snap_slot)
{
    s->pc.iter_snap_slot = (snap_slot >= 0 && check_rides_in_nnls(s)) ? snap_slot : -1;
    int rc = solver_iteration(s);
    if (!rc) rc = guard_step(s);
    if (rc) s->pc.iter_snap_slot = -1;
    return rc;
}

// `iters` iterations as NmfSolve<> runs them past min_iter (nmf_solve_generic.hpp:98-121): after every iteration the stopping rule's
// metric is formed (gradients for PG_RATIO, nmf_solver_bpp.hpp:370-377 / nmf_solver_mu.hpp:151-164; W - Wprev for DELTA_FNORM) and
// read back -- by the same one-iteration-late scheme as smk_solver_run (snapshot, pinned slot, event), with a tolerance that never
// fires.  What bench.py --check-every-iteration times.  *last_metric (optional): the metric of the last iteration.
int smk_solver_iterate_checked(smk_solver* s, int iters, double* last_metric)
{
    if (!s || iters < 0) return SMK_BAD_PARAM;
    if (!s->have_factors) { set_error("set_factors() first"); return SMK_BAD_PARAM; }
    int rc = 0;
    if (!s->inited) { rc = solver_init(s); if (rc) return rc; }
    if (s->o.algorithm == SMK_ALG_RANK2) { set_error("iterate_checked: MU / HALS / BPP"); return SMK_UNSUPPORTED; }
    check_ring::Params p;
    p.depth = progress_depth(s);
    p.max_iter = iters;
    p.every = true;
    p.base = s->iter;                               // the very first iteration of a run initialises the estimator (PG_RATIO: pg0)
    const check_ring::Result r = check_ring::drive(p,
        [s](int, int snap_slot) { return checked_iteration(s, snap_slot); },
        [s](int, int b, bool snapshot) { return progress_begin(s, b, snapshot); },
        [s](int i, int b, double* metric) { return progress_end(s, b, i, metric); },
        [](int, int) { return 0; }, [](const char*) {});
    if (!r.code && last_metric) *last_metric = r.metric;
    return r.code;
}

// which product form the solver is using now (SMK_NSPLIT numbering; 8 = the accurate form), how often the run-time guard has
// looked and how often it changed the form, and cond * delta of its last look
int smk_solver_product_form(const smk_solver* s, int* guard_checks, int* guard_fired, double* guard_last)
{
    if (!s) return SMK_BAD_PARAM;
    if (guard_checks) *guard_checks = s->guard.checks;
    if (guard_fired) *guard_fired = s->guard.fired;
    if (guard_last) *guard_last = s->guard.last;
    return s->nsplit;
}

int smk_solver_sync(smk_solver* s)
{
    if (!s) return SMK_BAD_PARAM;
    const int target = s->iter;
    int rc = gather_w(s);                 // every rank calls sync: the fp64 W is whole again afterwards
    if (rc) return rc;
    rc = sync_and_check(s, nullptr);
    if (rc == SMK_FAILURE && !is_dist(s) && (hals_fail_soft(s) || pack_fail_soft(s))) {
        rc = smk_solver_iterate(s, target);
        if (rc == SMK_OK) rc = sync_and_check(s, nullptr);
    }
    return rc;
}

int smk_solver_progress(smk_solver* s, double* metric)
{
    if (!s || !metric) return SMK_BAD_PARAM;
    if (!s->inited) return SMK_BAD_PARAM;
    return update_progress(s, s->iter > 0 ? s->iter - 1 : 0, metric);
}

// the four scalars evaluate_progress saw last and pg0: host state only, nothing is launched or read
int smk_solver_progress_sums(const smk_solver* s, double out5[5])
{
    if (!s || !out5) return SMK_BAD_PARAM;
    if (s->pc.sums_state == 0) { set_error("progress_sums: no check has been evaluated since set_factors()"); return SMK_BAD_PARAM; }
    if (s->pc.sums_state == 2) { set_error("progress_sums: the resident RANK2 kernel returns the metric only"); return SMK_UNSUPPORTED; }
    for (int i = 0; i < 4; ++i) out5[i] = s->pc.sums[i];
    out5[4] = s->pc.pg0;
    return SMK_OK;
}

int smk_solver_iteration_count(const smk_solver* s) { return s ? s->iter : 0; }

static int solver_run_once(smk_solver* s, smk_stats* stats);

// NmfSolve<>, common/include/nmf_solve_generic.hpp:34-140
int smk_solver_run(smk_solver* s, smk_stats* stats)
{
    int rc = solver_run_once(s, stats);
    if (rc == SMK_FAILURE && s && !is_dist(s) && (hals_fail_soft(s) || pack_fail_soft(s))) rc = solver_run_once(s, stats);
    return rc;
}

// ---- RANK2 on sparse A: the driver loop below as ONE launch (rank2_persist.hip) -------------------------------------------
// For small and medium node matrices an iteration is six 7 - 12 us launches on a few MB: launch-latency bound.  The
// resident kernel carries the loop, the stopping rule (PG_RATIO, min_iter / tolcount as NmfSolve<>), the per-iteration
// normalisation and the final state; the host waits for one 128-byte result.  Measured on the C5-shaped run
// (profiles/r04_c5_*): 54 -> 37 us per iteration on the 1 M-entry nodes (the two gather products alone are 24 us at the
// chip's ~84 G random 16-byte gathers per second), and it also wins on the large nodes (9 M entries: 495 -> 291 us, the
// 16 M-entry root 645 -> 556 us) because its entry-parallel products issue exactly one gather per stored entry with all of
// a chunk's gathers in flight -- so there is no size limit by default (SMK_R2_PERSIST_NNZ sets one, SMK_R2_PERSIST=0 turns
// the kernel off).
// devices on which a resident launch could not synchronise its workgroups (a CU mask, another process holding CUs): latched
// for the PROCESS, not per solver handle -- HierNMF2 and flatclust create a solver per node and per trial, and each would pay the
// start-up deadline again and print the warning again
static std::atomic<unsigned long long> g_r2p_off_devices{0};
static bool rank2_persist_eligible(const smk_solver* s)
{
    const int mode = sw::r2_persist();
    const i64 max_nnz = sw::r2_persist_nnz();
    if (!mode || s->r2p.off) return false;
    if (g_r2p_off_devices.load(std::memory_order_relaxed) & (1ull << (smk_current_device() & 63))) return false;
    if (s->o.algorithm != SMK_ALG_RANK2 || !s->a->sparse || s->o.prog_est_algorithm != SMK_PROG_PG_RATIO) return false;
    if (is_dist(s) || s->ex.comm || s->o.verbose || s->timing.on || !s->Hc || !s->Wc) return false;
    if (rank2_persist_workgroups(s->m, s->n, s->a->nnz, ctx().cus) < 1) return false;      // more than 4096 rows per workgroup
    return s->a->nnz <= max_nnz || mode == 2;
}

// returns 0 with *status = one of R2P_*: CONVERGED / EXHAUSTED (factors, W'W, counters in place), SOLVER_FAILED / NAN (the
// failure flag is set as the launch-per-kernel loop sets it), ABORTED (nothing was touched: the caller runs the classic loop)
static int rank2_persist_run(smk_solver* s, int* status, int* count)
{
    const int nwg = rank2_persist_workgroups(s->m, s->n, s->a->nnz, ctx().cus);
    if (nwg < 1 || nwg > 1024) { *status = R2P_ABORTED; return 0; }
    // TEST HOOK: behave as if the kernel's workgroups had not all become resident (the caller must then finish the run on the
    // launch-per-kernel loop from the state solver.Init left)
    if (sw::r2p_test_abort()) { *status = R2P_ABORTED; return 0; }
    if (!s->r2p.sync) {
        int rc = s->own.dev(&s->r2p.hc1, (size_t)2 * s->n);
        rc |= s->own.dev(&s->r2p.r2c, (size_t)2 * s->m);
        rc |= s->own.dev(&s->r2p.part, (size_t)3 * 8 * 1024);                  // three arrays of [workgroups <= 1024][8]
        rc |= s->own.dev(&s->r2p.out, (size_t)16);
        rc |= s->own.pinned((void**)&s->r2p.pin, 16 * sizeof(double));
        rc |= s->own.dev((unsigned char**)&s->r2p.sync, rank2_persist_sync_bytes());           // last: its presence says the set is complete
        if (rc) return SMK_DEVICE_ERROR;
    }
    R2PersistArgs a;
    a.colptr = s->a->colptr; a.rowidx = s->a->rowidx; a.val = s->a->val;
    a.colptr_t = s->a->colptr_t; a.rowidx_t = s->a->rowidx_t; a.val_t = s->a->val_t;
    a.m = s->m; a.n = s->n;
    a.Gw0 = s->Gw; a.R1 = view1(s);
    a.Wc = s->Wc; a.Hc0 = s->Hc; a.Hc1 = s->r2p.hc1; a.R2c = s->r2p.r2c;
    a.gp_h = s->r2p.part; a.gp_w = s->r2p.part + 8 * 1024; a.pgp = s->r2p.part + 2 * 8 * 1024;
    a.sync = s->r2p.sync;
    a.min_iter = s->o.min_iter; a.max_iter = s->o.max_iter; a.tolcount = s->o.tolcount; a.tol = s->o.tol;
    a.iter_tag0 = s->iter;
    a.Wt = s->Wt; a.H = s->H; a.Gw = s->Gw;
    a.fail_flag = s->fail_flag;
    a.lds_bytes = (unsigned)rank2_persist_lds_bytes();
    a.out = s->r2p.out;
    int rc = launch_rank2_persist(a, nwg, s->st);
    if (rc == 1) { *status = R2P_ABORTED; return 0; }       // the grid does not fit the device as it is now
    if (rc) return rc;
    SMK_HIP(hipMemcpyAsync(s->r2p.pin, s->r2p.out, 16 * sizeof(double), hipMemcpyDeviceToHost, s->st));
    SMK_HIP(hipStreamSynchronize(s->st));
    *status = (int)s->r2p.pin[0];
    *count = (int)s->r2p.pin[1];
    {
        if (sw::r2p_profile()) {
            const double it = std::max(1.0, s->r2p.pin[2]);
            fprintf(stderr, "[r2p] %ld x %ld nnz %ld: %d workgroups, status %d, %.0f iterations; per iteration (workgroup 0): "
                    "B1 %.1f us, phase W %.1f, B2 %.1f, phase G %.1f\n", (long)s->m, (long)s->n, (long)s->a->nnz, nwg, *status, it,
                    s->r2p.pin[8] / it, s->r2p.pin[9] / it, s->r2p.pin[10] / it, s->r2p.pin[11] / it);
        }
    }
    if (*status == R2P_CONVERGED || *status == R2P_EXHAUSTED) {
        s->iter += (int)s->r2p.pin[2];
        s->pc.pg0 = s->r2p.pin[3];
        s->pc.last_metric = s->r2p.pin[4];
        s->pc.sums_state = 2;          // the launch returns no sums (smk_solver_progress_sums: SMK_UNSUPPORTED)
        s->normalized = false;
        s->inited = false;             // HH' and the stored products were never materialised: a later run starts from solver.Init
        s->wc_valid = false;
    }
    return 0;
}

static int solver_run_once(smk_solver* s, smk_stats* stats)
{
    if (!s) return SMK_BAD_PARAM;
    set_error("");                                  // smk_last_error() describes THIS run afterwards
    if (!s->have_factors) { set_error("set_factors() first"); return SMK_BAD_PARAM; }
    const smk_options& o = s->o;
    const double t0 = wall_us();
    int rc = 0, result = SMK_OK;
    bool success = false;
    int iter = 0, fail_iter = INT_MAX;
    static std::mutex r2p_device_mu[64];
    std::unique_lock<std::mutex> r2p_lock;

    if (!s->inited) { rc = solver_init(s); if (rc) { result = rc; goto done; } }

    // One resident kernel per device at a time: two of them launched together (two host threads with a context each on ONE
    // device, the two-device HierNMF2 test) would each get part of the CUs and wait for workgroups that cannot start.  The
    // second caller WAITS (it does not take the other path: which path runs must not depend on timing, the two differ in the
    // last bits and the tree search is discrete).  Contexts on different devices do not meet here.
    if (rank2_persist_eligible(s)) {
        const int dev = smk_current_device();
        r2p_lock = std::unique_lock<std::mutex>(r2p_device_mu[dev >= 0 && dev < 64 ? dev : 0]);
    }
    if (r2p_lock.owns_lock()) {
        int status = R2P_ABORTED, count = 0;
        rc = rank2_persist_run(s, &status, &count);
        r2p_lock.unlock();
        if (rc) { result = rc; goto done; }
        if (status == R2P_CONVERGED || status == R2P_EXHAUSTED) {
            success = true;
            iter = count;
            goto finish;
        }
        if (status == R2P_NAN) { set_error("ProjectedGradientNorm: NaN"); iter = count; result = SMK_FAILURE; goto done; }
        if (status == R2P_SOLVER_FAILED) { result = SMK_FAILURE; goto failed_check; }
        // ABORTED: some workgroup never became resident (or the deadline passed); the solver state is the one solver.Init
        // left, so the launch-per-kernel loop below takes over, latched for the life of the handle
        s->r2p.off = true;
        s->wc_valid = false;           // the compact copy of W served as the kernel's work array
        const unsigned long long bit = 1ull << (smk_current_device() & 63);
        if (!(g_r2p_off_devices.fetch_or(bit, std::memory_order_relaxed) & bit))       // once per device and process
            fprintf(stderr, "smallk_amd: the resident RANK2 kernel could not synchronise its workgroups on device %d; this process continues on the launch-per-kernel path there\n", smk_current_device());
    }

    // The stopping rule of iteration i (NmfSolve, nmf_solve_generic.hpp:81-121) is evaluated AFTER iteration i + 1 has been enqueued
    // and i is restored from its snapshot when it fires (check_ring.h); SMK_SYNC_PROGRESS=1 runs the check-every-iteration loop.
    {
        check_ring::Params p;
        p.depth = progress_depth(s);
        p.min_iter = o.min_iter;  p.max_iter = o.max_iter;  p.tol = o.tol;  p.tolcount = o.tolcount;
        p.sync = sw::sync_progress();
        p.verbose = o.verbose != 0;
        bool in_check = false;                   // the error came out of a check, not out of an iteration
        const check_ring::Result r = check_ring::drive(p,
            [s](int, int snap_slot) { return checked_iteration(s, snap_slot); },
            [s](int, int b, bool snapshot) { return progress_begin(s, b, snapshot); },
            [&](int i, int b, double* metric) { const int e = progress_end(s, b, i, metric); in_check |= e != 0; return e; },
            [&](int i, int b) { const int e = progress_restore(s, b); in_check |= e != 0; if (!e) s->iter = i + 1; return e; },
            [](const char* line) { fputs(line, stdout); });
        iter = r.iterations;
        success = r.converged;
        if (r.code) { result = r.code; if (in_check) goto failed_check; goto done; }
    }

finish:
    rc = gather_w(s);
    if (rc) { result = rc; goto done; }
    if (o.normalize) { rc = normalize_device(s); if (rc) { result = rc; goto done; } }
    if (is_dist(s)) { rc = dist_agree(s); if (rc) { result = rc; goto done; } }
    rc = sync_and_check(s, &fail_iter);
    if (rc) { result = rc; goto failed_check; }
    if (!success && iter == o.max_iter) success = true;
    result = success ? SMK_OK : SMK_FAILURE;
    goto done;

failed_check:
    if (result == SMK_FAILURE) {
        // which iteration set the device flag (BPP pivot limit / non-SPD / zero column norm)
        int flag = INT_MAX;
        (void)hipMemcpy(&flag, s->fail_flag, sizeof(int), hipMemcpyDeviceToHost);
        if (flag != INT_MAX && flag >= 0) {
            iter = flag;
            fprintf(stderr, "\tNMF solver failure on iteration %d\n", iter + 1);
        }
    }
done:
    if (stats) {
        stats->elapsed_us = (unsigned long long)(wall_us() - t0);
        stats->iteration_count = iter;
    }
    return result;
}

// NnlsHals (common/include/nnls.hpp:249-316): W stays fixed, H is swept with the HALS row update until
// the projected-gradient norm of H drops below tol * (its value after the first sweep).  W'A is
// formed once by the streaming product, every iteration is two column-tile kernels over H.
// Returns SMK_OK on convergence (W, H then normalised like the reference does) or SMK_FAILURE when
// the iteration limit is reached.
int smk_solver_nnls_hals(smk_solver* s, double tol, int verbose, int max_iter, int* iterations)
{
    if (!s || max_iter < 0) return SMK_BAD_PARAM;
    if (!s->have_factors) { set_error("set_factors() first"); return SMK_BAD_PARAM; }
    if (is_dist(s)) { set_error("NnlsHals: not available on a sharded solver"); return SMK_UNSUPPORTED; }
    if (verbose) printf("\nRunning NNLS solver...\n");
    int rc = 0;
    // W'A is formed ONCE and every sweep of the loop below reads it: the accurate product form (the fp64 product of the stored
    // data) for the price of one slower pass, so that the converged H differs from the reference's by summation order only
    if (!s->a->sparse && s->nsplit != NSPLIT_F64 && !sw::nsplit().set) {
        s->nsplit = NSPLIT_F64;
        rc = plan_products(s);
        if (!rc && alloc_product_buffers(s)) rc = SMK_DEVICE_ERROR;
        if (rc) return rc;
    }
    rc = gram_w(s);
    if (!rc) rc = prod1(s);
    if (rc) return rc;
    bool success = false;
    double pg0 = 0.0;
    int i = 0;
    for (i = 0; i < max_iter; ++i) {
        rc = launch_hals_sweep(s->H, s->k, s->n, view1(s), s->Gw, s->st);
        if (!rc) rc = launch_grad_pg(s->H, s->k, s->n, view1(s), s->Gw, nullptr, s->pg_partials + s->pg_half, s->scal, 1, s->st, s->wide_tmp);
        if (rc) return rc;
        double sum = 0.0;
        SMK_HIP(hipMemcpyAsync(&sum, s->scal + 1, sizeof(double), hipMemcpyDeviceToHost, s->st));
        SMK_HIP(hipStreamSynchronize(s->st));
        const double pg = std::sqrt(sum);
        if (std::isnan(pg)) { set_error("ProjectedGradientNorm: NaN"); return SMK_FAILURE; }
        if (i == 0) {
            pg0 = pg;
            if (verbose) printf("1:\tprogress metric:\t%g\n", 1.0);
            continue;
        }
        if (verbose && ((i + 1 < 10) || ((i + 1) % 10 == 0))) printf("%d:\tprogress metric:\t%g\n", i + 1, pg / pg0);
        if (pg < tol * pg0) {
            success = true;
            s->normalized = false;
            rc = normalize_device(s);
            if (rc) return rc;
            break;
        }
    }
    if (iterations) *iterations = success ? i + 1 : i;
    s->inited = false;       // Gw/R1 no longer describe a solver schedule
    rc = sync_and_check(s, nullptr);
    if (rc) return rc;
    if (!success) fprintf(stderr, "NNLS solver reached iteration limit.\n");
    return success ? SMK_OK : SMK_FAILURE;
}

// The fold-in ("transform") step of a trained model: H = argmin_{H >= 0} ||A - W H||_F with the solver's W fixed, by ONE exact
// block-pivoting solve of (W'W) H = W'A from the current H as the warm start (passive set = H > 0).  W is not touched, nothing is
// normalised, the iteration count stays.  SMK_FAILURE = the reference's `false` (a rank-deficient W).
int smk_solver_project_h(smk_solver* s)
{
    if (!s) { set_error("smk_solver_project_h: null solver"); return SMK_BAD_PARAM; }
    if (!s->have_factors) { set_error("smk_solver_project_h: set_factors() first"); return SMK_BAD_PARAM; }
    if (s->o.algorithm != SMK_ALG_BPP) { set_error("smk_solver_project_h: a BPP solver"); return SMK_BAD_PARAM; }
    if (is_dist(s) || s->ex.w_sharded) { set_error("smk_solver_project_h: not available on a sharded solver"); return SMK_UNSUPPORTED; }
    int rc = 0;
    // one pass: the accurate product form (the fp64 product of the stored data) costs one slower pass, and H then differs from the
    // reference's by summation order only (as smk_solver_nnls_hals)
    if (!s->a->sparse && s->nsplit != NSPLIT_F64 && !sw::nsplit().set) {
        s->nsplit = NSPLIT_F64;
        rc = plan_products(s);
        if (!rc && alloc_product_buffers(s)) rc = SMK_DEVICE_ERROR;
        if (rc) return rc;
    }
    // as solver.Init: the factors are the caller's, nothing is known to come from an NNLS launch, nothing is pending
    s->forget_handoffs();
    s->pc.reset();
    s->normalized = false;          // H is about to change
    rc = gram_w(s);
    if (!rc) rc = prod1(s);
    if (!rc) rc = nnls_side(s, 0, s->H, 0, s->n, view1(s), s->Gw);
    s->inited = false;              // Gw / R1 no longer describe a solver schedule
    s->forget_handoffs();           // (what the solve left is for a schedule that does not follow)
    if (rc) return rc;
    return sync_and_check(s, nullptr);
}

int smk_debug_nnls_stats(unsigned long long* out256, int reset)
{
    if (!ctx().init) return SMK_NOTINITIALIZED;
    const int rc = nnls_stats_read(out256, reset);
    return rc == 0 ? SMK_OK : rc == -1 ? SMK_UNSUPPORTED : SMK_DEVICE_ERROR;
}

}  // extern "C"
