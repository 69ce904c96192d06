// smallk_amd/csrc/progress.cpp -- the stopping rule's check (progress_est->Update of the reference): forming the metric, and the
// same evaluation one iteration late -- begin / end / restore of one slot of the ring whose schedule is check_ring.h.  Its state
// is the solver's ProgressCheck (state.h); solver.cpp keeps the three places where a check rides in other launches (the riders of
// nnls_side, the tail of prod2, the snapshot slot handed to a checked iteration).
#include "solver_internal.h"
#include "check_ring.h"

#include <algorithm>
#include <atomic>
#include <climits>
#include <cmath>
#include <string>

namespace smk {

static_assert(check_ring::MAX_DEPTH + 1 == ProgressCheck::PROG_SLOTS, "one slot per check in flight and one for the iteration being enqueued");

// Latency-bound BPP (C2; DESIGN.md 6, "Checked iterations"): gradH_i = W_i'W_i H_i - W_i'A is formed from the system matrix, the
// warm start and the right-hand side of iteration i + 1's H-side NNLS launch (gradW is the W-side NNLS's dual: sum exactly 0).
// So that launch forms the sum on its way in (NnlsRiders::pg_part), both NNLS launches of an iteration store their result a second
// time into the snapshot slot (NnlsRiders::snap_x), and a check costs ONE small launch, the totals.  When no further iteration
// follows, progress_end forms the check the old way.  SMK_PROGRESS_DEFER=0: off.
bool check_rides_in_nnls(const smk_solver* s)
{
    if (!sw::progress_defer() || !sw::progress_fused() || sw::bpp_gradw() || sw::guard_every() > 0) return false;
    if (s->o.algorithm != SMK_ALG_BPP || s->KP > 16 || s->o.prog_est_algorithm != SMK_PROG_PG_RATIO) return false;
    if (is_dist(s) || s->ex.comm || s->ex.w_sharded) return false;
    const i64 gpb = 256 / s->KP;
    return (s->n + gpb - 1) / gpb <= (i64)s->pg_half;          // one partial per workgroup of the H-side launch
}

// A solver with a native communicator allocates nothing once its collectives are in flight (several ranks may live in one process):
// smk_solver_attach_comm makes what a checked iteration needs (progress_prealloc: `attaching`), an object missing later is an error.
// Every other solver allocates on first use.
static int missing_behind_comm(const char* what, int b)
{
    set_error(std::string("progress check: ") + what + " of slot " + std::to_string(b) + " was not allocated when the communicator was attached");
    return SMK_FAILURE;
}
// the snapshot (W, H, W'W) of progress slot b
int ensure_snapshot(smk_solver* s, int b, bool attaching)
{
    if (s->pc.snap[b]) return 0;
    if (s->ex.comm && !attaching) return missing_behind_comm("the snapshot", b);
    return s->own.dev(&s->pc.snap[b], snapshot_elems(s->k, s->m, s->n));
}
// the pinned result slots and their events
static int ensure_progress_slots(smk_solver* s, int b, bool attaching = false)
{
    if (s->pc.pin) return 0;
    if (s->ex.comm && !attaching) return missing_behind_comm("the pinned result", b);
    int rc = s->own.pinned((void**)&s->pc.pin, ProgressCheck::PROG_SLOTS * sizeof(ProgressCheck::ProgSlot));
    for (int i = 0; i < ProgressCheck::PROG_SLOTS && !rc; ++i) rc = s->own.event(&s->pc.pev[i], hipEventDisableTiming);
    return rc;
}

// The totals of a deferred progress check (nnls_side left the per-workgroup sums): W'W of the checked iteration is still in place
// until the W-side solve of this iteration has run, so they may be formed anywhere in front of it.  pl != nullptr and the pass
// carries a tail already: one more tail workgroup forms them (the caller records the slot's event behind the pass: returns 1);
// otherwise a launch of their own, now.  SMK_PROGRESS_TAIL=0: always the launch.
// The result is awaited by polling its pinned slot (the kernel stores a tag behind the totals, system scope) instead of an event:
// an event record between two launches costs 3 - 4 us of idle stream.  SMK_PROGRESS_POLL=0: the event.
int check_totals(smk_solver* s, BigProdPlan* pl)
{
    ProgressCheck& pc = s->pc;
    if (pc.pg_totals_slot < 0) return 0;
    const bool ride = sw::progress_tail();
    const bool poll = sw::progress_poll();
    const int b = pc.pg_totals_slot, k2 = (s->k + 1) / 2 * 2;
    double* snap_g = pc.pg_defer_snap ? pc.snap[b] + (size_t)(s->m + s->n) * k2 : nullptr;
    const double* part = s->pg_partials + s->pg_half;
    const double tag = poll ? (double)(pc.pg_defer_tag + 2) : 0.0;
    pc.poll_tag[b] = tag;
    if (ride && pl && pl->tail_nblk > 0) {
        BigProdPlan::TailCheck& tc = pl->tail_check;
        tc.part = part;  tc.n = pc.pg_defer_nblk;  tc.flag_slot = 5;  tc.tag_limit = pc.pg_defer_tag;  tc.kk = s->KP * s->KP;
        tc.out = s->scal;  tc.host_out = pc.pin[b].h;  tc.flag = s->fail_flag;  tc.G = s->Gw;  tc.snap_g = snap_g;  tc.tag = tag;
        ++pc.check_routes[3];
        return 1;
    }
    pc.pg_totals_slot = -1;
    ++pc.check_routes[2];
    const int rc = launch_pg_defer_sum(part, pc.pg_defer_nblk, s->scal, pc.pin[b].h, s->fail_flag, 5, pc.pg_defer_tag, s->Gw, snap_g,
                                       s->KP * s->KP, s->st, tag);
    if (rc) return rc;
    if (tag == 0.0) SMK_HIP(hipEventRecord(pc.pev[b], s->st));
    return 0;
}

// the kernels (and, sharded, the scalar all-reduce) of one progress evaluation; results land in s->scal
static int enqueue_progress_kernels(smk_solver* s)
{
    int rc = wait_r2(s);
    if (rc) return rc;
    if (s->o.prog_est_algorithm == SMK_PROG_DELTA_FNORM) {
        rc = gather_w(s);             // a row-sharded W: the norm runs over all of it (BPP's default rule is PG_RATIO)
        if (rc) return rc;
        rc = launch_delta_fnorm(s->Wt, s->Wprev, (i64)s->KP * s->m, s->pg_partials, s->scal + 2, s->st);
        if (rc) return rc;
    } else {
        // gradW = W*HHt - AHt  (slot 0, replicated), gradH = WtW*H - WtA (slot 1, local shard)
        if (s->ex.w_sharded) {           // only this rank's rows of the summed (AH')' exist here: partial sum, joined in dist_agree
            rc = s->ex.n_own > 0 ? launch_grad_pg(s->ex.Wown, s->k, s->ex.n_own, view_own(s), s->Gh, nullptr, s->pg_partials, s->scal, 0, s->st, s->wide_tmp)
                              : launch_zero_f64(s->scal, 1, s->st);
        } else {
            rc = launch_grad_pg(s->Wt, s->k, s->m, view2(s), s->Gh, nullptr, s->pg_partials, s->scal, 0, s->st, s->wide_tmp);
        }
        if (rc) return rc;
        rc = launch_grad_pg(s->H, s->k, s->n, view1(s), s->Gw, nullptr, s->pg_partials + s->pg_half, s->scal, 1, s->st, s->wide_tmp);
        if (rc) return rc;
    }
    if (is_dist(s)) { rc = dist_agree(s); if (rc) return rc; }
    return 0;
}

// metric from the four scalars (PG sums for W and H, delta-Fnorm numerator / denominator)
static int evaluate_progress(smk_solver* s, const double* h, int iter_index, double* metric)
{
    ProgressCheck& pc = s->pc;
    if (s->o.prog_est_algorithm == SMK_PROG_DELTA_FNORM) {
        *metric = std::sqrt(h[2]) / std::sqrt(h[3]);
        pc.sums[0] = pc.sums[1] = 0.0;  pc.sums[2] = h[2];  pc.sums[3] = h[3];
    } else {
        const double pg = std::sqrt(h[0] + h[1]);
        if (std::isnan(pg)) { set_error("ProjectedGradientNorm: NaN"); return SMK_FAILURE; }   // reference throws
        if (iter_index == 0) { s->pc.pg0 = pg; *metric = 1.0; }
        else *metric = pg / s->pc.pg0;
        pc.sums[0] = h[0];  pc.sums[1] = h[1];  pc.sums[2] = pc.sums[3] = 0.0;
    }
    pc.sums_state = 1;
    s->pc.last_metric = *metric;
    return SMK_OK;
}

// progress_est->Update(iter, W, H, gradW, gradH): returns the metric (synchronises)
int update_progress(smk_solver* s, int iter_index, double* metric)
{
    int rc = enqueue_progress_kernels(s);
    if (rc) return rc;
    double h[4] = {0, 0, 0, 0};
    SMK_HIP(hipMemcpyAsync(h, s->scal, 4 * sizeof(double), hipMemcpyDeviceToHost, s->st));
    int fail_iter = INT_MAX;
    rc = sync_and_check(s, &fail_iter);
    if (rc) return rc;
    return evaluate_progress(s, h, iter_index, metric);
}

// ---- the same evaluation, one iteration late ------------------------------------------------
// How many progress checks may be in flight.  ONE is the default, as in rounds 1 - 5: the host enqueues iteration i + 1, then waits
// for check i.  Round 6 measured two and three in flight on C2: 10 980 / 11 100 it/s against 11 010 (profiles/r06_progress_check.txt)
// -- the host is not the limit, the gradient pass is.  SMK_PROGRESS_DEPTH=2|3 keeps the deeper ring selectable; sharded runs always
// use one (their checks carry collectives), and so does a run whose snapshot exceeds 1 GiB.
int progress_depth(const smk_solver* s)
{
    const int forced = sw::progress_depth();
    if (is_dist(s) || s->ex.comm || forced <= 1) return 1;
    if (snapshot_elems(s->k, s->m, s->n) * sizeof(double) > ((size_t)1 << 30)) return 1;
    return std::min(forced, check_ring::MAX_DEPTH);
}

// smk_solver_attach_comm: everything a checked iteration of a sharded run needs, before the collectives start -- the pinned block,
// the events and one snapshot per slot of its ring (ONE check in flight: two slots)
int progress_prealloc(smk_solver* s)
{
    check_ring::Params ring;
    ring.depth = progress_depth(s);
    int rc = ensure_progress_slots(s, 0, true);
    for (int b = 0; b < ring.slots() && !rc; ++b) rc = ensure_snapshot(s, b, true);
    return rc;
}

// Enqueue the progress kernels of the iteration that has just been enqueued, copy their scalars and
// the failure flag into pinned slot `b` and record an event; when `snapshot` is set also keep
// (W, H, W'W) of this iteration so that the NEXT, speculatively enqueued iteration can be undone.
int progress_begin(smk_solver* s, int b, bool snapshot, bool allow_defer)
{
    ProgressCheck& pc = s->pc;
    const bool promised = pc.iter_snap_slot == b;       // this iteration's NNLS launches have been writing the snapshot of slot b
    pc.iter_snap_slot = -1;                             // (the hand-over of solver.cpp's checked_iteration ends here)
    int rc = ensure_progress_slots(s, b);
    if (!rc) rc = wait_r2(s);
    if (rc) return rc;
    pc.poll_tag[b] = 0.0;
    pc.pin[b].h[7] = 0.0;
    // deferred (check_rides_in_nnls): nothing is enqueued now -- the next H-side NNLS launch forms the sum; a snapshot can be
    // promised only if this iteration's NNLS launches have been writing it
    if (allow_defer && pc.pg_defer_slot < 0 && (!snapshot || promised) && check_rides_in_nnls(s)) {
        pc.pg_defer_slot = b;
        pc.pg_defer_snap = snapshot;
        pc.pg_defer_tag = s->iter - 1;              // the iteration just enqueued
        pc.pin[b].fused = 1;
        return 0;
    }
    ++pc.check_routes[1];
    if (s->o.algorithm == SMK_ALG_RANK2 && s->o.prog_est_algorithm == SMK_PROG_PG_RATIO && !is_dist(s)) {
        // one launch: both gradient sums, the failure flag and the snapshot (rank2.hip)
        if (snapshot) { rc = ensure_snapshot(s, b); if (rc) return rc; }
        const size_t pe = rank2_progress_scratch_elems(s->m, s->n);
        if (!pc.pin_r2[b] && s->own.pinned((void**)&pc.pin_r2[b], pe * sizeof(double))) return SMK_DEVICE_ERROR;
        rc = launch_rank2_progress(s->Wt, s->m, view2(s), s->Gh, s->H, s->n, view1(s), s->Gw, s->r2_prog, s->fail_flag,
                                   snapshot ? pc.snap[b] : nullptr, s->st);
        if (rc) return rc;
        pc.pin[b].fused = 2;             // per-workgroup partials: progress_end adds them up in index order
        SMK_HIP(hipMemcpyAsync(pc.pin_r2[b], s->r2_prog, pe * sizeof(double), hipMemcpyDeviceToHost, s->st));
        SMK_HIP(hipEventRecord(pc.pev[b], s->st));
        return 0;
    }
    const bool fused_check = sw::progress_fused();
    // BPP: gradW is the dual of the W-side NNLS (nmf_solver_bpp.hpp:362-366), whose projected-gradient sum is exactly zero after a
    // solve that reached optimality (a solve that did not has raised the failure flag); SMK_BPP_GRADW=1 forms HH' W' - (AH')' anyway
    const bool bpp_dual_is_gradient = !sw::bpp_gradw();
    if (fused_check && s->o.prog_est_algorithm == SMK_PROG_PG_RATIO && !is_dist(s) && !is_wide(s->k) && !s->ex.w_sharded) {
        // round 6: gradients + snapshot in one launch, sums + failure flag written into the pinned slot by a second (kernels.hip:
        // grad_pg2_snap_kernel, sum_partials2_host_kernel); SMK_PROGRESS_FUSED=0: the four stream operations of before
        if (snapshot) { rc = ensure_snapshot(s, b); if (rc) return rc; }
        const double tag = sw::progress_poll() ? (double)(s->iter + 1) : 0.0;
        rc = launch_grad_pg2_fused(s->Wt, s->m, view2(s), s->Gh, s->pg_partials, s->H, s->n, view1(s), s->Gw, s->pg_partials + s->pg_half,
                                   s->k, s->scal, s->fail_flag, 5, snapshot ? pc.snap[b] : nullptr, pc.pin[b].h, s->st,
                                   (s->o.algorithm == SMK_ALG_BPP && bpp_dual_is_gradient) ? 1 : 0, tag);
        if (rc) return rc;
        pc.pin[b].fused = 1;
        pc.poll_tag[b] = tag;
        if (tag == 0.0) SMK_HIP(hipEventRecord(pc.pev[b], s->st));
        return 0;
    }
    if (s->o.prog_est_algorithm == SMK_PROG_PG_RATIO && !is_dist(s) && !is_wide(s->k)) {
        // both gradients in one launch, both sums + the failure flag in a second, one 64-byte read-back
        rc = launch_grad_pg2(s->Wt, s->m, view2(s), s->Gh, s->pg_partials, s->H, s->n, view1(s), s->Gw,
                             s->pg_partials + s->pg_half, s->k, s->scal, s->fail_flag, 5, s->st,
                             (s->o.algorithm == SMK_ALG_BPP && bpp_dual_is_gradient) ? 1 : 0);      // as the fused route: W's sum is exactly 0
        if (rc) return rc;
        pc.pin[b].fused = 1;
        SMK_HIP(hipMemcpyAsync(pc.pin[b].h, s->scal, 8 * sizeof(double), hipMemcpyDeviceToHost, s->st));
    } else {
        rc = enqueue_progress_kernels(s);
        if (rc) return rc;
        pc.pin[b].fused = 0;
        SMK_HIP(hipMemcpyAsync(pc.pin[b].h, s->scal, 4 * sizeof(double), hipMemcpyDeviceToHost, s->st));
        SMK_HIP(hipMemcpyAsync(&pc.pin[b].flag, s->fail_flag, sizeof(int), hipMemcpyDeviceToHost, s->st));
    }
    if (snapshot) {
        rc = ensure_snapshot(s, b); if (rc) return rc;
        rc = s->ex.w_sharded ? launch_snapshot(s->ex.Wown, s->ex.n_own, s->H, s->n, s->Gw, pc.snap[b], s->k, 1, s->st)
                          : launch_snapshot(s->Wt, s->m, s->H, s->n, s->Gw, pc.snap[b], s->k, 1, s->st);
        if (rc) return rc;
    }
    SMK_HIP(hipEventRecord(pc.pev[b], s->st));
    return 0;
}

// wait for slot b; SMK_FAILURE when the device flagged a solver failure up to that iteration
int progress_end(smk_solver* s, int b, int iter_index, double* metric)
{
    ProgressCheck& pc = s->pc;
    if (pc.pg_defer_slot == b) {                    // no further iteration was enqueued: the check is formed the direct way now
        pc.pg_defer_slot = -1;
        const int frc = progress_begin(s, b, false, false);
        if (frc) return frc;
    }
    if (pc.poll_tag[b] != 0.0) {
        // the kernel that forms the totals stores the tag behind them (system scope); the stream going idle without it is an error
        const volatile double* tagp = &pc.pin[b].h[7];
        const double want = pc.poll_tag[b];
        for (unsigned long spins = 1; *tagp != want; ++spins) {
#if defined(__x86_64__) || defined(__i386__)
            __builtin_ia32_pause();
#endif
            if ((spins & 0x3FFFF) == 0) {
                const hipError_t q = hipStreamQuery(s->st);
                if (q == hipErrorNotReady) continue;
                if (q == hipSuccess && *tagp == want) break;
                set_error(q == hipSuccess ? "the progress check's result never arrived in its pinned slot" : hipGetErrorString(q));
                return q == hipSuccess ? SMK_FAILURE : SMK_DEVICE_ERROR;
            }
        }
        std::atomic_thread_fence(std::memory_order_acquire);
        pc.poll_tag[b] = 0.0;
    } else {
        SMK_HIP(hipEventSynchronize(pc.pev[b]));
    }
    if (pc.pin[b].fused == 2) {
        const int nb = rank2_progress_blocks(s->m, s->n);
        const double* p = pc.pin_r2[b];
        double sw = 0.0, sh = 0.0;
        for (int i = 0; i < nb; ++i) { sw += p[2 * i]; sh += p[2 * i + 1]; }
        pc.pin[b].h[0] = sw;
        pc.pin[b].h[1] = sh;
        pc.pin[b].flag = (int)p[2 * (size_t)nb];
    } else if (pc.pin[b].fused) pc.pin[b].flag = (int)pc.pin[b].h[5];
    if (pc.pin[b].flag != INT_MAX) return SMK_FAILURE;
    return evaluate_progress(s, pc.pin[b].h, iter_index, metric);
}

int progress_restore(smk_solver* s, int b)
{
    int rc = s->ex.w_sharded ? launch_snapshot(s->ex.Wown, s->ex.n_own, s->H, s->n, s->Gw, s->pc.snap[b], s->k, 0, s->st)
                          : launch_snapshot(s->Wt, s->m, s->H, s->n, s->Gw, s->pc.snap[b], s->k, 0, s->st);
    if (rc) return rc;
    // whatever the undone iteration did to the failure flag is void; products / HH' are stale
    const int big = INT_MAX;
    SMK_HIP(hipMemcpyAsync(s->fail_flag, &big, sizeof(int), hipMemcpyHostToDevice, s->st));
    SMK_HIP(hipStreamSynchronize(s->st));
    s->inited = false;
    s->wc_valid = false;
    if (s->ex.w_sharded) s->ex.w_full = false;    // the snapshot holds this rank's own rows; the full copy is stale
    return 0;
}

}  // namespace smk
