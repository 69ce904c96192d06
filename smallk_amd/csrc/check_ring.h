// smallk_amd/csrc/check_ring.h -- the schedule of the stopping-rule check, host-only: which iteration is checked in which slot, when
// a check is read, when a snapshot is promised and what is restored.  Nothing here knows a solver or HIP: smk_solver_run and
// smk_solver_iterate_checked (solver.cpp) pass their operations in, tests/check_ring/ring_sim.cpp passes scripted ones.
// The rule is NmfSolve<>'s (common/include/nmf_solve_generic.hpp:67-139): iteration 0 is checked to initialise the estimator,
// iterations in (0, min_iter) are not, from min_iter on every iteration is, and `tolcount` successive metrics <= tol end the run.
// It is evaluated LATE: up to `depth` further iterations are enqueued before the host reads a check, so the device never waits for
// a scalar.  A check from min_iter on keeps a snapshot of its iteration; when the rule fires at p and something ran after p, p is
// restored: results and iteration counts are those of the check-every-iteration loop.
#pragma once
#include <cstdio>

namespace smk {
namespace check_ring {

static const int MAX_DEPTH = 3;        // checks in flight; a per-slot array holds MAX_DEPTH + 1 entries

struct Params {
    int depth = 1;                     // checks in flight, 1 .. MAX_DEPTH (one: the host enqueues i + 1, then reads the check of i)
    int min_iter = 0, max_iter = 0, tolcount = 1;
    double tol = 0.0;
    bool sync = false;                 // every check is read before the next iteration is enqueued: no snapshot, nothing to restore
    bool verbose = false;
    bool every = false;                // every iteration checked with a snapshot, the rule never fires (smk_solver_iterate_checked) ...
    int base = 0;                      // ... and the operations see iteration numbers offset by this
    int slots() const { return depth + 1; }
    int slot(int i) const { return i % (depth + 1); }      // depth 1: i & 1
};

// code != 0: an operation failed, nothing was started after it, `iterations` is the iteration it belonged to.  Otherwise the
// iteration the rule fired at (converged) or max_iter.  metric: of the last check read.
struct Result { int code = 0, iterations = 0; bool converged = false; double metric = 1.0; };

// step(i, snap): run iteration i; snap >= 0: its check will want a snapshot in that slot, the iteration may write it itself.
// begin(i, slot, snapshot) / end(i, slot, &metric): enqueue the check of iteration i / wait for it.  restore(i, slot): make
// iteration i the current state again.  report(line): verbose output.  All but report return 0 or an error code.
template <class Step, class Begin, class End, class Restore, class Report>
Result drive(const Params& p, Step step, Begin begin, End end, Restore restore, Report report)
{
    Result r;
    int pend[MAX_DEPTH + 1], npend = 0, enqueued = 0, success_count = 0;      // outstanding checks, oldest first
    char line[96];
    auto resolve = [&]() -> int {      // reads the oldest outstanding check and applies the rule: 0 go on, 1 converged, -1 error
        const int i = r.iterations = pend[0];
        for (int j = 1; j < npend; ++j) pend[j - 1] = pend[j];
        --npend;
        if ((r.code = end(p.base + i, p.slot(i), &r.metric)) != 0) return -1;
        if (p.every || i < p.min_iter) return 0;           // iteration 0 only initialises the estimator
        if (p.verbose && (i + 1 < 10 || (i + 1) % 10 == 0)) {
            snprintf(line, sizeof line, "%d:\tprogress metric:\t%g\n", i + 1, r.metric);      // nmf_progress_estimation.hpp:22-33
            report(line);
        }
        if (!(r.metric <= p.tol)) { success_count = 0; return 0; }
        if (++success_count < p.tolcount) return 0;
        if (p.verbose) {
            snprintf(line, sizeof line, "\nSolution converged after %d iterations.\n\n", i + 1);
            report(line);
        }
        if (i + 1 < enqueued && (r.code = restore(p.base + i, p.slot(i))) != 0) return -1;
        r.converged = true;
        return 1;
    };
    for (int i = 0; i < p.max_iter; ++i) {
        const bool check = p.every || i == 0 || i >= p.min_iter;
        const bool snapshot = p.every || (!p.sync && i >= p.min_iter);
        r.iterations = i;
        if ((r.code = step(p.base + i, snapshot ? p.slot(i) : -1)) != 0) return r;
        ++enqueued;
        if (check) {
            if ((r.code = begin(p.base + i, p.slot(i), snapshot)) != 0) return r;
            pend[npend++] = i;
        }
        // at most `depth` checks stay in flight behind this iteration (none in synchronous mode); an unchecked iteration
        // (0 < i < min_iter) leaves nothing behind
        const int keep = (check && !p.sync) ? p.depth : 0;
        while (npend > keep)
            if (resolve()) return r;
        if (p.verbose && !p.every && i < p.min_iter) {
            snprintf(line, sizeof line, "%d:\tprogress metric: \t(min_iter)\n", i + 1);
            report(line);
        }
    }
    while (npend > 0)                  // what is still outstanding when the iterations are used up
        if (resolve()) return r;
    r.iterations = p.max_iter;
    return r;
}

}  // namespace check_ring
}  // namespace smk
