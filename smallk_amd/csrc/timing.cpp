// smallk_amd/csrc/timing.cpp -- what a caller reads about a solver's passes: smk_solver_enable_timing, the sampled event times
// (smk_solver_kernel_time), which kernel a pass launches (smk_solver_kernel_name) and what it moves (smk_solver_kernel_work).  Its
// state is the solver's Timing (state.h); solver.cpp opens the spans on the per-iteration path (begin_pass, span_open) and reads them
// back through resolve_events whenever it has synchronised the stream.
#include "solver_internal.h"

#include <algorithm>
#include <cmath>
#include <cstdio>
#include <string>

namespace smk {

int resolve_events(smk_solver* s)
{
    Timing& t = s->timing;
    for (int w = 0; w < 6; ++w) {
        for (auto& e : t.ev[w]) {
            float ms = 0.f;
            SMK_HIP(hipEventElapsedTime(&ms, e.e0, e.e1));
            t.acc_ms[w] += (double)ms;                                // sampled totals; smk_solver_kernel_time scales them by passes seen / passes sampled
            t.launches[w] += e.counts;
        }
        t.span_pool.insert(t.span_pool.end(), t.ev[w].begin(), t.ev[w].end());      // read: span_open hands them out again
        t.ev[w].clear();
    }
    return 0;
}

}  // namespace smk

extern "C" {

int smk_solver_enable_timing(smk_solver* s, int on)
{
    if (!s) return SMK_BAD_PARAM;
    Timing& t = s->timing;
    t.on = on != 0;
    // one pass in 16 under 1 GB of streamed matrix per pass, one in 8 under 32 GB (a C4 shard in chunks: 8 launches and 8
    // collectives per iteration would carry ~0.1 ms of event gaps in 3.4 ms), every pass above
    {
        const double bytes = (double)s->m * (double)s->n * (s->a->sparse ? 12.0 : (double)elem_size(s->a->storage));
        t.stride = bytes < (double)((i64)1 << 30) ? 16 : bytes < 32.0 * (double)((i64)1 << 30) ? 8 : 1;
    }
    if (const auto ts = sw::timing_stride(); ts.set) t.stride = std::max(1, ts.v);
    t.pass_counter[0] = t.pass_counter[1] = 0;
    t.pass_sampled[0] = t.pass_sampled[1] = 0;
    for (int w = 0; w < 6; ++w) { t.acc_ms[w] = 0.0; t.launches[w] = 0; }
    return SMK_OK;
}

int smk_solver_kernel_time(smk_solver* s, int which, double* total_ms, int* launches)
{
    if (!s || which < 0 || which > 5) return SMK_BAD_PARAM;      // 2: the (AH')' sum and the W all-gather of a sharded run; 3: main-stream waits for them; 5: block pivoting
    const Timing& t = s->timing;
    if (which == 4) {       // calibration brackets: unscaled (their average is what matters)
        if (total_ms) *total_ms = t.acc_ms[4];
        if (launches) *launches = t.launches[4];
        return SMK_OK;
    }
    // one pass in `stride` carries events: totals are scaled by the TRUE ratio passes seen / passes sampled (100 passes
    // at stride 8 are 13 samples standing for 100, not for 104); the collectives (slot 2) are sampled with either pass
    const unsigned seen = which < 2 ? t.pass_counter[which] : t.pass_counter[0] + t.pass_counter[1];
    const unsigned sampled = which < 2 ? t.pass_sampled[which] : t.pass_sampled[0] + t.pass_sampled[1];
    const double f = sampled > 0 ? (double)seen / (double)sampled : 1.0;
    if (total_ms) *total_ms = t.acc_ms[which] * f;
    if (launches) *launches = (int)llround((double)t.launches[which] * f);
    return SMK_OK;
}

// the kernel pass `which` launches (what the bench lines and profiles attribute their time to); same decision as timed_spmm
// (solver.cpp) / launch_bigprod
int smk_solver_kernel_name(const smk_solver* s, int which, char* out, int cap)
{
    if (!s || which < 0 || which > 2 || !out || cap < 8) return SMK_BAD_PARAM;
    std::string name;
    if (which == 2) {
        static const char* const route[4] = {"", "launches of its own behind the iteration",
                                             "sums in the next H-side NNLS launch, totals as one launch",
                                             "sums in the next H-side NNLS launch, totals in the tail of the pass behind it"};
        for (int r = 3; r >= 1; --r)
            if (s->pc.check_routes[r]) name += (name.empty() ? "" : "; ") + std::to_string(s->pc.check_routes[r]) + " x " + route[r];
        if (name.empty()) name = "none formed yet";
    } else if (s->a->sparse) {
        const int ldx = s->Wc ? 2 : s->KP;
        if (s->r2p.sync && s->o.algorithm == SMK_ALG_RANK2) name = "smk::rank2_persist_kernel";
        else if (blocked2_route(s, which, ldx)) name = "smk::spmm_blocked2_kernel";
        else if (seg_route(s, which, ldx, which == 0 ? s->n : s->m)) name = "smk::spmm_seg_kernel";
        else name = "smk::spmm_gather_kernel";
    } else {
        const BigProdPlan& pl = which == 0 ? s->pl1 : s->pl2;
        name = s->nsplit == NSPLIT_F64 ? (s->k <= 2 ? "smk::bigprod_f64_k2_kernel" : "smk::bigprod_f64_kernel")
             : s->a->storage == SMK_STORE_F32 ? "smk::bigprod_f3_kernel" : "smk::bigprod_kernel";
        name += " variant " + std::to_string(pl.variant) + (pl.tr ? " (transposed source)" : "");
    }
    snprintf(out, (size_t)cap, "%s", name.c_str());
    return SMK_OK;
}

int smk_solver_kernel_work(const smk_solver* s, int which, double* bytes, double* flops)
{
    if (!s || which < 0 || which > 1) return SMK_BAD_PARAM;
    if (s->a->sparse) {   // per nonzero: 12 bytes of A (value + row index) + one KP-row of X gathered
        if (bytes) *bytes = (double)s->a->nnz * (12.0 + 8.0 * (s->Wc ? 2 : s->KP));      // RANK2 gathers 16 B rows of the compact copy
        if (flops) *flops = 2.0 * (double)s->a->nnz * s->k;
        return SMK_OK;
    }
    const double mn = (double)s->m * (double)s->n;
    if (bytes) *bytes = mn * elem_size(s->a->storage);
    if (flops) *flops = 2.0 * mn * s->k / s->ng;      // per launch: k > 64 streams the matrix once per group of 64 rows
    return SMK_OK;
}

}  // extern "C"
