// smallk_amd/csrc/solver_internal.h -- what the files behind the solver handle (solver.cpp, progress.cpp, attach.cpp, factors.cpp,
// guard.cpp, timing.cpp) call of each other
#pragma once
#include "state.h"

#include <algorithm>

namespace smk {

static inline bool is_dist(const smk_solver* s) { return s->ex.ar != nullptr || s->ex.comm != nullptr; }
// the partial products as the kernels read them: W'A; (AH')', summed over the ranks when sharded; this rank's rows of that sum
static inline PartialView view1(const smk_solver* s) { return PartialView{s->P1, s->pl1.S, (i64)s->pl1.ncols_pad * s->kpp, s->kpp, 1}; }
static inline PartialView view2(const smk_solver* s)
{
    if (is_dist(s)) return PartialView{s->R2red, 1, 0, s->kpp, s->ex.red_f64 ? 1 : 0};
    return PartialView{s->P2, s->pl2.S, (i64)s->pl2.ncols_pad * s->kpp, s->kpp, 1};
}
static inline PartialView view_own(const smk_solver* s) { return PartialView{s->ex.R2own, 1, 0, s->kpp, s->ex.red_f64 ? 1 : 0}; }
// this rank's block [a, b) of chunk j of a row-sharded W (valid rows only: b <= m; empty when b <= a)
static inline void own_block(const smk_solver* s, int j, i64* a, i64* b)
{
    *a = ((i64)j * s->ex.world + s->ex.rank) * s->ex.blk;
    *b = std::min<i64>(*a + s->ex.blk, s->m);
}
// the routes of a gather product with a factor of ldx doubles per column (timed_spmm takes them, smk_solver_kernel_name names them):
// the rank-2 product by row blocks, else the entry-balanced segments, else the column-per-lane-group kernel
static inline bool blocked2_route(const smk_solver* s, int which, int ldx) { return ldx == 2 && (which == 0 ? s->a->bA : s->a->bAt).nb > 1; }
static inline bool seg_route(const smk_solver* s, int which, int ldx, i64 ncols)
{
    const SegPlan& seg = (which == 0) ? s->a->segA : s->a->segAt;
    return ldx == s->KP && s->k > 2 && !is_wide(s->k) && seg.ncols == ncols && seg.rowflag && !seg.uniform;
}

// solver.cpp
int plan_products(smk_solver* s);
int alloc_product_buffers(smk_solver* s);
int solver_init(smk_solver* s);
int normalize_device(smk_solver* s);
int wait_r2(smk_solver* s);
int gather_w(smk_solver* s);
int dist_agree(smk_solver* s);
int sync_and_check(smk_solver* s, int* fail_iter);

// attach.cpp
int scatter_own(smk_solver* s);
// guard.cpp
int guard_step(smk_solver* s);
// timing.cpp
int resolve_events(smk_solver* s);

// progress.cpp
bool check_rides_in_nnls(const smk_solver* s);
int ensure_snapshot(smk_solver* s, int b, bool attaching = false);
int check_totals(smk_solver* s, BigProdPlan* pl);
int update_progress(smk_solver* s, int iter_index, double* metric);
int progress_prealloc(smk_solver* s);
int progress_depth(const smk_solver* s);
int progress_begin(smk_solver* s, int b, bool snapshot, bool allow_defer = true);
int progress_end(smk_solver* s, int b, int iter_index, double* metric);
int progress_restore(smk_solver* s, int b);

}  // namespace smk
