// smallk_amd/csrc/solver_internal.h -- what solver.cpp and progress.cpp call of each other
#pragma once
#include "state.h"

namespace smk {

static inline bool is_dist(const smk_solver* s) { return s->ar != nullptr || s->comm != nullptr; }
// the partial products as the kernels read them: W'A; (AH')', summed over the ranks when sharded; this rank's rows of that sum
static inline PartialView view1(const smk_solver* s) { return PartialView{s->P1, s->pl1.S, (i64)s->pl1.ncols_pad * s->kpp, s->kpp, 1}; }
static inline PartialView view2(const smk_solver* s)
{
    if (is_dist(s)) return PartialView{s->R2red, 1, 0, s->kpp, s->red_f64 ? 1 : 0};
    return PartialView{s->P2, s->pl2.S, (i64)s->pl2.ncols_pad * s->kpp, s->kpp, 1};
}
static inline PartialView view_own(const smk_solver* s) { return PartialView{s->R2own, 1, 0, s->kpp, s->red_f64 ? 1 : 0}; }

// solver.cpp
int wait_r2(smk_solver* s);
int gather_w(smk_solver* s);
int dist_agree(smk_solver* s);
int sync_and_check(smk_solver* s, int* fail_iter);

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
