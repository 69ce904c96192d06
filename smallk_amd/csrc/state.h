// smallk_amd/csrc/state.h -- host state shared by context.cpp, matrix.cpp and the files behind the solver handle (solver.cpp, progress.cpp,
// attach.cpp, factors.cpp, guard.cpp, timing.cpp): the per-thread device
// context, the resident matrix and the solver handle behind the opaque types of include/smallk_amd.h, and the
// few functions that cross those files.
#pragma once
#include "common.h"
#include "switches.h"
#include "owned.h"
#include "../../include/smallk_amd.h"

#include <chrono>
#include <cstdlib>
#include <vector>

namespace smk {

// One device context per process by default; the single-process multi-GPU driver (smk_nmf_dense_sharded) runs
// one host thread per shard and gives each its own context through t_ctx.
struct DeviceCtx {
    bool init = false;
    int cus = 256;
    hipStream_t stream = nullptr;
    bool own_stream = false;
    int live_solvers = 0;               // solver handles cache the stream: it cannot change under them
    std::vector<struct ::smk_matrix*> mats;   // live matrices: they follow the context's stream when it is replaced
};
// context.cpp.  __thread, not thread_local: an extern thread_local is read through a wrapper that first looks for a dynamic
// initialiser in the defining file, and ctx() is read on the per-iteration path
extern DeviceCtx g_ctx;
extern __thread DeviceCtx* t_ctx;
inline DeviceCtx& ctx() { return t_ctx ? *t_ctx : g_ctx; }

static inline double wall_us()
{
    using namespace std::chrono;
    return (double)duration_cast<nanoseconds>(steady_clock::now().time_since_epoch()).count() * 1e-3;
}

static const int MAX_CHUNKS = 8;
static const int GRAM_BLOCKS = 256;

}  // namespace smk

using namespace smk;      // context.cpp, matrix.cpp and solver.cpp are written in its names, and so are the two handles below

struct smk_matrix {
    i64 m = 0, n_global = 0, c0 = 0, n = 0;
    int storage = SMK_STORE_F32;
    hipStream_t st = nullptr;                        // stream of the context that created it
    smk::DeviceCtx* owner = nullptr;                 // the context whose registry lists it (nullptr once that context is gone)
    mutable float ascale = 0.f;                      // fp16 two-term products: power of two with max|A| ascale in [2^13, 2^14); 0 = not yet measured
    mutable int col_spread_log2 = -1;                // log2(largest / smallest non-zero column maximum of |A|); -1 = not yet measured
    mutable double colnorm_max = -1.0, rownorm_max = -1.0;   // largest 2-norm of a column / a row of A (dense; NnlsPack's bound); < 0 = not yet measured
    void* A = nullptr;  i64 ldA = 0, colsA = 0;      // m_pad x n_pad
    void* At = nullptr; i64 ldAt = 0, colsAt = 0;    // n_pad x m_pad
    // single copy (MU / HALS): no stored transpose -- the H*A' pass contracts down the strided direction of A itself
    // (bigprod.hip: TRB for bf16, TAIL = 2 for fp32), as the reference's MU / HALS do (Gemm(NORMAL, TRANSPOSE) on A, nmf_solver_mu.hpp:121-164,
    // nmf_solver_hals.hpp:166-199); half the footprint, no transpose pass at load time
    bool single = false;
    // sparse A: CSC of the local columns and CSC of its transpose (fp64 values, 64-bit offsets)
    bool sparse = false;
    i64 nnz = 0;
    i64 *colptr = nullptr, *colptr_t = nullptr;
    unsigned *rowidx = nullptr, *rowidx_t = nullptr;
    double *val = nullptr, *val_t = nullptr;
    // host copy of the CSC (column subsets for HierNMF2 nodes are cut on the host)
    // RANK2 on a factor larger than an L2: the entries regrouped by row block (spmm_blocked.hip), built on first use
    mutable BlockedCsc bA, bAt;
    mutable bool blocked_tried = false;
    // ranks 3 .. 128 on sparse A: the entry-balanced segments of CSC(A) / CSC(A') (spmm_seg.hip), built on first use
    mutable SegPlan segA, segAt;
    mutable bool seg_tried = false;
    mutable std::vector<unsigned> h_colptr, h_rowidx;     // fetched on first use (matrix_host_csc)
    mutable std::vector<double> h_val;
    // sparse A, residual.cpp: whether the CSC stores an entry twice (they add up in every product, so sum a_e^2 over the stored
    // entries is not ||A||^2): -1 = not yet looked, 0 = no, 1 = yes and dup_colsq holds the sum of squares per column of the
    // merged entries.  Looked up once: a sparse matrix does not change after creation.
    mutable int dup_state = -1;
    mutable double* dup_colsq = nullptr;
    // kl.cpp (sparse A) / kl_dense.cpp (dense A; reset with new contents): whether a stored value is negative (the KL divergence
    // refuses such a matrix): -1 = not yet looked, 0 = no, 1 = yes
    mutable int kl_negative = -1;
    // dense A, beta_dense.cpp: whether a stored value is zero or negative (beta <= 0 refuses such a matrix); written by the look that
    // fills kl_negative and valid while kl_negative >= 0, so every reset of that record resets this one
    mutable int kl_zero = 0;
    mutable smk::Owned own;                          // every device block above (the lazily built stored transpose included); the blocked CSC and the segment plans free themselves
};

// The stopping rule's check (progress.cpp), evaluated one iteration late on the schedule of check_ring.h: per slot of the ring a
// pinned result, an event and a snapshot of (W, H, W'W), so that a speculative iteration can be undone.  Everything lives in the
// solver's Owned.
struct ProgressCheck {
    static constexpr int PROG_SLOTS = 4;         // array bound: the largest depth + 1 (a run uses depth + 1 of them)
    struct ProgSlot { double h[8]; int flag; int fused; };     // fused: the flag travels in h[5]
    ProgSlot* pin = nullptr;
    hipEvent_t pev[PROG_SLOTS] = {nullptr, nullptr, nullptr, nullptr};
    double poll_tag[PROG_SLOTS] = {0, 0, 0, 0};      // != 0: the kernel stores this into h[7] behind the result; progress_end polls the slot (no event)
    double* snap[PROG_SLOTS] = {nullptr, nullptr, nullptr, nullptr};
    double* pin_r2[PROG_SLOTS] = {nullptr, nullptr, nullptr, nullptr};      // RANK2: pinned copies of the progress partials (the host sums them)
    // deferred check (BPP, k <= 16; check_rides_in_nnls): the slot whose totals the NEXT H-side NNLS launch produces, the
    // iteration tag up to which a failure counts for it, whether its snapshot is being written by this iteration's NNLS launches
    int pg_defer_slot = -1, pg_defer_tag = 0, pg_defer_nblk = 0, iter_snap_slot = -1;
    bool pg_defer_snap = false;
    int pg_totals_slot = -1;                 // >= 0: the H-side launch has left the partial sums of this slot's check; its totals are due
    unsigned check_routes[4] = {0, 0, 0, 0}; // checks formed so far by route (smk_solver_kernel_name(2)): 1 own launches, 2 NNLS riders + totals launch, 3 riders + pass tail
    double pg0 = 1.0, last_metric = 1.0;     // the estimator: PG_RATIO's first norm, the metric last read
    // the scalars of the check evaluated last (smk_solver_progress_sums): projected sums of W and H (PG_RATIO), ||W - Wprev||^2 and
    // ||W||^2 (DELTA_FNORM), the pair the rule does not use reads 0; sums_state: 0 no check yet, 1 valid, 2 the resident RANK2
    // kernel finished the run (it returns pg0 and the metric only)
    double sums[4] = {0, 0, 0, 0};
    int sums_state = 0;
    void reset() { pg_defer_slot = iter_snap_slot = pg_totals_slot = -1; }      // nothing deferred, nothing promised, no totals due
    void reset_estimator() { pg0 = last_metric = 1.0; sums_state = 0; }         // a run from the start
};

// What one launch tells the next about a factor (solver.cpp).  smk_solver::hand[f] is indexed by the FACTOR, 0 = W and 1 = H, and by
// nothing else: the NNLS launch of side 0 solves H against W'W, so it reads hand[0] (is W the output of a solve, is the inverse of
// W'W in place) and writes hand[1] (what it left of H).
enum class Inverse {
    none,               // nobody has formed it: launch_nnls_bpp does, in stream order
    ride_due,           // the product launch that follows this Gram matrix is to carry it (start_inverse)
    on_side_stream,     // enqueued on st_inv, ev_inv[f] recorded behind it: the solve waits for that event
    done                // in inv_scratch(f), ordered before the main stream
};
struct Handoff {
    // what the launch that last wrote this factor left
    bool from_nnls = false;          // the factor is the output of an NNLS launch of this run (hence >= 0)
    bool packed_by_solve = false;    // that launch also packed it (NnlsPack: k in (8, 16], BPP, fp16 form, one GPU -- C2) ...
    int gram_partials = 0;           // ... and left that many Gram partials of it in gram_scratch (k <= 16; 0: none)
    // what this factor's Gram matrix owes the next product of this factor
    bool packed_fresh = false;       // the Gram launch has already written packW / packH for that product
    int tail_nblk = 0;               // > 0: the product carries the reduction of that many partials in its tail (BigProdPlan::tail_*)
    bool gram_ride = false;          // sparse, k in (8, 32]: the Gram matrix is due and rides in the two launches of the gather product (gram_factor, timed_spmm)
    // the inverse of this factor's Gram matrix (BPP, k in (16, 64]): start_inverse begins every life of it with forget_inverse()
    Inverse inverse = Inverse::none;
    void forget_inverse() { inverse = Inverse::none; }                       // the Gram matrix is new
    void inverse_will_ride() { inverse = Inverse::ride_due; }                // the product launch that follows is to carry it
    bool take_inverse_ride()                                                 // "this launch will carry it" (asked by every product launch)
    {
        if (inverse != Inverse::ride_due) return false;
        inverse = Inverse::none;                                             // until the launch says it did
        return true;
    }
    void inverse_carried() { inverse = Inverse::done; }                      // the launch returned 1
    void inverse_sent_to_side_stream() { inverse = Inverse::on_side_stream; }
    bool inverse_on_side_stream() const { return inverse == Inverse::on_side_stream; }
    void inverse_joined() { inverse = Inverse::done; }                       // the main stream waits for ev_inv[f]
    void inverse_formed_by_solve() { inverse = Inverse::done; }              // launch_nnls_bpp found none and formed it itself
    bool inverse_ready() const { return inverse == Inverse::done; }
    bool take_gram_ride() { const bool due = gram_ride; gram_ride = false; return due; }
    // the factor is the caller's (or a restored snapshot, or about to be): nothing is known to come from an NNLS launch, nothing
    // is owed, nothing is in flight that anybody will wait for
    void reset() { *this = Handoff(); }
};

// Run-time guard of the product form (guard.cpp): a column sample of A, its accurate-form product, the comparison scalars + both
// Gram matrices on their way to the host
struct ProductGuard {
    void* As = nullptr;
    unsigned* cols = nullptr;
    double *P = nullptr, *dev = nullptr, *pin = nullptr;
    hipEvent_t ev = nullptr;
    BigProdPlan pl[MAX_GROUPS];
    int ncols = 0, checks = 0, fired = 0;
    bool pending = false, off = false;
    double last = 0.0;                     // cond * delta of the last check
};

// The whole RANK2 factorisation as one resident launch (rank2_persist.hip): second H buffer, the rows of (AH')', partial sums,
// barrier words, result slots (device + pinned); latched off after an aborted launch
struct ResidentRank2 {
    double *hc1 = nullptr, *r2c = nullptr, *part = nullptr, *out = nullptr, *pin = nullptr;
    unsigned* sync = nullptr;
    bool off = false;
};

// smk_solver_kernel_time (timing.cpp; the spans are opened on the per-iteration path, solver.cpp)
struct Timing {
    bool on = false;
    // a pair of event records around a launch costs ~11 us of idle time (5.7 us in front of the kernel, 5.8 behind it: measured
    // on C2, where that was 23 of 119 us per iteration): passes shorter than ~0.2 ms are timed one launch in `stride`
    // and the totals scaled back up, so that measuring does not change what is measured
    int stride = 1;
    unsigned pass_counter[2] = {0, 0}, pass_sampled[2] = {0, 0};     // passes seen / passes that carried events since enable_timing
    bool pass_timed[2] = {false, false};     // this W'A / H*At pass (all of its launches, and the collectives behind it) is a timed sample
    struct TimedSpan { hipEvent_t e0, e1; int counts; };     // counts: this span completes one launch (a pass cut into chunks is ONE launch)
    // 0: W'A passes, 1: H*At passes, 2: the big collectives of a sharded run (on st2), 3: what the MAIN stream spends waiting
    // for events of the collective stream (the exposed part of the exchange: the bracket holds nothing but the wait)
    // 4: the same bracket around a wait for an event that completed long ago -- what a bracket costs by itself (three packets
    // through the command processor, ~15 us): exposure = slot 3 - brackets x the average of slot 4
    std::vector<TimedSpan> ev[6];       // 0 / 1: the passes, 2 - 4: collectives, waits, calibration, 5: the block-pivoting launches
    std::vector<TimedSpan> span_pool;   // event pairs whose times have been read (resolve_events): span_open hands them out again
    double acc_ms[6] = {0, 0, 0, 0, 0, 0};
    int launches[6] = {0, 0, 0, 0, 0, 0};
    hipEvent_t ev_cal = nullptr;          // recorded once on the collective stream
    unsigned cal_counter = 0;
};

// comm: a native communicator (RCCL or the in-process stand-in, comm.cpp) or -- test hook -- a host callback (attach.cpp; the
// exchange itself runs on the per-iteration path, solver.cpp)
struct Exchange {
    int rank = 0, world = 1;
    smk_allreduce_fn ar = nullptr;
    double* home[3] = {nullptr, nullptr, nullptr};   // callback hook: where Gh / scal / Wt pointed before smk_solver_set_comm moved them into the caller's workspace
    void* ar_user = nullptr;
    smk_comm* comm = nullptr;
    void* comm_ws = nullptr;              // owned workspace when a native communicator is attached
    // Native communicator: EVERY collective is issued on st2 (one stream per communicator), tied to the main stream by
    // events.  The rows of A (= columns of A', rows of W) are cut into `nchunk` chunks of world * blk rows; block r of a
    // chunk belongs to rank r (block-cyclic), so a chunk is at once a contiguous range of the H*At pass, the send buffer
    // of one reduce-scatter / all-reduce and the receive buffer of one all-gather: the exchange of chunk j runs on st2
    // while the streaming product works on chunk j + 1.
    int nchunk = 1;
    i64 blk = 0, rows_cap = 0;            // rows per (chunk, rank) block (multiple of 256); world * nchunk * blk >= m_pad
    bool r2_alias = false;                // the H*At pass writes ONE slab of fp64 partial products: the collectives work on it directly (no copy)
    bool red_f64 = false;                 // element type of the summed (AH')' on the wire (native communicator: fp64 unless SMK_COMM_F64=0)
    bool w_sharded = false;               // BPP: every rank solves (and holds current) only its own blocks of W
    bool w_full = true;                   // all rows of the fp64 W on this rank are current
    // a row-sharded W: this rank's blocks back to back (KP x nchunk*blk; the n_own valid rows are a prefix because only the
    // last non-empty block of a rank can be short) and, in the same order, its rows of the summed (AH')'
    double* Wown = nullptr;
    void* R2own = nullptr;
    i64 n_own = 0;
    hipStream_t st2 = nullptr;
    hipEvent_t ev_gram = nullptr, ev_gh = nullptr, ev_x = nullptr, ev_y = nullptr;
    hipEvent_t ev_c[MAX_CHUNKS] = {}, ev_r[MAX_CHUNKS] = {}, ev_a[MAX_CHUNKS] = {};
    bool gh_pending = false;
    bool r2_pending = false;              // the chunk exchanges of the last H*At pass have not been joined by the main stream yet
};

// The solver handle.  Its subsystems are members held by value, each with its comment at its struct above; every device block,
// pinned block, event and stream of every one of them is created through the handle's single `own`.
struct smk_solver {
    smk_options o;
    const smk_matrix* a = nullptr;
    int k = 0, KP = 0, kpp = 0, nsplit = 3;
    i64 m = 0, n = 0;
    hipStream_t st = nullptr;
    smk::Owned own;                       // every device block, pinned block, event and stream below was created through it and is released by it alone
    double *H = nullptr, *Wt = nullptr, *Gw = nullptr, *Gh = nullptr, *gram_scratch = nullptr;
    double* seg_pieces[2] = {nullptr, nullptr};     // sparse A, spmm_seg.hip: partial sums of the long columns of pass 0 / 1
    double *Wprev = nullptr, *hals_scratch = nullptr, *pg_partials = nullptr, *scal = nullptr, *tmpW = nullptr;
    double* wide_tmp = nullptr;           // k > 128: max(m, n) x KP, the product X G of the MU rule and of the gradients
    double* tmpH = nullptr;               // k x n compact copy of H for the host (get_factors)
    // RANK2 (rank2.hip): scratch of the fused solve / progress kernels (ticket + partial sums), W'W of the W just solved
    // (before its normalisation), and -- sparse A -- compact N x 2 copies of the factors for the gather products
    double *r2_scratch = nullptr, *r2_prog = nullptr, *Graw = nullptr, *Hc = nullptr, *Wc = nullptr;
    ResidentRank2 r2p;
    ProductGuard guard;
    bool wc_valid = false;
    double* nnls_scratch = nullptr;       // BPP: inverses of W'W and HH' + path selectors (k in (16, 64]), two halves
    int hals_ep_blocks = 0;               // HALS, k <= 32: Gram partials the sweeps' epilogues may write into gram_scratch (0: epilogues off)
    hipStream_t st_inv = nullptr;         // the 0.1 ms single-workgroup inversions run here, beside the streaming products
    hipEvent_t ev_g[2] = {nullptr, nullptr}, ev_inv[2] = {nullptr, nullptr};
    Handoff hand[2];                      // by factor: 0 = W, 1 = H
    void forget_handoffs() { hand[0].reset(); hand[1].reset(); }
    double *xscale[2] = {nullptr, nullptr}, *oscale[2] = {nullptr, nullptr};   // fp16 two-term products: row scales of W / H (from the Gram diagonal) and their inverses
    // k in (8, 16], BPP, fp16 form, one GPU (C2): the NNLS launch also PACKS the factor it solves (row scales from an a-priori
    // bound, NnlsPack) and the reduction of its Gram partials rides in the streaming pass that follows (Handoff::tail_nblk),
    // so nothing stands between the solve and the product.
    bool pack_in_solve = false;              // the shape qualifies (decided with the plans)
    bool pack_in_solve_off = false;          // latched by pack_fail_soft
    // HALS: the fused W sweep needs every workgroup resident; if its bounded polls ever expire (flag -3) the run is
    // repeated from the initial factors on the one-launch-per-column path, latched for the life of the handle
    double *W0c = nullptr, *H0c = nullptr;
    bool hals_multi = false;
    int hals_calls = 0;
    void *packW = nullptr, *packH = nullptr;
    double *P1 = nullptr, *P2 = nullptr;
    float* R2red = nullptr;
    BigProdPlan pl1, pl2;                 // first group of each pass (row splits, P layout)
    BigProdPlan pg1[MAX_GROUPS], pg2[MAX_GROUPS];   // all groups: k > 64 streams the big matrix once per 64 factor rows
    int ng = 1;
    int* fail_flag = nullptr;
    int iter = 0;
    bool have_factors = false, inited = false, normalized = false;
    ProgressCheck pc;                     // the stopping rule's check (progress.cpp)
    size_t pg_half = 2048;
    Exchange ex;
    Timing timing;
};

namespace smk {

// context.cpp: the registry of live matrices of the calling thread's context
void repoint_matrices(hipStream_t st);
void orphan_matrices();
void register_matrix(smk_matrix* a);
void unregister_matrix(smk_matrix* a);

// matrix.cpp: the lazily built parts of a resident matrix.  The solver calls them while it plans (smk_solver_create,
// set_factors, a re-plan after a fail-soft or a fired guard), never from a regular iteration.
int matrix_materialize_transpose(const smk_matrix* ca);
int ensure_seg_plans(const smk_matrix* a);
int matrix_measure_scale(const smk_matrix* a, hipStream_t st);
int matrix_measure_norms(const smk_matrix* a, hipStream_t st);
int matrix_host_csc(const smk_matrix* a);         // the host copy of a resident CSC (h_colptr / h_rowidx / h_val), fetched on first use

// residual.cpp: the once-per-matrix duplicate record of a sparse matrix (dup_state, dup_colsq; fetches the host copy of the CSC)
int ensure_dup_record(const smk_matrix* a);

// matrix.cpp: a strided view in device memory handed in by a caller (the *_device entries).  check_device_view: SMK_OK, or
// SMK_BAD_PARAM with the error text set -- null pointer, unknown element type, negative stride (or a zero stride of an output),
// not device memory of the current device, or an extent that leaves the allocation; nothing is launched.
// join_caller_stream: the library's stream waits for what the caller has enqueued on its own so far (event record + stream
// wait).  The event belongs to `own`, a local of the entry: it lives until the entry returns and is destroyed on every path.
int check_device_view(const void* p, int dtype, i64 rows, i64 cols, i64 rs, i64 cs, bool output, const char* what);
int join_caller_stream(smk::Owned& own, hipStream_t lib, void* caller_stream);

// assign.cpp: labels / memberships of H (k x n) and top terms of W (m x k) from strided fp64 / fp32 views in device memory, on `st`
// (DESIGN.md 14).  A view that is not k-contiguous is converted into a workspace of `own` first.  The outputs are device memory the
// caller has checked.  Both synchronise `st` before they return.
int labels_from_view(const void* H, int dtype, i64 rs, i64 cs, int k, i64 n, hipStream_t st, smk::Owned& own, void* labels, void* memberships);
int top_terms_from_view(const void* W, int dtype, i64 rs, i64 cs, i64 m, int k, int maxterms, hipStream_t st, smk::Owned& own, void* term_indices);

}  // namespace smk
