// smallk_amd/csrc/switches.h -- every environment switch the library reads, in one table.
//
// The switches are the project's test surface.  A route other than the default stays selectable when a test selects it by name
// as a reference (the wave-per-column kernel the four-per-wave one must match bit for bit, the direct form) or as a recovery path
// (the one-launch-per-column W sweep), or when it is an override of a computed choice.  A variant that lost its A/B is deleted,
// code and switch, once its numbers are in profiles/ and DESIGN.md.
//
// A row states a switch's accessor, its environment name, how the text is parsed (with the default for "unset"), when
// it is read, and what it means.  No other file under csrc calls getenv (preprocess.cpp reads OMP_NUM_THREADS, which is not
// ours).  The measurements behind a switch stay in the comment at the site that uses it; tools/README.md lists the values.
//
// Plain C++17, no HIP: the host-only sanitizer build (tests/asan) includes it, the .hip files include it as host code.
#pragma once
#include <cstdint>
#include <cstdlib>

namespace smk { namespace sw {

// ---- the parse conventions (e: what getenv returned, nullptr when the variable is unset) --------------------------------------
inline bool on_unless_0(const char* e) { return !(e && e[0] == '0'); }          // default ON; off only when the text starts with '0'
inline bool on_if_nonzero(const char* e) { return e && atoi(e) != 0; }          // default OFF; on when it is a non-zero number ("" is off)
inline bool starts_with(const char* e, char c) { return e && e[0] == c; }       // default OFF; on by the first character alone ('m'ulti, 'h'ost, '1')
inline int int_or(const char* e, int unset) { return e ? atoi(e) : unset; }     // a number ("" is 0); the site states which values it honours
inline int64_t i64_or(const char* e, int64_t unset) { return e ? (int64_t)atoll(e) : unset; }
inline double double_or(const char* e, double unset) { return e ? atof(e) : unset; }
// a number that overrides a computed choice only when the variable is present: no value of it can stand for "unset"
template <typename T> struct Maybe { bool set; T v; };
inline Maybe<int> int_if_set(const char* e) { return {e != nullptr, e ? atoi(e) : 0}; }
inline Maybe<int64_t> i64_if_set(const char* e) { return {e != nullptr, e ? (int64_t)atoll(e) : 0}; }
inline Maybe<uint64_t> u64_if_set(const char* e) { return {e != nullptr, e ? (uint64_t)strtoull(e, nullptr, 10) : 0}; }

// ---- the two read times ------------------------------------------------------------------------------------------------------
// ONCE: latched at the first call for the life of the process (one instance per shared library, initialised thread-safely).
// LIVE: read on every call -- per plan, per solver or per API call -- because tests change it inside one process.
#define SMK_SW_ONCE(fn, env, parse) inline auto fn() { static const auto v = [] { const char* e = std::getenv(env); return parse; }(); return v; }
#define SMK_SW_LIVE(fn, env, parse) inline auto fn() { const char* e = std::getenv(env); return parse; }

// ---- product form and streaming products (solver.cpp, guard.cpp, bigprod.hip, matrix.cpp) -----------------------------------------
SMK_SW_LIVE(nsplit,             "SMK_NSPLIT",               int_if_set(e))          // product form: 1 native fp32 / 2 two bf16 terms / 3 bf16x3 / 4 fp16 two-term / 8 accurate fp64; unset: chosen per solver (other numbers: the default form, but no spread measurement)
SMK_SW_LIVE(bpp_small_accurate, "SMK_BPP_SMALL_ACCURATE",   on_unless_0(e))         // BPP, k in (32, 64], A of at most 2^24 entries takes the accurate form (0: keeps the fp16 form; the test suite sets it)
SMK_SW_LIVE(bp_variant,         "SMK_BP_VARIANT",           int_if_set(e))          // streaming-kernel variant (unset: by storage, form and length)
SMK_SW_LIVE(bp_variant_k64,     "SMK_BP_VARIANT_K64",       int_if_set(e))          // the same, only for k in (32, 64]
SMK_SW_LIVE(bp_splits,          "SMK_BP_SPLITS",            int_or(e, 0))           // row splits of a streaming pass, rounded up to a power of two <= 64 (<= 0: by the number of CUs)
SMK_SW_ONCE(bp_tr_variant,      "SMK_BP_TR_VARIANT",        int_or(e, -1))          // kernel shape for the transposed source of a single-copy matrix (-1: the built-in choice)
SMK_SW_ONCE(bp_temporal,        "SMK_BP_TEMPORAL",          int_or(e, -1))          // cache policy of the streamed loads: 0 non-temporal / 1 temporal (< 0: by streamed bytes)
SMK_SW_ONCE(ld_skew,            "SMK_LD_SKEW",              i64_if_set(e))          // rows added to a column stride that is a multiple of 1 MiB, rounded down to the row padding (0: off; unset: one padding)
SMK_SW_LIVE(single_copy,        "SMK_SINGLE_COPY",          starts_with(e, '1'))    // dense matrices are created without the stored transpose
SMK_SW_ONCE(guard_every,        "SMK_GUARD_EVERY",          int_or(e, 0))           // BPP: re-examine the product form every n iterations (<= 0: no guard)
SMK_SW_ONCE(guard_tau,          "SMK_GUARD_TAU",            double_or(e, 1e-4))     // the guard's threshold on cond x discrepancy
SMK_SW_ONCE(guard_verbose,      "SMK_GUARD_VERBOSE",        on_if_nonzero(e))       // one line on stderr per look of the guard

// ---- Gram matrices, packing, block pivoting (solver.cpp, kernels.hip, nnls.hip, nnls_g16.hip, wide.hip) ------------------------------
SMK_SW_ONCE(fused_gram,         "SMK_FUSED_GRAM",           on_unless_0(e))         // Gram + pack in one launch (bf16 forms); 0: two launches
SMK_SW_ONCE(reduce_pack,        "SMK_REDUCE_PACK",          on_unless_0(e))         // k <= 16: reduce the Gram partials and pack in one launch; 0: two
SMK_SW_ONCE(nnls_gram,          "SMK_NNLS_GRAM",            on_unless_0(e))         // k in (8, 16]: the NNLS launch leaves the Gram partials of the factor it solves
SMK_SW_LIVE(nnls_pack,          "SMK_NNLS_PACK",            on_unless_0(e))         // k in (8, 16] BPP: the NNLS launch also packs its factor; 0: the separate reduce-and-pack launch
SMK_SW_ONCE(gram_ride,          "SMK_GRAM_RIDE",            on_unless_0(e))         // sparse A, k in (8, 32]: the Gram matrix rides in the gather product's launches
SMK_SW_ONCE(inv_ride,           "SMK_INV_RIDE",             on_unless_0(e))         // BPP, k in (16, 64]: the Gram inverse rides in the product launch; 0: a launch of its own
SMK_SW_ONCE(inv_stream,         "SMK_INV_STREAM",           int_or(e, -1))          // that launch on a second stream: 0 nowhere / non-zero everywhere (< 0: dense and k > 32)
SMK_SW_ONCE(nnls_inv,           "SMK_NNLS_INV",             int_or(e, 1))           // block pivoting through the Gram inverse; 0: the direct form only
SMK_SW_ONCE(nnls_inv32,         "SMK_NNLS_INV32",           on_unless_0(e))         // k in (16, 32] solves through the inverse too; 0: the masked elimination
SMK_SW_ONCE(nnls_rounds,        "SMK_NNLS_ROUNDS",          int_or(e, 0))           // workgroups of the inverse-based kernels = resident workgroups x rounds (<= 0: 1 up to 65536 columns, 4 above)
SMK_SW_ONCE(nnls_g16,           "SMK_NNLS_G16",             int_or(e, 1))           // four columns per wave at k in (16, 32]; 0: a wave per column
SMK_SW_ONCE(wide_nw,            "SMK_WIDE_NW",              int_or(e, 0))           // tile kernel: 1 a wave per column / other non-zero: the workgroup per column (0: by LDS fit)
SMK_SW_ONCE(nnls_stats,         "SMK_NNLS_STATS",           on_if_nonzero(e))       // 256 device counters of block pivoting's work (smk_debug_nnls_stats)
SMK_SW_ONCE(bpp_gradw,          "SMK_BPP_GRADW",            starts_with(e, '1'))    // BPP: form the W-side gradient although it is the dual of the W-side NNLS

// ---- HALS (solver.cpp, kernels.hip) --------------------------------------------------------------------------------------------
SMK_SW_ONCE(hals_epilogue,      "SMK_HALS_EPILOGUE",        on_unless_0(e))         // k <= 32: the sweeps leave the packed operand and Gram partials; 0: separate launches
SMK_SW_ONCE(hals_w_blocked,     "SMK_HALS_W_BLOCKED",       on_unless_0(e))         // k > 64: the W sweep in blocks of 16 columns; 0: one full-row launch per column
SMK_SW_ONCE(hals_w_multi,       "SMK_HALS_W",               starts_with(e, 'm'))    // "multi": the one-launch-per-column W sweep instead of the persistent kernel
SMK_SW_ONCE(hals_spin,          "SMK_HALS_SPIN",            int_or(e, 0))           // bound of the persistent sweep's exchange polls (<= 0: 2^22; tests set 1 to force the fallback)
SMK_SW_ONCE(hals_nt,            "SMK_HALS_NT",              int_or(e, 256))         // smallest workgroup size of the persistent W sweep

// ---- stopping rule and timing (solver.cpp, progress.cpp, timing.cpp) -------------------------------------------------------------
SMK_SW_ONCE(sync_progress,      "SMK_SYNC_PROGRESS",        on_if_nonzero(e))       // check the stopping rule synchronously every iteration
SMK_SW_ONCE(progress_fused,     "SMK_PROGRESS_FUSED",       on_unless_0(e))         // the check as two launches without a copy packet; 0: four stream operations
SMK_SW_ONCE(progress_defer,     "SMK_PROGRESS_DEFER",       on_unless_0(e))         // BPP, k <= 16: the check rides in the next iteration's NNLS launches
SMK_SW_ONCE(progress_tail,      "SMK_PROGRESS_TAIL",        on_unless_0(e))         // its totals ride in the tail of the pass behind that launch; 0: one launch
SMK_SW_ONCE(progress_poll,      "SMK_PROGRESS_POLL",        on_unless_0(e))         // the host polls the pinned result slot for a tag; 0: waits for an event
SMK_SW_ONCE(progress_depth,     "SMK_PROGRESS_DEPTH",       int_or(e, 0))           // checks in flight: 2 / 3 (<= 1: one)
SMK_SW_LIVE(timing_stride,      "SMK_TIMING_STRIDE",        int_if_set(e))          // smk_solver_enable_timing: one timed pass in n, at least 1 (unset: by the bytes a pass streams)

// ---- sparse products (kernels.hip, matrix.cpp, spmm_seg.hip, spmm_blocked.hip) --------------------------------------------------------
SMK_SW_ONCE(spmm_seg,           "SMK_SPMM_SEG",             on_unless_0(e))         // ranks 3 .. 128: gather products on entry-balanced segments; 0: the column-per-lane-group kernel
SMK_SW_ONCE(spmm_seg_len,       "SMK_SPMM_SEG_LEN",         int_or(e, 64))          // entries per segment, clamped to 8 .. 4096
SMK_SW_ONCE(spmm_seg_u,         "SMK_SPMM_SEG_U",           int_or(e, 0))           // entries in flight per lane of the segment kernel (0: by rank)
SMK_SW_ONCE(spmm2_lpc,          "SMK_SPMM2_LPC",            int_or(e, 0))           // rank-2 gather product: lanes per column (0: by the average column length)
SMK_SW_ONCE(spmm_blocks,        "SMK_SPMM_BLOCKS",          int_or(e, 0))           // rank-2 gather product: row blocks of the gathered factor, 1 / 2 / 4 / 8 (else: by its size)
SMK_SW_ONCE(spmm_blocked_lpc,   "SMK_SPMM_BLOCKED_LPC",     int_or(e, 0))           // the blocked product: lanes per column (0: by the average length)
SMK_SW_ONCE(spmm_unroll,        "SMK_SPMM_UNROLL",          int_or(e, 1))           // the blocked product: columns in flight per lane group, 1 / 2 / 4
SMK_SW_ONCE(transpose_host,     "SMK_TRANSPOSE",            starts_with(e, 'h'))    // "host": the CSC transpose on the host instead of the device sort
SMK_SW_ONCE(sparse_subset_host, "SMK_SPARSE_SUBSET",        starts_with(e, 'h'))    // "host": column subsets cut on the host

// ---- RANK2 as one resident launch (solver.cpp, rank2_persist.hip) ----------------------------------------------------------------
SMK_SW_ONCE(r2_persist,         "SMK_R2_PERSIST",           int_or(e, 1))           // 0 off / 1 on within the size limit / 2 on for any size
SMK_SW_ONCE(r2_persist_nnz,     "SMK_R2_PERSIST_NNZ",       i64_or(e, (int64_t)1 << 40))   // the size limit, in stored entries
SMK_SW_ONCE(r2p_wgs,            "SMK_R2P_WGS",              int_or(e, 0))           // cap on its workgroups (<= 0: one per CU)
SMK_SW_ONCE(r2p_lds,            "SMK_R2P_LDS",              int_or(e, 1))           // 0: products and offsets only in LDS, no row-index copies
SMK_SW_ONCE(r2p_profile,        "SMK_R2P_PROFILE",          on_if_nonzero(e))       // the kernel's phase timers per factorisation on stderr

// ---- several GPUs (facade.cpp, attach.cpp, solver.cpp, comm.cpp) -----------------------------------------------------------------
SMK_SW_LIVE(num_gpus,           "SMK_NUM_GPUS",             int_or(e, 0))           // Nmf() runs column-sharded over n devices, at most 16 (<= 1: one device)
SMK_SW_LIVE(shards_on_one_gpu,  "SMK_SHARDS_ON_ONE_GPU",    on_if_nonzero(e))       // all shards / HierNMF2 workers on the current device, stand-in collectives
SMK_SW_LIVE(comm_force,         "SMK_COMM_FORCE",           on_if_nonzero(e))       // the collectives are issued at world 1 too
SMK_SW_LIVE(comm_chunks,        "SMK_COMM_CHUNKS",          int_if_set(e))          // chunks of the exchange pipeline, clamped to 1 .. 8 (unset: by the rows per rank)
SMK_SW_LIVE(comm_f64,           "SMK_COMM_F64",             int_or(e, 1))           // 0: the summed (AH')' travels as fp32 (non-zero: fp64)
SMK_SW_LIVE(comm_emulate_world, "SMK_COMM_EMULATE_WORLD",   int_or(e, 0))           // measurement hook: the geometry of rank 0 of n ranks (2 .. 64) on a one-rank communicator

// ---- HierNMF2 (hierclust.cpp) -------------------------------------------------------------------------------------------------------
SMK_SW_LIVE(clust_devices,      "SMK_CLUST_DEVICES",        int_or(e, 0))           // trial splits on n devices, at most 8 (< 2: one device)
SMK_SW_ONCE(clust_serialize,    "SMK_CLUST_SERIALIZE",      on_if_nonzero(e))       // measurement hook: the trial splits of a round run one after the other
SMK_SW_ONCE(clust_timing,       "SMK_CLUST_TIMING",         int_or(e, 0))           // level: non-zero a line per node factorisation, > 1 also the laps of the priority score
SMK_SW_LIVE(clust_timing_live,  "SMK_CLUST_TIMING",         int_or(e, 0))           // the same variable, read per run: non-zero prints the breakdown of the run
SMK_SW_ONCE(priority_host,      "SMK_PRIORITY_HOST",        on_if_nonzero(e))       // the priority score's arithmetic on the host around the device sorts

// ---- memory, seed (state.h, devmem.cpp, facade.cpp) --------------------------------------------------------------------------------
SMK_SW_ONCE(poison,             "SMK_POISON",               on_if_nonzero(e))       // debugging aid: every fresh device workspace is filled with 0xFF bytes
SMK_SW_ONCE(devmem_cache,       "SMK_DEVMEM_CACHE",         int_or(e, 1))           // 0: freed device workspaces go back to the runtime instead of the cache
SMK_SW_ONCE(devmem_cache_mb,    "SMK_DEVMEM_CACHE_MB",      i64_or(e, 4096))        // cap of that cache per device, in MiB
SMK_SW_LIVE(seed,               "SMALLK_SEED",              u64_if_set(e))          // replaces the clock seed Initialize() takes

// ---- test hooks: they make a healthy run take a recovery path ---------------------------------------------------------------------
SMK_SW_LIVE(nnls_pack_test_anorm, "SMK_NNLS_PACK_TEST_ANORM", double_or(e, 1.0))    // scales the bound behind the packing NNLS launch's row scales (the launch must flag the overflow)
SMK_SW_LIVE(r2p_test_abort,     "SMK_R2P_TEST_ABORT",       on_if_nonzero(e))       // the resident RANK2 launch reports that its workgroups did not all become resident

#undef SMK_SW_ONCE
#undef SMK_SW_LIVE

}}  // namespace smk::sw
