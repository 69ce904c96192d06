// smallk_amd/csrc/bigprod_plan.h -- what the streaming products are planned from, each fact once: the variant tables, the rule for
// whether a variant fits a k and a form, the variant a plan settles on, which launches can carry the riders, and the product form
// a solver takes.  bigprod.hip builds its kernels and its dispatch from these tables; solver.cpp calls the form functions.
// Plain C++17, no HIP: tests/bigprod_plan/plan_dump.cpp includes it by itself, the .hip files include it as host code.
#pragma once
#include <cstdint>

namespace smk {

// Device storage of the big matrix A (and its transpose).
enum Storage { STORE_F32 = 0, STORE_BF16 = 1 };
// the solver's algorithms (= SMK_ALG_* of include/smallk_amd.h)
enum Algorithm { ALG_MU = 0, ALG_HALS = 1, ALG_RANK2 = 2, ALG_BPP = 3 };

// product form ("nsplit"): 1..3 = bf16 terms of the skinny operand; NSPLIT_F16X2 = two fp16 terms with per-row power-of-two scales
constexpr int NSPLIT_F16X2 = 4;
// the accurate form: A's entries (exact in fp64) times the fp64 factor itself on the fp64 matrix cores (v_mfma_f64_16x16x4),
// fp64 accumulation throughout -- no packed operand; Xp of launch_bigprod is then the factor (KP doubles per column, rows
// from the plan's k0 on)
constexpr int NSPLIT_F64 = 8;
// number of 32-wide k tiles of the streaming product
constexpr int kt_of(int k) { return (k + 31) / 32; }
// terms of the packed operand a form stages per k tile
constexpr int pack_terms(int nsplit) { return nsplit == NSPLIT_F16X2 ? 2 : nsplit; }
// the form a plan carries: fp32 storage takes 3 as the bf16x3 emulation, 2 / 4 as the two-term forms, anything below as the native fp32 MFMA
constexpr int plan_nsplit(int storage, int nsplit) { return storage == STORE_BF16 ? nsplit : (nsplit >= 2 ? nsplit : 1); }

// an override that holds only when its variable is present (sw::Maybe<int> of switches.h, without the environment)
struct Want { bool set; int v; };

// ---- kernel variants (tile shape / pipeline depth); chosen per plan, SMK_BP_VARIANT overrides ----------------------------------
// bigprod_kernel: variant = index
struct BPRow { int mb, nstage, cw, wk, nwl; };      // rows per stage, ring depth, 128-column tiles per workgroup, wave groups along k, loader waves
inline constexpr BPRow kVariants[] = {
    {64, 3, 1, 1, 0},    // 0: 128 cols x 64 rows, 3-deep ring
    {64, 4, 1, 1, 0},    // 1
    {64, 5, 1, 1, 0},    // 2
    {128, 2, 1, 1, 0},   // 3
    {128, 3, 1, 1, 0},   // 4
    {64, 3, 2, 1, 0},    // 5: 256 cols per workgroup
    {64, 2, 1, 1, 0},    // 6: two workgroups per CU
    {32, 2, 1, 1, 0},    // 7: 32-row stages (fp32: one 128-B line per column per stage)
    {32, 3, 1, 1, 0},    // 8
    {32, 4, 1, 1, 0},    // 9
    {64, 2, 1, 2, 0},    // 10: k in (32,64]: 8 waves, the two k tiles on different waves
    {64, 3, 1, 2, 0},    // 11
    {64, 4, 1, 2, 0},    // 12
    {32, 4, 1, 2, 0},    // 13
    {64, 2, 2, 2, 0},    // 14: 256 columns, 8 waves
    // wave-specialised: +4 (or +2) loader waves that only issue the LDS-DMA loads
    {64, 3, 1, 1, 4},    // 15
    {64, 4, 1, 1, 4},    // 16
    {64, 5, 1, 1, 4},    // 17
    {64, 3, 1, 2, 4},    // 18: k in (32,64]
    {64, 4, 1, 2, 4},    // 19
    {32, 4, 1, 1, 2},    // 20: fp32 emulation, k <= 32
    {32, 4, 1, 2, 4},    // 21: fp32 emulation, k in (32,64]
    {32, 5, 1, 2, 4},    // 22
    {64, 2, 1, 1, 4},    // 23
};
constexpr int kNumVariants = (int)(sizeof(kVariants) / sizeof(kVariants[0]));

// the fp32-storage kernels: variant = 100 + index.  `arg` is the workgroups-per-SIMD hint (WPS) of bigprod_f3_kernel and the
// schedule / experiment mask (PIN) of the software-pipelined bigprod_f3p_kernel; bf / f16: the row is built for the two- and
// three-term bf16 forms / for the fp16 two-term form; tail: also built with TAIL = 1 at one k tile (fp16 form)
enum F3Kernel { F3 = 0, F3P = 1 };
struct F3Row { int kernel, mb, nstage, nwl, fold, arg; bool bf, f16, tail; };
inline constexpr F3Row kF3Variants[] = {
    {F3, 32, 2, 0, 2, 2, true, false, false},     // 100: no loader waves, two workgroups per CU
    {F3, 32, 3, 0, 2, 2, true, false, false},     // 101
    {F3, 32, 4, 4, 2, 2, true, false, false},     // 102: 4 loader waves, one workgroup per CU, deep ring
    {F3, 32, 5, 4, 2, 2, true, false, false},     // 103
    {F3, 32, 2, 2, 2, 3, true, false, false},     // 104: 2 loader waves, two workgroups per CU (168 registers)
    {F3, 64, 2, 0, 1, 2, true, false, false},     // 105: 64-row stages
    {F3, 64, 2, 4, 1, 2, true, false, false},     // 106
    {F3, 32, 4, 4, 4, 2, true, false, false},     // 107: fold every 4 stages (128-row chains)
    {F3, 32, 2, 0, 4, 2, true, true, true},       // 108
    {F3, 32, 4, 2, 2, 2, true, false, false},     // 109
    // software-pipelined kernel (bigprod_f3p_kernel)
    {F3P, 32, 4, 4, 4, 1, true, true, false},     // 110: 4 loader waves, 4-deep ring, fold every 4 stages
    {F3P, 32, 5, 4, 4, 1, true, true, false},     // 111
    {F3P, 32, 5, 4, 2, 1, true, false, false},    // 112
    {F3P, 32, 4, 2, 4, 1, true, false, false},    // 113: 2 loader waves
    {F3P, 32, 5, 2, 4, 1, true, false, false},    // 114
    {F3P, 32, 3, 2, 4, 1, true, true, false},     // 115: shallow ring, two workgroups per CU fit
    {F3P, 32, 5, 4, 8, 1, true, false, false},    // 116: fold every 8 stages
    {F3P, 32, 5, 4, 4, 0, true, false, false},    // 117: as 111 without the pinned interleave (compiler's own schedule)
    {F3P, 32, 5, 4, 4, 2, true, false, false},    // 118: EXPERIMENT no bf16 split
    {F3P, 32, 5, 4, 4, 4, true, false, false},    // 119: EXPERIMENT no MFMA
    {F3P, 32, 5, 4, 4, 6, true, false, false},    // 120: EXPERIMENT neither
    {F3P, 32, 5, 4, 4, 9, true, false, false},    // 121: loader waves at priority 3
    {F3P, 32, 5, 4, 4, 8, true, false, false},    // 122: loader priority, compiler schedule
    {F3P, 32, 5, 4, 4, 16, true, false, false},   // 123: EXPERIMENT no X fetch (full compute)
    {F3P, 32, 5, 4, 4, 22, true, false, false},   // 124: EXPERIMENT no X fetch, no MFMA, no split
    {F3, 32, 2, 0, 8, 2, true, true, true},       // 125: as 108, folding into fp64 every 8 stages (256-row fp32 chains)
    {F3, 32, 3, 0, 4, 2, true, true, false},      // 126: as 108 with a 3-deep ring
    {F3, 32, 2, 0, 16, 2, true, true, false},     // 127: as 125, folding every 16 stages (512-row fp32 chains)
    {F3, 32, 2, 0, 2, 2, false, true, true},      // 128: as 108, folding every 2 stages (64-row fp32 chains)
    {F3, 32, 2, 0, 1, 2, false, true, true},      // 129: as 108, folding every stage (32-row fp32 chains: two roundings per accumulator and fold)
};
constexpr int kNumF3 = (int)(sizeof(kF3Variants) / sizeof(kF3Variants[0]));
constexpr int ACCURATE_VARIANT = 200;               // what a plan of the accurate form reports

constexpr bool is_f3_variant(int v) { return v >= 100 && v < 100 + kNumF3; }

// ---- does a shape fit?  A stage (the tile of A plus the operand fragments of its rows) is fetched as 1-KiB wave-level loads ----
// MFMA steps per stage of bigprod_kernel: 16 rows each on the bf16 MFMA (bf16 storage, bf16x3 emulation), two 16-B chunks on the fp32 one
constexpr int bp_steps(int ebytes, int nsplit, int mb) { return (ebytes == 2 || nsplit == 3) ? mb / 16 : mb / (16 / ebytes) / 2; }
constexpr int bp_stage_bytes(int ebytes, int kt, int nsplit, const BPRow& r) { return 128 * r.cw * r.mb * ebytes + bp_steps(ebytes, nsplit, r.mb) * nsplit * kt * 1024; }
constexpr int f3_stage_bytes(const F3Row& r, int kt, int terms) { return 128 * r.mb * 4 + (r.mb / 16) * terms * kt * 1024; }
// the loads of a stage split evenly over the loading waves, the stages in flight stay within vmcnt (a 6-bit counter), the ring
// stays within the 160 KiB of LDS
constexpr bool ring_fits(int stage_bytes, int loading_waves, int nstage)
{
    const int ti = stage_bytes / 1024;
    return ti % loading_waves == 0 && ti / loading_waves * (nstage - 1) <= 63 && stage_bytes * nstage <= 160 * 1024;
}
constexpr bool bp_fits(int ebytes, int kt, int nsplit, const BPRow& r)
{
    if (kt % r.wk != 0 || bp_steps(ebytes, nsplit, r.mb) < 1) return false;      // k tiles split evenly over the wave groups
    return ring_fits(bp_stage_bytes(ebytes, kt, nsplit, r), r.nwl > 0 ? r.nwl : 4 * r.wk, r.nstage);
}
constexpr bool f3_fits(const F3Row& r, int kt, int terms) { return ring_fits(f3_stage_bytes(r, kt, terms), r.nwl > 0 ? r.nwl : 4, r.nstage); }

// ---- the variant a plan settles on.  want / want_k64: SMK_BP_VARIANT / SMK_BP_VARIANT_K64; tr: the H*A' pass taken from A itself ----
constexpr int f16_variant_by_length(int64_t len) { return len >= 65536 ? 125 : len >= 16384 ? 108 : len >= 4096 ? 128 : 129; }
constexpr int choose_variant(int storage, int kt, int nsplit, int64_t len, Want want, Want want_k64, bool tr = false)
{
    // fp32: the two-workgroup shape of bigprod_f3_kernel (32-column stages, 2-deep ring), the fold interval by the contraction length as
    // below.  bf16: k <= 32: 4 waves, 2-deep ring, two workgroups per CU; k in (32, 64]: 8 compute + 4 loader waves, 3-deep
    if (tr) return storage == STORE_F32 ? f16_variant_by_length(len) : kt == 2 ? 18 : 6;
    if (nsplit == NSPLIT_F64) return ACCURATE_VARIANT;
    const int ns = plan_nsplit(storage, nsplit);
    // measured best on MI355X: bf16 -> 64-row stages, 2-deep ring, 2 workgroups per CU (C3: 5.98 TB/s)
    int v = (storage == STORE_BF16) ? 6 : 7;
    // k in (32,64]: 8 compute waves (one k tile each) + 4 loader waves
    if (kt == 2) v = (storage == STORE_BF16) ? 18 : 21;
    // fp32 A as bf16 planes: the second-generation kernels (power-bound at ~4.1 TB/s for k = 64)
    if (storage == STORE_F32 && ns >= 2) v = (kt == 2) ? 108 : 115;
    // fp16 two-term form: the two-workgroup kernel wins or ties at every shape measured (C2, 32768 x 8192 k = 32, both
    // passes of a C4 shard); the pipelined ones stay selectable (110, 111, 115)
    // The error of this form is the fp32 accumulation of the 22-bit hi * hi products (one rounding per MFMA), so it falls with
    // the length of the fp32 chains (stages between two folds into fp64) and, relative to the result, with the number of
    // folds: the fold interval follows the contraction length so that the product stays at 1e-8 .. 2e-8 of the exact one at
    // every size (profiles/r04_fold_interval_sweep.txt, max over 512 entries against an fp64 host product: len 1500 9.2e-8
    // with 8 stages per fold, 1.9e-8 with 1; len 8192 4.4e-8 -> 1.3e-8 with 2; len 65536 1.7e-8 and len 262144 1.0e-8 with 8).
    // Short contractions are latency-bound, the extra folds cost nothing there; at C4 (len >= 65536) folding every 8 stages
    // instead of 4 is worth 0 .. 2 %.
    if (storage == STORE_F32 && ns == NSPLIT_F16X2) v = f16_variant_by_length(len);
    if (want.set) v = want.v;
    if (want_k64.set && kt == 2) v = want_k64.v;                                   // only for k in (32, 64]
    if (storage == STORE_F32 && ns == 2 && v < 100) v = (kt == 2) ? 108 : 115;     // the 2-term forms exist only there
    if (ns != NSPLIT_F16X2 && is_f3_variant(v) && !kF3Variants[v - 100].bf) v = 108;          // the short-chain variants exist for the fp16 form only
    if (ns == NSPLIT_F16X2 && !(is_f3_variant(v) && kF3Variants[v - 100].f16)) v = 125;       // fp16 two-term form: the variants that won for the bf16 forms
    if (v >= 100 && storage == STORE_F32 && ns >= 2) {
        const int terms = pack_terms(ns);
        const auto fits = [=](int vv) { return is_f3_variant(vv) && f3_fits(kF3Variants[vv - 100], kt, terms); };
        if (!fits(v)) v = (ns == NSPLIT_F16X2) ? 125 : 108;
        if (!fits(v)) v = 115;
        if (!fits(v)) v = 110;
        return v;
    }
    if (v < 0 || v >= kNumVariants) v = 6;
    // variants that do not fit the 160 KiB LDS for this dtype / k fall back to variant 0
    const auto fits = [=](int vv) { return bp_fits(storage == STORE_BF16 ? 2 : 4, kt, ns, kVariants[vv]); };
    if (!fits(v)) v = (kt == 2) ? 11 : 0;
    if (!fits(v) && kt == 2) v = 13;
    if (!fits(v)) v = 0;
    if (!fits(v)) v = 7;
    return v;
}

// ---- what a launch can carry besides the product ----------------------------------------------------------------------------------
// the Gram inverse (InvRide): the accurate form, bigprod_kernel and bigprod_f3_kernel from the stored transpose
constexpr bool variant_rides(int storage, int nsplit, int variant, bool tr)
{
    if (nsplit == NSPLIT_F64) return !tr;                        // the accurate form (bigprod_f64_kernel at k > 2), either storage
    if (tr) return false;
    if (storage == STORE_BF16 || variant < 100) return true;     // bigprod_kernel (bf16 storage; fp32 storage in its older forms)
    if (storage != STORE_F32 || !is_f3_variant(variant)) return false;
    const F3Row& r = kF3Variants[variant - 100];                 // bigprod_f3_kernel, where the row is built for this form
    return r.kernel == F3 && (nsplit == NSPLIT_F16X2 ? r.f16 : (nsplit == 2 || nsplit == 3) && r.bf);
}
// the Gram reduction (TAIL = 1): the fold intervals 4 / 8 / 2 / 1 of the two-workgroup kernel, fp16 form, one k tile
constexpr bool variant_tails(int storage, int nsplit, int kt, int variant)
{
    return nsplit == NSPLIT_F16X2 && storage == STORE_F32 && kt == 1 && is_f3_variant(variant) && kF3Variants[variant - 100].tail;
}
// rows of the longest fp32 chain between two folds into fp64: bigprod_kernel flushes after every stage, the fp32-storage kernels fold
// every `fold` stages; the transposed source of bf16 storage always takes 64-column stages, whatever variant the plan names
constexpr int chain_rows(int storage, int variant, bool tr)
{
    const bool known = is_f3_variant(variant) || (variant >= 0 && variant < kNumVariants);
    if (!known) return 0;                                        // the accurate form (fp64 from the first product on), or no kernel at all
    if (tr && storage == STORE_BF16) return 64;
    return is_f3_variant(variant) ? kF3Variants[variant - 100].mb * kF3Variants[variant - 100].fold : kVariants[variant].mb;
}

// ---- the product form of a solver ("Precision design") ---------------------------------------------------------------------
// entries = m x n_global of A; col_spread_log2: log2 of the ratio of A's largest to its smallest column scale (matrix_measure_scale;
// read only where smk_solver_create measures it); small_accurate: SMK_BPP_SMALL_ACCURATE; nsplit_set: SMK_NSPLIT is present
constexpr int default_product_form(int algorithm, int k, int storage, bool sparse, int64_t entries, int col_spread_log2,
                                   bool small_accurate, bool nsplit_set)
{
    // fp32 A: the fp16 two-term form (3 MFMAs per product, 2^-22 operand error) unless SMK_NSPLIT picks the bf16 forms
    // (3 = bf16x3, 6 MFMAs, power-bound; 2 = two bf16 terms, 2^-16); bf16 A: three bf16 terms of the factor
    // HALS amplifies the product error several thousand times (its W update is a difference of nearly equal terms per
    // column, more so at high rank): the 24-bit bf16x3 operands stay inside the parity bar where the 22-bit fp16 ones
    // do not always (tools/fuzz_parity.py: k = 117 .. 253 1e-4 .. 5e-4 against < 1e-4, one k = 62 case at 1.1e-4 after
    // 17 iterations), so HALS keeps bf16x3; MU and BPP take the fp16 form
    // The amplification grows with the rank for every algorithm (BPP k = 191 after 34 iterations: 1.26e-4 with the
    // fp16 form), so above k = 64 the 24-bit operands are kept as well; C2 (k = 16) and C4 (k = 64) take the fp16 form.
    const bool hals = algorithm == ALG_HALS;
    int form = (storage == STORE_F32 && !hals && k <= 64) ? NSPLIT_F16X2 : 3;
    // HALS above k = 64: the 1e-8-class products of the 16-bit forms, amplified ~2x per five iterations at these ranks, leave
    // the 1e-4 parity bar in runs of 30+ iterations (1.4e-4 .. 1.6e-4 at k = 100 .. 150 after 30) -- with either 16-bit form
    // and with bf16 A alike, so it is the accumulation, not the operands.  Those runs take the ACCURATE form (NSPLIT_F64:
    // the stored A against the fp64 factor on the fp64 matrix cores), ~3x the product time.  SMK_NSPLIT=8 selects it anywhere.
    if (hals && k > 64 && !sparse) form = NSPLIT_F64;
    // Block pivoting above k = 64 as well: the Gram matrix of a uniform start has condition ~3k, so 1e-8-class products are
    // 2e-6 in the factors after ONE iteration at k = 100, and on data with sparse planted factors that grows ~1.3x per iteration
    // (tools/wide_long_run.py: 1200 x 1000, k = 100, bf16x3: 1.2e-4 after 20 iterations, 1.1e-3 after 30; k = 160: 4e-5 after 25;
    // the accurate form: 8.5e-12 after 30).  At k <= 64 the same data stays below 2e-5 over 30 iterations with the fp16 form.
    if (algorithm == ALG_BPP && k > 64 && !sparse) form = NSPLIT_F64;
    // ... and at k in (32, 64] where the accurate form costs nothing measurable (A of at most 2^24 entries: the streaming pass
    // is a 10 - 30 us launch next to a 100 us NNLS).  Block pivoting at these ranks amplifies the product error ~3000 x while
    // the passive sets are still moving: on data with sparse planted factors (1500 x 1100, k = 64) the distance to the oracle's
    // trajectory peaks at 0.4e-4 .. 2e-4 around iteration 100 with the fp16 form whatever its fold interval (3e-8 .. 9e-8
    // products), 5e-6 with bf16x3, 2e-12 with the accurate form, and contracts to 4e-7 by iteration 500
    // (profiles/r04_long_runs_500_iterations.txt).  Larger matrices keep the fp16 form (C4: 3 x the pass time otherwise);
    // SMK_NSPLIT=8 / 3 select the other forms anywhere.
    // (SMK_BPP_SMALL_ACCURATE=0 keeps the fp16 form: the test suite sets it, its small cases stand in for C4's path.)
    if (small_accurate && algorithm == ALG_BPP && k > 32 && !sparse && entries <= ((int64_t)1 << 24)) form = NSPLIT_F64;
    // Dense RANK2 (every node factorisation of HierNMF2 / flatclust on dense A runs 100 .. 1000 iterations to a tight
    // tolerance): the accurate form costs nothing at two factor rows -- bigprod_f64_k2_kernel does its 2 fp64 multiply-adds
    // per stored entry on the vector ALUs at the streaming rate -- and leaves only summation order between this path and
    // the reference's fp64 arithmetic (common/src/nmf.cpp:33).
    if (algorithm == ALG_RANK2 && !sparse) form = NSPLIT_F64;
    // Column scales of A more than 2^28 apart: the small columns fall below what fp32-class products resolve next to the
    // large ones (HALS / BPP leave the bar at 2^+-20, tests/test_gpu_parity.py) -- the accurate form as well.
    if (!nsplit_set && !sparse && algorithm != ALG_RANK2 && col_spread_log2 > 28) form = NSPLIT_F64;
    return form;
}
constexpr int resolve_product_form(int algorithm, int k, int storage, bool sparse, int64_t entries, int col_spread_log2,
                                   bool small_accurate, Want nsplit /* SMK_NSPLIT */)
{
    const int dflt = default_product_form(algorithm, k, storage, sparse, entries, col_spread_log2, small_accurate, nsplit.set);
    int form = nsplit.set ? nsplit.v : dflt;
    if (form != NSPLIT_F64 && (form < 1 || form > NSPLIT_F16X2)) form = dflt;
    if (form == NSPLIT_F64 && sparse) form = 3;       // sparse A: gather products in fp64 already
    // the fp16 two-term form applies to fp32 storage; RANK2 keeps its Gram matrices inside its own solve kernel
    if (form == NSPLIT_F16X2 && (storage != STORE_F32 || sparse || algorithm == ALG_RANK2)) form = 3;
    return form;
}

}  // namespace smk
