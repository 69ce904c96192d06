// smallk_amd/csrc/nnls.hip -- NnlsBlockpivot on the device (nnls.hpp:144-244, src/nnls.cpp:18-74,
// nmf_solver_bpp.hpp:146-219, normal_eq.hpp:27-54): the per-column masked Gauss-Jordan kernel and the
// inverse-based kernel for k in (32, 64].
#include "devutil.h"
#include "gram_inverse.h"
#include "nnls_masked.h"
#include "switches.h"

namespace smk {

// --------------------------------------------------------------------------
// Diagnostics (SMK_NNLS_STATS=1; tools/nnls_sets.py, smk_debug_nnls_stats): histograms of the work block pivoting does, kept in
// 256 device counters -- [0..15] exchanges per column (15 = 15 or more), [16..80] size t of the FIRST compact solve of a column
// (16 + t), [96..160] size of every later solve, [176] solves in the complement form, [177] in the direct form, [178] columns,
// [179] solves with every variable passive, [180] with none.  nullptr (the default) costs one uniform branch per column.
// --------------------------------------------------------------------------
unsigned long long* nnls_stats_ptr()
{
    static unsigned long long* buf = [] {
        unsigned long long* p = nullptr;
        if (sw::nnls_stats() && hipMalloc((void**)&p, 256 * sizeof(unsigned long long)) == hipSuccess) (void)hipMemset(p, 0, 256 * sizeof(unsigned long long));
        else p = nullptr;
        return p;
    }();
    return buf;
}
int nnls_stats_read(unsigned long long* out256, int reset)
{
    unsigned long long* p = nnls_stats_ptr();
    if (!p) return -1;
    if (hipDeviceSynchronize() != hipSuccess) return -2;
    if (out256 && hipMemcpy(out256, p, 256 * sizeof(unsigned long long), hipMemcpyDeviceToHost) != hipSuccess) return -2;
    if (reset) (void)hipMemset(p, 0, 256 * sizeof(unsigned long long));
    return 0;
}

// the masked elimination by itself (device code: nnls_masked.h)
// KP = 64: left alone the compiler takes 256 VGPRs + 40 AGPRs (one wave per SIMD) and every
// readlane -> FMA dependency is exposed; capping at 168 registers (3 waves per SIMD, 516 B of
// scratch per lane) is 1.45x faster on a 262144 x 8192 k = 64 BPP iteration.  No gain at KP <= 32.
template <int KP>
__global__ __launch_bounds__(256, (KP == 64 ? 3 : 1)) void nnls_bpp_kernel(double* __restrict__ X, double* __restrict__ Y, int k, i64 N,
                                                       PartialView R, const double* __restrict__ G,
                                                       int* __restrict__ fail_flag, int iter_tag, i64 col_begin,
                                                       const int* __restrict__ skip_if, double* __restrict__ Gp, NnlsPack pk,
                                                       unsigned long long* __restrict__ stats, NnlsRiders rd = NnlsRiders())
{
    if (skip_if && *skip_if != 0) return;           // the inverse-based kernel took this launch
    nnls_bpp_body<KP>(X, Y, k, N, R, G, fail_flag, iter_tag, col_begin, Gp, pk, stats, rd);
}

// --------------------------------------------------------------------------
// k in (32, 64]: block principal pivoting through the INVERSE of the Gram matrix.
//
// On noise-like data every column has its own passive set F (|F| ~ 45-58 of 64, 8192 distinct sets in
// 8192 columns) and needs ~2 solves, so neither the reference's "all passive" shortcut nor its grouping
// by identical sets (nmf_solver_bpp.hpp:29-142) ever fires; a factorisation per column and pivot of the
// |F| x |F| system costs O(k^3).  With Ginv = G^-1 (one 64 x 64 inversion per launch) and v = Ginv r:
//     Z = complement of F,  S = Ginv[Z,Z]:   y_Z = -S^-1 v_Z,   x = v + Ginv[:,Z] y_Z   (x_Z = 0, y_F = 0)
// (block elimination on G x = r + y), i.e. one |Z| x |Z| solve plus |Z| rank-one terms -- and both x and
// the dual y come out of it.  When |F| < |Z| the direct form G[F,F] x_F = r_F, y = G[:,F] x_F - r is
// cheaper; both are the same "compact solve + accumulate" on (M, T, s) = (Ginv, Z, -v) or (G, F, r) with
// t = min(|F|, |Z|) <= 32 rows in the first t lanes of the wave.  One wave per column; the set is
// wave-uniform, so index lists, loop bounds and pivot broadcasts are scalar.
// The inverse is taken only when every Gauss-Jordan pivot of G is positive and not tiny (gram_inverse64_kernel
// sets status = 1); otherwise nnls_bpp_kernel<64> above runs and reproduces the reference's non-SPD failure.
// --------------------------------------------------------------------------
// Ginv = G^-1 (k x k live, KP x KP storage, pads zero) by in-place Gauss-Jordan, one workgroup of 256 threads.
// status = 1 when every pivot p_j satisfies p_j > 1e-9 * G[j][j] (SPD and usable), else 0.
// (the elimination itself: gram_inverse.h -- it also rides in the sparse product launch)
template <int KP>
__global__ __launch_bounds__(256) void gram_inverse64_kernel(const double* __restrict__ G, int k, double* __restrict__ Ginv,
                                                             int* __restrict__ status)
{
    __shared__ __attribute__((aligned(16))) double lds[GRAM_INVERSE_LDS(KP)];
    gram_inverse64_body<KP>(G, k, Ginv, status, lds);
}

template <int KP, int NT, int WPS>
__global__ __launch_bounds__(NT, WPS) void nnls_bpp_inv_kernel(double* __restrict__ X, double* __restrict__ Y, int k, i64 N,
                                                          PartialView R, const double* __restrict__ G,
                                                          const double* __restrict__ Ginv,
                                                          const int* __restrict__ status,
                                                          int* __restrict__ fail_flag, int iter_tag, i64 col_begin,
                                                          unsigned long long* __restrict__ stats,
                                                          const unsigned* __restrict__ worklist)
{
    static_assert(KP == 64 || KP == 32, "one wave per column, one lane per component");
    constexpr int NW = NT / 64;
    if (*status == 0) return;
    // worklist != nullptr: only the columns of a work list (worklist[0] of them, col_begin + worklist[1 + i]); the count is read
    // before the matrices are copied.  Its one producer, the four-columns-per-wave kernel at KP = 64, was removed after 97e83fd
    // and launch_nnls_bpp passes nullptr.  The walk through the list stays on purpose: with the plain column walk in its place
    // the KP = 64 instance goes from 127 to 128 VGPRs and from 148 to 156 bytes of scratch per lane, and its launches measure
    // 2 - 10 % longer (16384 x 8192, k = 64: 2.07 -> 2.14 ms over twelve iterations; profiles/variant_cut_ab.txt)
    const i64 nwork = worklist ? (i64)worklist[0] : 0;
    if (worklist && (i64)blockIdx.x * NW >= nwork) return;
    extern __shared__ __attribute__((aligned(16))) double lds[];
    double* gs = lds;                               // gs[c*KP + i]  = G[i][c]
    double* gis = lds + KP * KP;                    // gis[c*KP + i] = Ginv[i][c]
    for (int t = threadIdx.x; t < KP * KP; t += NT) { gs[t] = G[t]; gis[t] = Ginv[t]; }
    const int lane = threadIdx.x & 63;
    // KP = 32 (k in (16, 32], round 4): the upper half of the wave has no component; it runs along masked (comp_ok, the set
    // masks) and reads the matrices at ln = lane mod KP so that it stays inside them
    const int ln = lane & (KP - 1);
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    double* sv = lds + 2 * KP * KP + wave * 128;               // wave-private: 64 doubles of values
    int* sidx = (int*)(sv + 64);                               //               64 ints of indices
    __syncthreads();

    const unsigned long long kmask = (k >= 64) ? ~0ull : ((1ull << k) - 1ull);
    const bool comp_ok = lane < k;
    const int max_iter = 5 * k;
    int failed_any = 0;

    // A wave works through its columns one after the other, and a column is load -> ~0.3 us of arithmetic -> store: without
    // the loads of column c + 1 in flight during the arithmetic of column c every column costs a round trip to memory on top
    // (1 M columns at k = 32, 256 columns per wave: 1.19 ms per launch, 4.6 us per column and wave, of which the arithmetic
    // is a tenth; profiles/r05_s_1m_kernel_stats.md).  The right-hand side and the start of the NEXT column are requested
    // before the current one is touched.
    // positions idx walk the columns [col_begin, N) or the work list
    const i64 col_stride = (i64)gridDim.x * NW;
    const i64 nidx = worklist ? nwork : (N - col_begin);
    auto col_of = [&](i64 idx) -> i64 { return col_begin + (worklist ? (i64)worklist[1 + idx] : idx); };
    i64 idx = (i64)blockIdx.x * NW + wave;
    RhsPending rq;
    rq.t[0] = rq.t[1] = rq.t[2] = rq.t[3] = rq.tail = 0.0;
    double x_next = 0.0;
    i64 col_nx = idx < nidx ? col_of(idx) : 0;
    if (idx < nidx && comp_ok) {
        rhs_issue(R, col_nx, lane, rq);
        x_next = X[col_nx * KP + lane];
    }
    for (; idx < nidx; idx += col_stride) {
        const i64 col = col_nx;
        double rhs = comp_ok ? rhs_finish(R, rq) : 0.0, x = x_next, y = 0.0;
        if (idx + col_stride < nidx) {
            col_nx = col_of(idx + col_stride);
            if (comp_ok) {
                rhs_issue(R, col_nx, lane, rq);
                x_next = X[col_nx * KP + lane];
            }
        }
        unsigned long long F = __ballot(comp_ok && x > 0.0) & kmask;       // passive_set = (X > 0), nnls.hpp:157

        // v = Ginv r, the unconstrained solution: needed by the complement form only (and when every variable is passive).
        // A column whose passive sets stay small -- sparse factors: a document in two or three topics, a node in one community
        // -- never takes that form, and the KP-step product was a third of its time (s_1m: 1.19 ms per launch of 1 M columns,
        // profiles/r05_s_1m_kernel_stats.md), so it is computed when the first solve of the column asks for it.
        double v = 0.0;
        bool have_v = false;
        auto need_v = [&]() {
            if (have_v) return;
            have_v = true;
            sv[lane] = rhs;
            double v0 = 0.0, v1 = 0.0;
#pragma unroll 8
            for (int c = 0; c < KP; c += 2) {
                const f64x2_t rr = *(const f64x2_t*)(sv + c);              // broadcast read
                v0 = __builtin_fma(gis[c * KP + ln], rr[0], v0);
                v1 = __builtin_fma(gis[(c + 1) * KP + ln], rr[1], v1);
            }
            v = v0 + v1;
        };

        int failed = 0;
        int nsolve = 0;                                                     // diagnostics only
        // compact solve of M[T,T] u = s_T on the first TB lanes (rows >= t are identity rows), then
        // out = base + M[:,T] u.  TB is a compile-time bound: no branch inside the elimination.
        auto compact = [&](auto tb_tag, const double* M, int t, int tl, double sc, double base, double& u_out) -> double {
            constexpr int TB = decltype(tb_tag)::value;
            const bool live = lane < t;
            double a[TB];
#pragma unroll
            for (int b = 0; b < TB; ++b) {
                const int tb = __builtin_amdgcn_readlane(tl, b);           // lanes >= t carry tl = 0: harmless
                const double mv = M[tb * KP + tl];
                a[b] = (live && b < t) ? mv : ((b == lane) ? 1.0 : 0.0);
            }
            double d = 1.0;
#pragma unroll
            for (int j = 0; j < TB; ++j) {
                const double piv = readlane_f64(a[j], j);
                if (!(piv > 0.0)) failed = 1;
                const double ip = fast_rcp(piv);
                if (lane == j) d = a[j];
                const double f = (lane == j) ? 0.0 : a[j] * ip;
#pragma unroll
                for (int c = j + 1; c < TB; ++c) a[c] = __builtin_fma(-f, readlane_f64(a[c], j), a[c]);
                sc = __builtin_fma(-f, readlane_f64(sc, j), sc);
            }
            const double u = live ? sc * fast_rcp(d) : 0.0;
            double out = base;
#pragma unroll
            for (int b = 0; b < TB; ++b) {
                const int tb = __builtin_amdgcn_readlane(tl, b);
                out = __builtin_fma(M[tb * KP + ln], readlane_f64(u, b), out);       // u = 0 beyond t
            }
            u_out = u;
            return out;
        };
        // one block-pivot solve for the passive set Fs: leaves x (zero outside Fs) and y (zero inside Fs)
        auto solve = [&](unsigned long long Fs) {
            const unsigned long long Zs = ~Fs & kmask;
            const int p = __popcll(Fs), q = __popcll(Zs);
            const bool inF = (Fs >> lane) & 1ull;
            if (stats && lane == 0) {
                const int tt = q <= p ? q : p;
                nnls_stat(stats, (nsolve == 0 ? 16 : 96) + tt);
                nnls_stat(stats, q == 0 ? 179 : p == 0 ? 180 : q <= p ? 176 : 177);
            }
            ++nsolve;
            if (q == 0) { need_v(); x = v; y = 0.0; return; }
            if (p == 0) { x = 0.0; y = comp_ok ? -rhs : 0.0; return; }
            const bool comp = q <= p;                                       // complement form on Ginv
            if (comp) need_v();
            const unsigned long long T = comp ? Zs : Fs;
            const int t = comp ? q : p;
            const double* M = comp ? gis : gs;
            const bool inT = (T >> lane) & 1ull;
            // compact index list: lane l < t gets the l-th member of T
            const int rank = __popcll(T & ((1ull << lane) - 1ull));
            if (inT) sidx[rank] = lane;
            sv[lane] = comp ? -v : rhs;
            const int tl = (lane < t) ? sidx[lane] : 0;
            const double sc = (lane < t) ? sv[tl] : 0.0;
            const double base = comp ? v : -rhs;
            double u = 0.0, out;
            // the elimination costs ~TB^2 / 2 broadcast + FMA pairs: bounds in steps of 4 waste a quarter less
            // than steps of 8 on the |Z| = 6 .. 20 of noise-like data
            if (t <= 4) out = compact(std::integral_constant<int, 4>{}, M, t, tl, sc, base, u);
            else if (t <= 8) out = compact(std::integral_constant<int, 8>{}, M, t, tl, sc, base, u);
            else if (t <= 12) out = compact(std::integral_constant<int, 12>{}, M, t, tl, sc, base, u);
            else if (t <= 16) out = compact(std::integral_constant<int, 16>{}, M, t, tl, sc, base, u);
            else if (t <= 20) out = compact(std::integral_constant<int, 20>{}, M, t, tl, sc, base, u);
            else if (t <= 24) out = compact(std::integral_constant<int, 24>{}, M, t, tl, sc, base, u);
            else if (t <= 28) out = compact(std::integral_constant<int, 28>{}, M, t, tl, sc, base, u);
            else out = compact(std::integral_constant<int, 32>{}, M, t, tl, sc, base, u);
            // u back to component positions
            if (lane < t) sv[tl] = u;
            const double ut = inT ? sv[lane] : 0.0;
            if (comp) { x = inF ? out : 0.0; y = ut; }
            else      { x = ut; y = (comp_ok && !inF) ? out : 0.0; }
        };

        solve(F);
        bool passive = (F >> lane) & 1ull;
        unsigned long long nonopt = __ballot(comp_ok && !passive && (y < 0.0));
        unsigned long long infeas = __ballot(comp_ok && passive && (x < 0.0));
        int ng = __popcll(nonopt) + __popcll(infeas);
        int Pc = 3, Ninf = k + 1;                    // PBAR = 3, nnls.hpp:152,170
        int iter = 0;
        while (ng > 0) {                             // uniform
            if (iter >= max_iter) { failed = 1; break; }
            // UpdatePassiveSet, src/nnls.cpp:18-74
            if (ng < Ninf) { Pc = 3; Ninf = ng; F = (F | nonopt) & ~infeas; }
            else if (Pc >= 1) { Pc -= 1; F = (F | nonopt) & ~infeas; }
            else {
                const int r1 = nonopt ? (63 - __clzll(nonopt)) : 0;
                const int r2 = infeas ? (63 - __clzll(infeas)) : 0;
                F ^= (1ull << (r1 > r2 ? r1 : r2));
            }
            F &= kmask;
            passive = (F >> lane) & 1ull;
            solve(F);
            if (fabs(x) < 1.0e-12) x = 0.0;          // ZeroizeSmallValues, nnls.hpp:213,224
            if (fabs(y) < 1.0e-12) y = 0.0;          // :225
            nonopt = __ballot(comp_ok && !passive && (y < 0.0));
            infeas = __ballot(comp_ok && passive && (x < 0.0));
            ng = __popcll(nonopt) + __popcll(infeas);
            ++iter;
        }
        if (fabs(x) < 1.0e-12) x = 0.0;              // columns that never pivot are zeroized too (nnls_bpp_kernel's note)
        if (fabs(y) < 1.0e-12) y = 0.0;
        if (comp_ok) {
            X[col * KP + lane] = x;
            if (Y) Y[col * KP + lane] = y;
        }
        if (stats && lane == 0) { nnls_stat(stats, iter < 15 ? iter : 15); nnls_stat(stats, 178); }
        failed_any |= failed;
    }
    if (failed_any && lane == 0) atomicMin(fail_flag, iter_tag);
}

bool nnls_uses_tiles(int k)
{
    // from k = 65 (measured on 16384 x 8192, 12 iterations: k = 80 / 100 / 128 took 3.96 / 4.53 / 5.27 ms per iteration on the
    // two-components-per-lane kernel that served k in (64, 128] before, 2.39 / 2.84 / 3.12 ms on the tile kernel)
    return k > 64;
}

size_t nnls_scratch_elems(int k) { return (size_t)kp_of(k) * kp_of(k) + 8; }     // k <= 64; above: nnls_wide_scratch_elems
// k in (16, 32] also solves through the inverse of the Gram matrix (round 4; SMK_NNLS_INV32=0: the masked elimination, as before)
// Workgroups of the inverse-based kernels = resident workgroups x rounds.  Every workgroup first copies G and Ginv into LDS (16 /
// 64 KB) and a wave prefetches its next column, so few columns per wave waste both: one round up to 65536 columns (s_reuters 159 ->
// 154 us per iteration, 32768 x 8192 at k = 32 466 -> 453), four above, where more workgroups in flight hide more latency (10^6
// columns: 3.39 against 3.56 ms per iteration; C4 whole: no difference).  SMK_NNLS_ROUNDS overrides.
static inline int nnls_rounds(i64 ncols)
{
    const int forced = sw::nnls_rounds();
    return forced > 0 ? forced : (ncols <= 65536 ? 1 : 4);
}

bool nnls_inverse_at_32()
{
    return sw::nnls_inv32();
}

// k in (16, 64]: Ginv and the path selector into `scratch` (nnls_scratch_elems(k) doubles).  One workgroup, ~0.05 ms: the
// solver runs it on a side stream beside the streaming product that separates the Gram matrix from its NNLS.
int launch_gram_inverse(const double* G, int k, double* scratch, hipStream_t st)
{
    const int KPv = kp_of(k);
    if ((KPv != 32 && KPv != 64) || !scratch) return 0;
    if (KPv == 32 && !nnls_inverse_at_32()) return 0;
    if (KPv == 32) gram_inverse64_kernel<32><<<1, 256, 0, st>>>(G, k, scratch, (int*)(scratch + 32 * 32));
    else gram_inverse64_kernel<64><<<1, 256, 0, st>>>(G, k, scratch, (int*)(scratch + 64 * 64));
    SMK_HIP(hipGetLastError());
    return 0;
}

// solves columns [col_begin, col_end) of X (col_end <= N); other columns are untouched.
// `scratch`: nnls_scratch_elems(k) doubles (the inverse of G and the path selector for k > 16);
// inverse_ready != 0: launch_gram_inverse(G, ...) has already been ordered before this call.
int launch_nnls_bpp(double* X, double* Y, int k, i64 col_begin, i64 col_end, PartialView R, const double* G,
                    int* fail_flag, int iter_tag, double* scratch, int inverse_ready, int num_cus, hipStream_t st,
                    double* gram_partials, int* gram_nblk, const NnlsPack* pack, const NnlsRiders* riders)
{
    if (gram_nblk) *gram_nblk = 0;
    if (riders && riders->pg_nblk) *riders->pg_nblk = 0;
    if (nnls_uses_tiles(k)) return launch_nnls_bpp_wide(X, Y, k, col_begin, col_end, R, G, fail_flag, iter_tag, scratch, inverse_ready, num_cus, st);
    const int KPv = kp_of(k);
    const int gpb = 256 / KPv;
    const i64 ncols = col_end - col_begin;
    if (ncols <= 0) return 0;
    const int grid = (int)((ncols + gpb - 1) / gpb);
    const i64 N = col_end;
    const int inv_mode = sw::nnls_inv();
    const int* skip_if = nullptr;
    if (KPv == 32 && inv_mode && scratch && nnls_inverse_at_32()) {
        // k in (16, 32]: the same kernel, one wave per column with its upper half idle.  The masked elimination costs a full
        // 32-step Gauss-Jordan per exchange and column (99 us per launch on 8192 x 4096 at k = 32, two thirds of the iteration);
        // through the inverse an exchange is a t x t solve with t <= 16 (profiles/r04_gram_inverse.txt)
        double* Ginv = scratch;
        int* status = (int*)(scratch + 32 * 32);
        if (!inverse_ready) { int irc = launch_gram_inverse(G, k, scratch, st); if (irc) return irc; }
        constexpr int NT = 512;
        const int lds = (2 * 32 * 32 + (NT / 64) * 128) * (int)sizeof(double);
        i64 g2 = (ncols + NT / 64 - 1) / (NT / 64);
        const i64 cap = (i64)num_cus * 2 * nnls_rounds(ncols);
        if (g2 > cap) g2 = cap;
        // round 6: four columns per wave (nnls_g16.hip), a launch that solves by masked elimination itself when the inverse was
        // rejected; SMK_NNLS_G16=0 keeps the wave-per-column kernel
        const int g16 = launch_nnls_bpp_g16(X, Y, k, col_begin, col_end, R, G, Ginv, status, fail_flag, iter_tag, num_cus, st, nnls_stats_ptr());
        if (g16 != 0) return g16 < 0 ? g16 : 0;
        nnls_bpp_inv_kernel<32, 512, 4><<<(unsigned)g2, NT, lds, st>>>(X, Y, k, N, R, G, Ginv, status, fail_flag, iter_tag, col_begin, nnls_stats_ptr(), nullptr);
        SMK_HIP(hipGetLastError());
        skip_if = status;
    }
    if (KPv == 64 && inv_mode && scratch) {
        double* Ginv = scratch;
        int* status = (int*)(scratch + 64 * 64);
        if (!inverse_ready) { int irc = launch_gram_inverse(G, k, scratch, st); if (irc) return irc; }
        constexpr int NT = 512;
        const int lds = (2 * 64 * 64 + (NT / 64) * 128) * (int)sizeof(double);
        SMK_HIP(hipFuncSetAttribute((const void*)nnls_bpp_inv_kernel<64, 512, 4>, hipFuncAttributeMaxDynamicSharedMemorySize, lds));
        i64 g2 = (ncols + NT / 64 - 1) / (NT / 64);
        const i64 cap = (i64)num_cus * 2 * nnls_rounds(ncols);
        if (g2 > cap) g2 = cap;
        nnls_bpp_inv_kernel<64, 512, 4><<<(unsigned)g2, NT, lds, st>>>(X, Y, k, N, R, G, Ginv, status, fail_flag, iter_tag, col_begin, nnls_stats_ptr(), nullptr);
        SMK_HIP(hipGetLastError());
        skip_if = status;
    }
    int grid1 = grid;
    // the fallback behind the inverse-based kernel almost always exits on its first load: two workgroups per CU (6.1 -> ~3 us
    // of launch at 1500 workgroups, profiles/r05_s_reuters_kernel_stats.md) and more trips on the rare launch that does run
    if (skip_if && grid1 > num_cus * 2) grid1 = num_cus * 2;
    // KP = 16, all columns, at most NNLS_GRAM_MAX workgroups: the launch also leaves the Gram partials of the solved factor
    double* gp = nullptr;
    if (gram_partials && gram_nblk && KPv == 16 && col_begin == 0 && grid1 == grid && grid <= NNLS_GRAM_MAX) { gp = gram_partials; *gram_nblk = grid; }
    NnlsPack pk;                                           // only together with the Gram partials (one trip per workgroup, all columns)
    if (pack && gp) pk = *pack;
    NnlsRiders rd;                                         // only the launch that solves by itself (k <= 16) carries them
    if (riders && !skip_if && KPv <= 16) {
        rd = *riders;
        if (rd.pg_nblk) *rd.pg_nblk = rd.pg_part ? grid1 : 0;
    }
    KP_DISPATCH(KPv, (nnls_bpp_kernel<KP><<<grid1, 256, 0, st>>>(X, Y, k, N, R, G, fail_flag, iter_tag, col_begin, skip_if, gp, pk, skip_if ? nullptr : nnls_stats_ptr(), rd)));
    SMK_HIP(hipGetLastError());
    return 0;
}

}  // namespace smk
