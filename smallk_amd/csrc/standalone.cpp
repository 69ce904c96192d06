// smallk_amd/csrc/standalone.cpp -- the two entries of the C ABI that use the solver's kernels and own no handle state: one
// block-pivoting solve on host arrays (smk_nnls_blockpivot) and the single-process driver of a column-sharded factorisation
// (smk_nmf_dense_sharded: one host thread, one device context and one solver handle per shard, through the public entries).
#include "state.h"
#include "entry.h"
#include "comm.h"

#include <algorithm>
#include <climits>
#include <cstdio>
#include <string>
#include <thread>
#include <vector>

extern "C" {

// NnlsBlockpivot(LHS, RHS, X, Y), common/include/nnls.hpp:144-244, on its own: min ||.|| s.t. X >= 0 for
// LHS X = RHS with LHS k x k SPD, warm start X (passive set = X > 0), dual Y = LHS X - RHS.
int smk_nnls_blockpivot(int k, int64_t ncols, const double* LHS, int64_t ldL, const double* RHS, int64_t ldR, double* X,
                        int64_t ldX, double* Y, int64_t ldY)
{
    if (int rc = require_init()) return rc;
    if (k <= 0 || ncols <= 0 || !LHS || !RHS || !X || ldL < k || ldR < k || ldX < k || (Y && ldY < k)) return SMK_BAD_PARAM;
    if (k > MAX_K_BPP) { set_error("device path supports k <= 2048"); return SMK_UNSUPPORTED; }
    const int KP = kp_of(k);
    std::vector<double> hg((size_t)KP * KP, 0.0), hr((size_t)KP * ncols, 0.0), hx((size_t)KP * ncols, 0.0);
    for (int c = 0; c < k; ++c)
        for (int r = 0; r < k; ++r) hg[(size_t)c * KP + r] = LHS[(size_t)c * ldL + r];
    for (int64_t c = 0; c < ncols; ++c)
        for (int r = 0; r < k; ++r) {
            hr[(size_t)c * KP + r] = RHS[(size_t)c * ldR + r];
            hx[(size_t)c * KP + r] = X[(size_t)c * ldX + r];
        }
    Scratch<double> dg, dr, dx, dy, dscratch;
    Scratch<int> dflag;
    int rc = dg.alloc(hg.size());
    rc |= dr.alloc(hr.size());
    rc |= dx.alloc(hx.size());
    rc |= dy.alloc(hx.size());
    rc |= dscratch.alloc(nnls_uses_tiles(k) ? nnls_wide_scratch_elems(k, ctx().cus, ncols) : nnls_scratch_elems(k));
    rc |= dflag.alloc(1);
    if (rc) return SMK_DEVICE_ERROR;
    const int big = INT_MAX;
    SMK_HIP(hipMemcpyAsync(dg, hg.data(), hg.size() * sizeof(double), hipMemcpyHostToDevice, ctx().stream));
    SMK_HIP(hipMemcpyAsync(dr, hr.data(), hr.size() * sizeof(double), hipMemcpyHostToDevice, ctx().stream));
    SMK_HIP(hipMemcpyAsync(dx, hx.data(), hx.size() * sizeof(double), hipMemcpyHostToDevice, ctx().stream));
    SMK_HIP(hipMemsetAsync(dy, 0, hx.size() * sizeof(double), ctx().stream));
    SMK_HIP(hipMemcpyAsync(dflag, &big, sizeof(int), hipMemcpyHostToDevice, ctx().stream));
    const PartialView pv{dr, 1, 0, KP, 1};
    rc = launch_nnls_bpp(dx, dy, k, 0, ncols, pv, dg, dflag, 0, dscratch, 0, ctx().cus, ctx().stream);
    if (rc) return rc;
    int flag = INT_MAX;
    SMK_HIP(hipMemcpyAsync(hx.data(), dx, hx.size() * sizeof(double), hipMemcpyDeviceToHost, ctx().stream));
    SMK_HIP(hipMemcpyAsync(hr.data(), dy, hx.size() * sizeof(double), hipMemcpyDeviceToHost, ctx().stream));
    SMK_HIP(hipMemcpyAsync(&flag, dflag, sizeof(int), hipMemcpyDeviceToHost, ctx().stream));
    SMK_HIP(hipStreamSynchronize(ctx().stream));
    for (int64_t c = 0; c < ncols; ++c)
        for (int r = 0; r < k; ++r) {
            X[(size_t)c * ldX + r] = hx[(size_t)c * KP + r];
            if (Y) Y[(size_t)c * ldY + r] = hr[(size_t)c * KP + r];
        }
    return flag == INT_MAX ? SMK_OK : SMK_FAILURE;
}

// Result Nmf(...) on `nshards` column shards of A, one host thread + one HIP device per shard: A and H
// column-sharded, W replicated, RCCL collectives issued from C on each shard's streams.  `devices` NULL: shard r on
// device r.  local_stub != 0: every shard on the CURRENT device with the in-process stand-in for RCCL (which refuses
// two ranks on one device) -- for boxes with fewer GPUs than shards, and for the tests.
int smk_nmf_dense_sharded(const smk_options* opts, const double* A, int64_t ldA, double* W, int64_t ldW, double* H,
                          int64_t ldH, smk_stats* stats, int storage, int nshards, const int* devices, int local_stub)
{
    if (!ctx().init) {
        fprintf(stderr, "nmflib error: nmf_initialize() must be called prior to any factorization routine\n\n");
        return SMK_NOTINITIALIZED;
    }
    if (!opts || !smk_is_valid(opts, 1)) return SMK_BAD_PARAM;
    if (!A || !W || !H || nshards < 1 || nshards > 16) return SMK_BAD_PARAM;
    if (opts->k > MAX_K || (opts->algorithm == SMK_ALG_BPP && opts->k > MAX_K_BPP)) { set_error("device path supports k <= 2048"); return SMK_UNSUPPORTED; }
    const int64_t m = opts->height, n = opts->width;
    if (ldA < m || ldW < m || ldH < opts->k) { set_error("leading dimension too small"); return SMK_BAD_PARAM; }
    if (nshards > n) nshards = (int)n;
    if (nshards == 1) return smk_nmf_dense(opts, A, ldA, W, ldW, H, ldH, stats, storage);
    int dev0 = 0;
    SMK_HIP(hipGetDevice(&dev0));
    if (!local_stub) {
        int ndev = 0;
        SMK_HIP(hipGetDeviceCount(&ndev));
        for (int r = 0; r < nshards; ++r)
            if ((devices ? devices[r] : r) >= ndev) { set_error("smk_nmf_dense_sharded: not enough devices for the shards"); return SMK_BAD_PARAM; }
    }
    std::vector<smk_comm*> comms((size_t)nshards, nullptr);
    std::vector<int> devs((size_t)nshards);
    for (int r = 0; r < nshards; ++r) devs[(size_t)r] = local_stub ? dev0 : (devices ? devices[r] : r);
    int rc = local_stub ? smk_comm_init_local(comms.data(), nshards) : smk_comm_init_all(comms.data(), nshards, devs.data());
    if (rc != SMK_OK) return rc;

    std::vector<int> rcs((size_t)nshards, SMK_OK);
    std::vector<smk_stats> sts((size_t)nshards, smk_stats{0, 0});
    std::vector<std::string> errs((size_t)nshards);
    std::vector<double> Wcopy((size_t)m * opts->k);          // every shard starts from the same W0
    for (int c = 0; c < opts->k; ++c) std::copy(W + (size_t)c * ldW, W + (size_t)c * ldW + m, Wcopy.begin() + (size_t)c * m);
    auto worker = [&](int r) {
        DeviceCtx local;
        t_ctx = &local;
        int wrc = SMK_OK;
        smk_matrix* a = nullptr;
        smk_solver* s = nullptr;
        const int64_t base = n / nshards, extra = n % nshards;
        const int64_t c0 = r * base + std::min<int64_t>(r, extra), nc = base + (r < extra ? 1 : 0);
        wrc = smk_initialize(devs[(size_t)r]);
        if (wrc == SMK_OK) wrc = smk_matrix_create(&a, m, n, c0, nc, storage);
        if (wrc == SMK_OK) wrc = smk_matrix_upload_f64(a, A + (size_t)c0 * ldA, ldA);
        if (wrc == SMK_OK) wrc = smk_solver_create(&s, opts, a);
        if (wrc == SMK_OK) wrc = smk_solver_attach_comm(s, comms[(size_t)r]);
        if (wrc == SMK_OK) wrc = smk_solver_set_factors(s, Wcopy.data(), m, H + (size_t)c0 * ldH, ldH);
        // a shard that failed before the first collective would strand the others: agree on the setup first
        {
            double ok = (wrc == SMK_OK) ? 0.0 : 1.0;
            Scratch<double> dflag;
            if (smk::dev_malloc(dflag.put(), sizeof(double)) == hipSuccess) {
                (void)hipMemcpy(dflag, &ok, sizeof(double), hipMemcpyHostToDevice);
                (void)comm_allreduce(comms[(size_t)r], dflag, 1, 1, ctx().stream);
                (void)hipStreamSynchronize(ctx().stream);
                (void)hipMemcpy(&ok, dflag, sizeof(double), hipMemcpyDeviceToHost);
            }
            if (ok != 0.0 && wrc == SMK_OK) wrc = SMK_FAILURE;
        }
        if (wrc == SMK_OK) {
            wrc = smk_solver_run(s, &sts[(size_t)r]);
            // anything but an agreed result (OK / FAILURE are all-reduced) means this rank left the loop alone: release the
            // peers that wait for it in a collective
            if (wrc != SMK_OK && wrc != SMK_FAILURE) smk_comm_abort(comms[(size_t)r]);
            if (wrc == SMK_OK || wrc == SMK_FAILURE) {
                // W is replicated: rank 0 returns it; every rank returns its own columns of H
                std::vector<double> Wl(r == 0 ? 0 : (size_t)m * opts->k);
                (void)smk_solver_get_factors(s, 0, r == 0 ? W : Wl.data(), r == 0 ? ldW : m, H + (size_t)c0 * ldH, ldH);
            }
        }
        errs[(size_t)r] = smk_last_error();
        smk_solver_destroy(s);
        smk_matrix_destroy(a);
        smk_finalize();
        rcs[(size_t)r] = wrc;
        t_ctx = nullptr;
    };
    std::vector<std::thread> th;
    for (int r = 0; r < nshards; ++r) th.emplace_back(worker, r);
    for (auto& t : th) t.join();
    for (smk_comm* c : comms) smk_comm_destroy(c);
    (void)hipSetDevice(dev0);
    int result = SMK_OK;
    for (int r = 0; r < nshards; ++r)
        if (rcs[(size_t)r] != SMK_OK && result == SMK_OK) { result = rcs[(size_t)r]; set_error(errs[(size_t)r]); }
    if (stats) *stats = sts[0];
    return result;
}

}  // extern "C"
