// smallk_amd/csrc/context.cpp -- the device context of the calling thread (device, stream, CU count, live handles),
// the registry of resident matrices that follow its stream, and the smk_initialize ... smk_set_stream entry points.
#include "state.h"

#include <algorithm>
#include <mutex>

namespace smk {

DeviceCtx g_ctx;
__thread DeviceCtx* t_ctx = nullptr;

// The registries of all contexts share one lock: a matrix may be destroyed from another thread than the one that created
// it (Python's collector, the workers of smk_nmf_dense_sharded), and it leaves the registry of the context that OWNS it.
static std::mutex g_mats_mu;
void repoint_matrices(hipStream_t st)
{
    std::lock_guard<std::mutex> lk(g_mats_mu);
    for (smk_matrix* a : ctx().mats) a->st = st;
}
// the context goes away: its matrices stay alive without an owner (they take the next context's stream)
void orphan_matrices()
{
    std::lock_guard<std::mutex> lk(g_mats_mu);
    for (smk_matrix* a : ctx().mats) { a->st = nullptr; a->owner = nullptr; }
    ctx().mats.clear();
}
void register_matrix(smk_matrix* a)
{
    std::lock_guard<std::mutex> lk(g_mats_mu);
    a->owner = &ctx();
    a->owner->mats.push_back(a);
}
void unregister_matrix(smk_matrix* a)
{
    std::lock_guard<std::mutex> lk(g_mats_mu);
    if (!a->owner) return;
    auto& v = a->owner->mats;
    v.erase(std::remove(v.begin(), v.end(), a), v.end());
    a->owner = nullptr;
}

hipStream_t context_stream(bool* initialized)
{
    if (initialized) *initialized = ctx().init;
    return ctx().stream;
}

}  // namespace smk

extern "C" {

int smk_initialize(int device_ordinal)
{
    if (device_ordinal >= 0) SMK_HIP(hipSetDevice(device_ordinal));
    int dev = 0;
    SMK_HIP(hipGetDevice(&dev));
    hipDeviceProp_t prop;
    SMK_HIP(hipGetDeviceProperties(&prop, dev));
    ctx().cus = prop.multiProcessorCount > 0 ? prop.multiProcessorCount : 256;
    if (!ctx().stream) {
        SMK_HIP(hipStreamCreateWithFlags(&ctx().stream, hipStreamNonBlocking));
        ctx().own_stream = true;
    }
    ctx().init = true;
    return SMK_OK;
}

int smk_is_initialized(void) { return ctx().init ? SMK_INITIALIZED : SMK_NOTINITIALIZED; }

void smk_finalize(void)
{
    if (ctx().stream) (void)hipStreamSynchronize(ctx().stream);
    if (ctx().own_stream && ctx().stream) (void)hipStreamDestroy(ctx().stream);
    orphan_matrices();                    // a matrix that outlives the context takes the next context's stream
    dev_trim();                           // cached device blocks of this device go back to the runtime
    ctx().stream = nullptr;
    ctx().own_stream = false;
    ctx().init = false;
}

// A host thread that drives a device of its own (the second device of a two-device HierNMF2 run, hierclust.cpp): its
// library state -- stream, CU count, live handles -- is separate from the process-wide context from here to _end().
int smk_thread_context_begin(int device_ordinal)
{
    if (t_ctx) { set_error("this thread already has a context of its own"); return SMK_BAD_PARAM; }
    t_ctx = new DeviceCtx;
    const int rc = smk_initialize(device_ordinal);
    if (rc != SMK_OK) { delete t_ctx; t_ctx = nullptr; }
    return rc;
}
void smk_thread_context_end(void)
{
    if (!t_ctx) return;
    smk_finalize();
    delete t_ctx;
    t_ctx = nullptr;
}
int smk_device_count(void)
{
    int n = 0;
    return hipGetDeviceCount(&n) == hipSuccess ? n : 0;
}
int smk_current_device(void)
{
    int d = 0;
    return hipGetDevice(&d) == hipSuccess ? d : -1;
}

size_t smk_device_trim(void)
{
    size_t cached = 0;
    smk::dev_cache_stats(nullptr, nullptr, &cached);
    smk::dev_trim();
    return cached;
}

int smk_device_synchronize(void)
{
    SMK_HIP(hipDeviceSynchronize());
    return SMK_OK;
}

int smk_device_cu_count(void) { return ctx().cus; }

int smk_set_stream(void* hip_stream)
{
    if (ctx().live_solvers > 0) { set_error("smk_set_stream: destroy every solver handle first"); return SMK_BAD_PARAM; }
    if (ctx().stream) (void)hipStreamSynchronize(ctx().stream);     // resident-matrix work queued on the old stream
    if (ctx().own_stream && ctx().stream) (void)hipStreamDestroy(ctx().stream);
    ctx().stream = (hipStream_t)hip_stream;
    ctx().own_stream = false;
    repoint_matrices(ctx().stream);           // resident matrices were created under the old stream
    return SMK_OK;
}

}  // extern "C"
