// smallk_amd/csrc/owned.h -- who frees what.  Owned: the device blocks, pinned blocks, events and streams a handle
// (smk_solver, smk_matrix) created, released together and by nothing else.  Scratch: one device buffer that lives as
// long as a function call.  Host code only: no .hip file and not common.h include this.
#pragma once
#include "common.h"
#include "switches.h"

#include <algorithm>
#include <vector>

namespace smk {

template <typename T>
static int dev_alloc(T** p, size_t count)
{
    *p = nullptr;
    if (count == 0) count = 1;
    SMK_HIP(smk::dev_malloc((void**)p, count * sizeof(T)));
    // debugging aid: SMK_POISON=1 fills every fresh workspace with 0xFF bytes (NaN as fp64 / fp32, -1 as int), so that a
    // kernel reading memory nobody wrote shows up in every run instead of once in a hundred
    if (sw::poison()) { SMK_HIP(hipMemset(*p, 0xFF, count * sizeof(T))); SMK_HIP(hipDeviceSynchronize()); }   // the fill must not trail work on the non-blocking streams
    return 0;
}

// A handle's resources are created through its Owned member, and release() (the destructor calls it too) is the only place
// that frees them: an allocation site needs no line anywhere else.  The handle's fields keep pointing at the blocks and may
// be repointed freely (Wt / Gh / scal move into a communicator workspace): the record, not the field, is what gets freed.
// A function may also hold a local Owned for events it creates and needs no longer when it returns (the timed loop of
// smk_matrix_sparse_product): the same rule with the function as the handle.
class Owned {
    std::vector<void*> dev_, pinned_;
    std::vector<hipEvent_t> events_;
    std::vector<hipStream_t> streams_;

public:
    Owned() = default;
    Owned(const Owned&) = delete;
    Owned& operator=(const Owned&) = delete;
    ~Owned() { release(); }
    template <class T> int dev(T** p, size_t count) { const int rc = dev_alloc(p, count); adopt(*p); return rc; }
    void adopt(void* p) { if (p) dev_.push_back(p); }      // also: a block that a kernel file allocated with dev_malloc on the handle's behalf
    int pinned(void** p, size_t bytes) { *p = nullptr; SMK_HIP(hipHostMalloc(p, bytes)); pinned_.push_back(*p); return 0; }
    int event(hipEvent_t* e, unsigned flags) { *e = nullptr; SMK_HIP(hipEventCreateWithFlags(e, flags)); events_.push_back(*e); return 0; }
    int stream(hipStream_t* s, unsigned flags) { *s = nullptr; SMK_HIP(hipStreamCreateWithFlags(s, flags)); streams_.push_back(*s); return 0; }
    // free one device block early (a re-plan sizes it anew) and null the field; a field that points at a block this handle
    // does not own (an alias) is only nulled
    template <class T> void drop(T** p)
    {
        const auto it = std::find(dev_.begin(), dev_.end(), (void*)*p);
        if (*p && it != dev_.end()) { dev_.erase(it); (void)smk::dev_free(*p); }
        *p = nullptr;
    }
    void release()
    {
        for (hipStream_t s : streams_) (void)hipStreamSynchronize(s);
        for (void* p : dev_) (void)smk::dev_free(p);
        for (void* p : pinned_) (void)hipHostFree(p);
        for (hipEvent_t e : events_) (void)hipEventDestroy(e);
        for (hipStream_t s : streams_) (void)hipStreamDestroy(s);
        dev_.clear(); pinned_.clear(); events_.clear(); streams_.clear();
    }
};

// A device buffer of one function: freed when it leaves scope, on every return path.  Move-only.
template <class T>
class Scratch {
    T* p_ = nullptr;

public:
    Scratch() = default;
    Scratch(Scratch&& o) noexcept : p_(o.p_) { o.p_ = nullptr; }
    Scratch& operator=(Scratch&& o) noexcept { std::swap(p_, o.p_); return *this; }
    ~Scratch() { reset(); }
    int alloc(size_t count) { reset(); return dev_alloc(&p_, count); }
    T** put() { reset(); return &p_; }       // for an allocator with conventions of its own (dev_malloc by bytes)
    void reset() { if (p_) (void)smk::dev_free(p_); p_ = nullptr; }
    operator T*() const { return p_; }
};

}  // namespace smk
