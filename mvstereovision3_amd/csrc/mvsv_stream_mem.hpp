// mvsv_stream_mem.hpp — move-only owners of what the frame stream allocates
// (mvsv_stream.cpp): device and pinned arrays, events and HIP streams.  An owner
// frees what it holds when it goes away or is assigned over, so a stage of the
// stream is switched off by `stage = {}`.  Not the context's DevBuf / ensure():
// those are its grow-only cache and tied to its graph epoch.
#pragma once

#include <hip/hip_runtime.h>

#include <cstddef>
#include <utility>

namespace mvsv {

struct FreeDevice {
    void operator()(void* p) const { (void)hipFree(p); }
};
struct FreePinned {
    void operator()(void* p) const { (void)hipHostFree(p); }
};
struct FreeEvent {
    void operator()(hipEvent_t e) const { (void)hipEventDestroy(e); }
};
struct FreeStream {
    void operator()(hipStream_t s) const { (void)hipStreamDestroy(s); }
};

// One handle (a pointer of some kind) and how to give it back.
template <class H, class Free>
class Owned {
  public:
    Owned() = default;
    explicit Owned(H h) : h_(h) {}
    Owned(Owned&& o) noexcept : h_(std::exchange(o.h_, H())) {}
    Owned& operator=(Owned&& o) noexcept
    {
        std::swap(h_, o.h_);  // o, a temporary or a moved-from object, frees the old handle
        return *this;
    }
    ~Owned()
    {
        if (h_) Free()(h_);
    }
    operator H() const { return h_; }
    H get() const { return h_; }

  protected:
    H h_ = H();
};

// T[count] in device memory
template <class T>
struct DevArray : Owned<T*, FreeDevice> {
    bool alloc(size_t count)
    {
        *this = DevArray();
        return hipMalloc((void**)&this->h_, count * sizeof(T)) == hipSuccess;
    }
};

// T[count] in pinned host memory
template <class T>
struct PinnedArray : Owned<T*, FreePinned> {
    using Owned<T*, FreePinned>::Owned;
    bool alloc(size_t count)
    {
        *this = PinnedArray();
        return hipHostMalloc((void**)&this->h_, count * sizeof(T), hipHostMallocDefault) == hipSuccess;
    }
};

struct Event : Owned<hipEvent_t, FreeEvent> {
    bool create() { return hipEventCreateWithFlags(&h_, hipEventDisableTiming) == hipSuccess; }
};

struct Stream : Owned<hipStream_t, FreeStream> {
    bool create() { return hipStreamCreateWithFlags(&h_, hipStreamNonBlocking) == hipSuccess; }
};

}  // namespace mvsv
