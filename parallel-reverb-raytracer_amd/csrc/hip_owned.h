// hip_owned.h — what the host layer (context, multi.hip, pipeline.hip) shares below the C-ABI: move-only owners of HIP resources,
// the stringify macro of the error texts and the HIP-check macro.
// The owners release in their destructors and never call hipSetDevice: the object that holds them binds its device in the body of its
// own destructor, before its members go (SceneStore, rvb_ctx, multi's Shard, pipeline's Lane).
#pragma once

#include <hip/hip_runtime.h>

#include <cstddef>
#include <string>

#define RVB_STR_(x) #x
#define RVB_STR(x) RVB_STR_(x)      // RVB_MAX_SPEAKERS in error texts

// `return failf(obj, RVB_ERR_HIP, "<call>: <HIP's text>")` if the call fails; failf is the file's own (fail, mfail, pfail: they write
// to different objects)
#define RVB_HIP(failf, obj, call)                                                                       \
    do {                                                                                                \
        hipError_t e_ = (call);                                                                         \
        if (e_ != hipSuccess)                                                                           \
            return failf(obj, RVB_ERR_HIP, std::string(#call) + ": " + hipGetErrorString(e_));          \
    } while (0)

#pragma GCC visibility push(hidden)

// A block of device memory (Pinned = false) or of pinned host memory (true) that only grows.  (Move-constructible, so that a vector
// can hold its owner; nothing assigns one.)
template <bool Pinned>
struct OwnedBlock {
    void * p = nullptr;
    size_t cap = 0;
    OwnedBlock() = default;
    OwnedBlock(OwnedBlock && o) noexcept : p(o.p), cap(o.cap) { o.p = nullptr; o.cap = 0; }
    ~OwnedBlock() { if (p) (void) free_block(p); }
    static hipError_t free_block(void * q) { return Pinned ? hipHostFree(q) : hipFree(q); }
    // what the block held is gone after a growth; ensure(0) on an empty block allocates nothing
    hipError_t ensure(size_t bytes)
    {
        if (bytes <= cap)
            return hipSuccess;
        if (p) { hipError_t e = free_block(p); p = nullptr; cap = 0; if (e != hipSuccess) return e; }
        hipError_t e = Pinned ? hipHostMalloc(&p, bytes ? bytes : 16, hipHostMallocDefault) : hipMalloc(&p, bytes ? bytes : 16);
        if (e == hipSuccess) cap = bytes;
        return e;
    }
    template <class T> T * as() const { return reinterpret_cast<T *>(p); }
};
using DevBuf = OwnedBlock<false>;
using PinnedBuf = OwnedBlock<true>;

// A stream / an event: created by the holder with the HIP call it needs (`hipStreamCreateWithPriority(&s.h, ...)`), destroyed here.
template <class Handle, hipError_t (*Destroy)(Handle)>
struct OwnedHandle {
    Handle h = nullptr;
    OwnedHandle() = default;
    OwnedHandle(OwnedHandle && o) noexcept : h(o.h) { o.h = nullptr; }
    ~OwnedHandle() { if (h) (void) Destroy(h); }
    operator Handle() const { return h; }
};
using Stream = OwnedHandle<hipStream_t, hipStreamDestroy>;
using Event = OwnedHandle<hipEvent_t, hipEventDestroy>;

#pragma GCC visibility pop
