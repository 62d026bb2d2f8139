// hip_owned.h — what the host layer (context, multi.hip, pipeline.hip) shares below the C-ABI: move-only owners of HIP resources,
// the stringify macro of the error texts and the HIP-check macro.
// The owners release in their destructors and never call hipSetDevice: the object that holds them binds its device in the body of its
// own destructor, before its members go (SceneStore, rvb_ctx, multi's Shard, pipeline's Lane).
#pragma once

#include <hip/hip_runtime.h>

#include <cstddef>
#include <cstring>
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

// A pinned staging block and the event behind the last copy that read it: host data goes up in stream order, with no host
// synchronisation unless a block has to grow, and the block is written again only after that copy has left it.
//   acquire(bytes, stream); fill host<T>(); hipMemcpyAsync from it, once or several times; record(stream)
struct StagedBlock {
    PinnedBuf block;
    Event free;
    // Room for `bytes` — in `dev` too, where one device buffer is filled from the block and grows with it —, then the block is the
    // caller's to write.  `stream` is synchronised before a block in use is replaced: a pass or a copy may still use the old one.
    hipError_t acquire(size_t bytes, hipStream_t stream, DevBuf * dev = nullptr)
    {
        hipError_t e = hipSuccess;
        if ((bytes > block.cap && block.p) || (dev && bytes > dev->cap && dev->p)) e = hipStreamSynchronize(stream);
        if (e == hipSuccess) e = block.ensure(bytes);
        if (e == hipSuccess && dev) e = dev->ensure(bytes);
        if (e != hipSuccess) return e;
        return free ? hipEventSynchronize(free) : hipEventCreateWithFlags(&free.h, hipEventDisableTiming);
    }
    template <class T> T * host() const { return block.as<T>(); }
    // behind the last copy out of the block on `stream`
    hipError_t record(hipStream_t stream) { return hipEventRecord(free, stream); }
    // the whole sequence for one device buffer
    hipError_t upload(DevBuf & dev, const void * src, size_t bytes, hipStream_t stream)
    {
        hipError_t e = acquire(bytes, stream, &dev);
        if (e != hipSuccess) return e;
        std::memcpy(block.p, src, bytes);
        e = hipMemcpyAsync(dev.p, block.p, bytes, hipMemcpyHostToDevice, stream);
        return e == hipSuccess ? record(stream) : e;
    }
};

#pragma GCC visibility pop
