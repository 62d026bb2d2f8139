// memory.hip — memory the caller owns and the ways between host and device: rvb_device_alloc / rvb_host_alloc and their frees, the staged
// copies of pageable host memory (rvb_copy_to_host / rvb_copy_to_device) and the export stream (rvb_copy_to_pinned_host_async).
#include "ctx.h"

#include <algorithm>
#include <cstdlib>
#include <cstring>
#include <thread>

extern "C" {

// (within extern "C", as these helpers always were: their four names stay among the library's dynamic symbols)
namespace {

const size_t kCopyChunk = 8u << 20;          // bytes per pinned bounce buffer

int copy_lane_count()
{
    static const int lanes = [] {
        if (const char * e = getenv("RVB_COPY_THREADS")) return std::max(1, std::min(32, atoi(e)));
        const unsigned hw = std::thread::hardware_concurrency();
        return (int) std::max(1u, std::min(8u, hw ? hw / 2 : 4u));
    }();
    return lanes;
}

hipError_t ensure_copy_lanes(rvb_ctx * ctx)
{
    if (!ctx->copy_lanes.empty()) return hipSuccess;
    std::vector<rvb_ctx::CopyLane> lanes((size_t) copy_lane_count());
    for (rvb_ctx::CopyLane & l : lanes) {
        hipError_t e;
        for (int i = 0; i < 2; ++i) {
            if ((e = l.pinned[i].ensure(kCopyChunk)) != hipSuccess) return e;
            if ((e = hipEventCreateWithFlags(&l.done[i].h, hipEventDisableTiming)) != hipSuccess) return e;
        }
        if ((e = hipStreamCreateWithFlags(&l.stream.h, hipStreamNonBlocking)) != hipSuccess) return e;
    }
    ctx->copy_lanes.swap(lanes);          // (a failure above releases the lanes made so far with `lanes`)
    return hipSuccess;
}

// One lane's slice: chunk k+1 is on the link while chunk k is copied between the bounce buffer and pageable memory.
hipError_t lane_copy(int device, rvb_ctx::CopyLane & l, char * host, char * dev, size_t bytes, bool to_host)
{
    hipError_t e = hipSetDevice(device);
    if (e != hipSuccess) return e;
    const size_t nchunks = (bytes + kCopyChunk - 1) / kCopyChunk;
    auto span = [&](size_t k) { return std::min(kCopyChunk, bytes - k * kCopyChunk); };
    if (to_host) {
        if (nchunks && (e = hipMemcpyAsync(l.pinned[0].p, dev, span(0), hipMemcpyDeviceToHost, l.stream)) != hipSuccess) return e;
        if (nchunks && (e = hipEventRecord(l.done[0], l.stream)) != hipSuccess) return e;
        for (size_t k = 0; k < nchunks; ++k) {
            if (k + 1 < nchunks) {
                if ((e = hipMemcpyAsync(l.pinned[(k + 1) & 1].p, dev + (k + 1) * kCopyChunk, span(k + 1), hipMemcpyDeviceToHost, l.stream)) != hipSuccess) return e;
                if ((e = hipEventRecord(l.done[(k + 1) & 1], l.stream)) != hipSuccess) return e;
            }
            if ((e = hipEventSynchronize(l.done[k & 1])) != hipSuccess) return e;
            std::memcpy(host + k * kCopyChunk, l.pinned[k & 1].p, span(k));
        }
    } else {
        for (size_t k = 0; k < nchunks; ++k) {
            if (k >= 2 && (e = hipEventSynchronize(l.done[k & 1])) != hipSuccess) return e;      // the buffer's previous chunk has left
            std::memcpy(l.pinned[k & 1].p, host + k * kCopyChunk, span(k));
            if ((e = hipMemcpyAsync(dev + k * kCopyChunk, l.pinned[k & 1].p, span(k), hipMemcpyHostToDevice, l.stream)) != hipSuccess) return e;
            if ((e = hipEventRecord(l.done[k & 1], l.stream)) != hipSuccess) return e;
        }
        if ((e = hipStreamSynchronize(l.stream)) != hipSuccess) return e;
    }
    return hipSuccess;
}

int staged_copy(rvb_ctx * ctx, void * host, void * dev, uint64_t bytes, bool to_host)
{
    if (bytes == 0) return RVB_OK;
    RVB_HIP(fail, ctx, hipStreamSynchronize(ctx->stream));          // ordered after the context's work
    if (bytes < (4u << 20)) {                                 // small: one plain copy
        RVB_HIP(fail, ctx, to_host ? hipMemcpy(host, dev, bytes, hipMemcpyDeviceToHost) : hipMemcpy(dev, host, bytes, hipMemcpyHostToDevice));
        return RVB_OK;
    }
    RVB_HIP(fail, ctx, ensure_copy_lanes(ctx));
    const size_t lanes = ctx->copy_lanes.size();
    // slices are multiples of the chunk so that every lane moves whole chunks (2 MiB-aligned destinations keep the page
    // faults of fresh memory apart)
    const size_t chunks = (bytes + kCopyChunk - 1) / kCopyChunk, per = (chunks + lanes - 1) / lanes;
    std::vector<hipError_t> status(lanes, hipSuccess);
    std::vector<std::thread> workers;
    for (size_t i = 0; i < lanes; ++i) {
        const size_t first = i * per * kCopyChunk;
        if (first >= bytes) break;
        const size_t len = std::min((size_t) bytes - first, per * kCopyChunk);
        workers.emplace_back([=, &status] {
            status[i] = lane_copy(ctx->device, ctx->copy_lanes[i], static_cast<char *>(host) + first, static_cast<char *>(dev) + first, len, to_host);
        });
    }
    for (std::thread & t : workers) t.join();
    for (hipError_t e : status)
        if (e != hipSuccess) return fail(ctx, RVB_ERR_HIP, std::string("staged copy: ") + hipGetErrorString(e));
    return RVB_OK;
}

}  // namespace

int rvb_device_alloc(rvb_ctx * ctx, uint64_t bytes, void ** d_ptr)
{
    if (!ctx || !d_ptr) return RVB_ERR_INVALID;
    RVB_BIND(ctx);
    *d_ptr = nullptr;
    RVB_HIP(fail, ctx, hipMalloc(d_ptr, bytes ? bytes : 16));
    return RVB_OK;
}

int rvb_device_free(rvb_ctx * ctx, void * d_ptr)
{
    if (!ctx) return RVB_ERR_INVALID;
    if (!d_ptr) return RVB_OK;
    RVB_BIND(ctx);
    RVB_HIP(fail, ctx, hipStreamSynchronize(ctx->stream));
    RVB_HIP(fail, ctx, hipStreamSynchronize(ctx->export_stream));       // ... or a copy out of it
    RVB_HIP(fail, ctx, hipFree(d_ptr));
    return RVB_OK;
}

int rvb_copy_to_host(rvb_ctx * ctx, void * dst, const void * d_src, uint64_t bytes)
{
    if (!ctx) return RVB_ERR_INVALID;
    if (bytes && (!dst || !d_src)) return fail(ctx, RVB_ERR_INVALID, "rvb_copy_to_host: null pointer");
    RVB_BIND(ctx);
    return staged_copy(ctx, dst, const_cast<void *>(d_src), bytes, true);
}

int rvb_copy_to_device(rvb_ctx * ctx, void * d_dst, const void * src, uint64_t bytes)
{
    if (!ctx) return RVB_ERR_INVALID;
    if (bytes && (!d_dst || !src)) return fail(ctx, RVB_ERR_INVALID, "rvb_copy_to_device: null pointer");
    RVB_BIND(ctx);
    return staged_copy(ctx, const_cast<void *>(src), d_dst, bytes, false);
}

int rvb_host_alloc(rvb_ctx * ctx, uint64_t bytes, void ** host_ptr)
{
    if (!ctx || !host_ptr) return RVB_ERR_INVALID;
    RVB_BIND(ctx);
    *host_ptr = nullptr;
    RVB_HIP(fail, ctx, hipHostMalloc(host_ptr, bytes ? bytes : 16, hipHostMallocDefault));
    return RVB_OK;
}

int rvb_host_free(rvb_ctx * ctx, void * host_ptr)
{
    if (!ctx) return RVB_ERR_INVALID;
    if (!host_ptr) return RVB_OK;
    RVB_BIND(ctx);
    RVB_HIP(fail, ctx, hipStreamSynchronize(ctx->stream));
    RVB_HIP(fail, ctx, hipStreamSynchronize(ctx->export_stream));       // a copy into this block may still be on its way
    RVB_HIP(fail, ctx, hipHostFree(host_ptr));
    return RVB_OK;
}

int rvb_copy_to_pinned_host_async(rvb_ctx * ctx, void * pinned_dst, const void * d_src, uint64_t bytes)
{
    if (!ctx) return RVB_ERR_INVALID;
    if (bytes && (!pinned_dst || !d_src)) return fail(ctx, RVB_ERR_INVALID, "rvb_copy_to_pinned_host_async: null pointer");
    if (bytes == 0) return RVB_OK;
    RVB_BIND(ctx);
    // Ordered behind what the context's stream holds now, but on a stream of its own: neither the host nor the context's next trace
    // waits for the link.  The copy itself is the runtime's (a blit kernel on this box: no DMA engine takes it).  Measured at
    // workload C2, ms per IR in the bench pipeline (profiles/r03_export_variants_n1.txt): no copy 4.51-4.79, this 4.57-4.62, the same
    // copy issued from a torch side stream when the IR is handed over 4.96, in stream order on the context's own stream 5.90, and
    // copy kernels of this library's own with 2-512 waves and plain / nt / sc1 / sc0 sc1 stores 4.83-5.97 — stores to host memory
    // from a few long-lived waves slow every other kernel's memory traffic down for as long as they last.
    RVB_HIP(fail, ctx, hipEventRecord(ctx->export_ready, ctx->stream));
    RVB_HIP(fail, ctx, hipStreamWaitEvent(ctx->export_stream, ctx->export_ready, 0));
    RVB_HIP(fail, ctx, hipMemcpyAsync(pinned_dst, d_src, bytes, hipMemcpyDeviceToHost, ctx->export_stream));
    return RVB_OK;
}

int rvb_synchronize_exports(rvb_ctx * ctx)
{
    if (!ctx) return RVB_ERR_INVALID;
    RVB_BIND(ctx);
    RVB_HIP(fail, ctx, hipStreamSynchronize(ctx->export_stream));
    return RVB_OK;
}

}  // extern "C"
