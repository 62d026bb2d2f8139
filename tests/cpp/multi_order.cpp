// multi_order — the call order of the multi-GPU layer (rvb_multi_*, csrc/multi.hip) without a GPU.  This program defines the hip*
// functions, the add launcher of csrc/kernels.h and the rvb_* functions of the public C-ABI that multi.hip calls, links neither
// librvb_hip.so nor the HIP runtime, and drives rvb_multi_* through named scenarios.  Every call is logged with the context or the
// stream it names and the integer arguments that define the schedule (device, block bounds, bin counts, `which`, mode, byte counts,
// events and streams by creation order), never an array or a float.  Calls of the caller's thread form ONE sequence per scenario;
// calls made on the per-device threads of multi.hip go to a log per shard, printed (marked `|`) before the caller's next call.
// Memory is real: hipMalloc is malloc, the copies copy, the stand-in folds add a signature per shard, and the driver holds the
// downloaded histogram against the sum of signatures.  tests/test_multi_order_host.py builds it with the sanitizers, runs it and holds
// stdout against tests/golden/multi_call_order.txt.  A broken invariant goes to stderr and the exit code.  No argument.
#include "rvb_capi.h"

#include "bin_blocks.h"

#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <map>
#include <mutex>
#include <string>
#include <vector>

// ---- the stand-ins ---------------------------------------------------------------------------------------------------------------------

struct rvb_ctx {                                  // touched by one thread at a time: the caller's, or the shard's own between start and join
    int slot = 0, device = 0;
    std::string error;
    uint64_t rays = 0, first_ray = 0, nreflections = 0, nchannels = 0, nimages = 0;
    int which = 0;                                // of the last rvb_ir_configure_*
    bool prepared = false;                        // rvb_ir_exact_prepare since the last configure
    uint64_t prepared_bins = 0, next_b0 = 0, folds = 0;
    void * waited = nullptr;                      // the event of the last rvb_wait_for_event
    uint64_t fail_fold = 0;                       // failure switches: the k-th rvb_ir_exact_fold fails (0: none); rvb_trace fails
    bool fail_trace = false;
};

namespace {

const float RATE = 1000.0f;
const float IMAGE_SIGNATURE = 1024.0f;
float signature(int slot) { return (float) (1u << (2 * slot)); }      // 4^slot: a block folded twice shows as a digit 2

struct Block { size_t bytes; int device; };
struct StreamRec {
    int id = 0, device = 0;
    uint64_t landed = 0;                          // bins [0, landed) of every row have been copied (or zeroed) on this stream in this call
    uint64_t b0 = 0, b1 = 0, next_row = 0;        // the block that the per-row peer copies are filling
    uint64_t waited = 0;                          // what the event of its last hipStreamWaitEvent covers
};
struct EventRec {
    int id = 0, device = 0;
    long recorded_in = -1;                        // the rvb_multi_ir_* call of its last record
    int stream = -1;                              // that record's stream (-1: a context's)
    uint64_t covers = 0;                          // bins [0, covers) were there at that record: StreamRec::landed, or what the context had folded
};

struct Harness {
    std::mutex mu;                                // blocks, violations
    std::map<char *, Block> blocks;               // hipMalloc
    int violations = 0;
    // the caller's thread only, or written before the shard threads start:
    std::vector<std::string> log;
    std::vector<std::vector<std::string>> shard_log;
    std::vector<rvb_ctx *> ctxs;
    std::vector<StreamRec *> streams;
    int events = 0;
    long call = 0;                                // counts rvb_multi_ir_* calls
    uint64_t bins = 0, asked_blocks = 0;
    const uint64_t rows = 2 * 8;                  // every scenario has two channels
    int max_ms = 100;                             // the last impulse of every shard, in milliseconds
    int fail_create = 0;                          // the k-th rvb_create fails (0: none)
    int creates = 0;
    std::string null_error;
} H;

thread_local bool caller_thread = false;
thread_local int bound_device = 0;

void violation(const std::string & what)
{
    std::fprintf(stderr, "VIOLATION: %s\n", what.c_str());
    std::lock_guard<std::mutex> lk(H.mu);
    ++H.violations;
}

std::string fmt(const char * f, ...)
{
    char buf[320];
    va_list ap;
    va_start(ap, f);
    std::vsnprintf(buf, sizeof(buf), f, ap);
    va_end(ap);
    return buf;
}

void flush_shard_logs()
{
    for (std::vector<std::string> & l : H.shard_log) {
        for (const std::string & e : l) H.log.push_back("| " + e);
        l.clear();
    }
}

// `index`: the shard whose thread may be making the call (contexts and streams are created in shard order)
void logto(int index, const std::string & entry)
{
    if (caller_thread) {
        flush_shard_logs();
        H.log.push_back(entry);
    } else {
        H.shard_log[(size_t) index].push_back(entry);
    }
}
void logc(const rvb_ctx * c, const std::string & entry) { logto(c->slot, fmt("ctx %d: ", c->slot) + entry); }
void logs(const StreamRec * s, const std::string & entry) { logto(s->id, fmt("stream %d: ", s->id) + entry); }
void logh(const std::string & entry)
{
    if (!caller_thread) violation("a call that names no context and no stream was made off the caller's thread: " + entry);
    else logto(0, "host: " + entry);
}

typedef unsigned long long ull;

// (e) [p, p + bytes) lies inside one allocation; -> its device, and the offset of p in it
bool inside(const void * p, size_t bytes, const char * what, int * device = nullptr, size_t * offset = nullptr)
{
    char * q = const_cast<char *>(static_cast<const char *>(p));
    std::unique_lock<std::mutex> lk(H.mu);
    std::map<char *, Block>::iterator it = H.blocks.upper_bound(q);
    if (it != H.blocks.begin()) {
        --it;
        if (q >= it->first && (size_t) (q - it->first) + bytes <= it->second.bytes) {
            if (device) *device = it->second.device;
            if (offset) *offset = (size_t) (q - it->first);
            return true;
        }
    }
    lk.unlock();
    violation(fmt("%s touches bytes outside its allocation (%llu bytes)", what, (ull) bytes));
    return false;
}

// (d) a stream or a buffer is used only while the thread is bound to the device under which it was created
void bound(int device, const char * what)
{
    if (device != bound_device) violation(fmt("%s: made for device %d, used while the thread is bound to device %d", what, device, bound_device));
}

StreamRec * rec(hipStream_t s) { return reinterpret_cast<StreamRec *>(s); }
EventRec * rec(hipEvent_t e) { return reinterpret_cast<EventRec *>(e); }

// (a) an event is named by a wait only after its record was enqueued (in this rvb_multi_ir_* call: the events are kept between calls)
void named_by_a_wait(const EventRec * e, const char * who)
{
    if (e->recorded_in != H.call) violation(fmt("%s waits for event %d before its record was enqueued", who, e->id));
}

// (b) a block is fetched behind the wait for the event that the device before recorded after folding it (or passing it on)
void fetched_behind_its_fold(const StreamRec * st, uint64_t b0, uint64_t b1)
{
    if (st->waited < b1) violation(fmt("stream %d fetches block [%llu, %llu) without having waited for the device before to fold it", st->id, (ull) b0, (ull) b1));
}

// (c) a block starts where the one before it ended, on a multiple of 16 bins, and ends inside the histogram
void block_bounds(uint64_t expected_b0, uint64_t b0, uint64_t b1, const char * who)
{
    if (b0 != expected_b0 || b0 % 16 != 0 || b1 <= b0 || b1 > H.bins)
        violation(fmt("%s: block [%llu, %llu) where one from %llu was due (%llu bins)", who, (ull) b0, (ull) b1, (ull) expected_b0, (ull) H.bins));
}

void add_to_rows(float * hist, uint64_t rows, uint64_t bins, uint64_t b0, uint64_t b1, float value)
{
    for (uint64_t r = 0; r < rows; ++r)
        for (uint64_t b = b0; b < b1; ++b) hist[r * bins + b] += value;
}

}  // namespace

// the add launcher (csrc/kernels.h): the peer-copy sum of the fast mode
void rvb_launch_add(float * acc, const float * x, uint64_t n, hipStream_t s)
{
    logs(rec(s), fmt("rvb_launch_add n=%llu", (ull) n));
    bound(rec(s)->device, "rvb_launch_add's stream");
    int da = -1, dx = -1;
    if (!inside(acc, n * sizeof(float), "rvb_launch_add (acc)", &da) || !inside(x, n * sizeof(float), "rvb_launch_add (x)", &dx)) return;
    bound(da, "rvb_launch_add's acc");
    bound(dx, "rvb_launch_add's x");
    for (uint64_t i = 0; i < n; ++i) acc[i] += x[i];
}

extern "C" {

// ---- HIP: memory is malloc and free, streams and events are small heap objects ----------------------------------------------------------
hipError_t hipSetDevice(int device) { bound_device = device; return hipSuccess; }      // tracked per thread, not logged
const char * hipGetErrorString(hipError_t) { return "no error"; }
hipError_t hipGetLastError(void) { logh("hipGetLastError"); return hipSuccess; }
hipError_t hipDeviceCanAccessPeer(int * can, int device, int peer)
{
    logh(fmt("hipDeviceCanAccessPeer device=%d peer=%d", device, peer));
    *can = 1;
    return hipSuccess;
}
hipError_t hipDeviceEnablePeerAccess(int peer, unsigned int)
{
    logh(fmt("hipDeviceEnablePeerAccess device=%d peer=%d", bound_device, peer));
    return hipSuccess;
}
hipError_t hipMalloc(void ** p, size_t bytes)
{
    logh(fmt("hipMalloc device=%d bytes=%llu", bound_device, (ull) bytes));
    *p = std::malloc(bytes);
    std::lock_guard<std::mutex> lk(H.mu);
    H.blocks[static_cast<char *>(*p)] = Block{bytes, bound_device};
    return hipSuccess;
}
hipError_t hipFree(void * p)
{
    int device = -1;
    if (inside(p, 0, "hipFree", &device)) {
        logh(fmt("hipFree device=%d", device));
        bound(device, "hipFree's buffer");
        std::lock_guard<std::mutex> lk(H.mu);
        H.blocks.erase(static_cast<char *>(p));
    }
    std::free(p);
    return hipSuccess;
}
hipError_t hipStreamCreateWithFlags(hipStream_t * s, unsigned int)
{
    StreamRec * r = new StreamRec();
    r->id = (int) H.streams.size();
    r->device = bound_device;
    H.streams.push_back(r);
    logh(fmt("hipStreamCreateWithFlags device=%d -> stream %d", bound_device, r->id));
    *s = reinterpret_cast<hipStream_t>(r);
    return hipSuccess;
}
hipError_t hipStreamDestroy(hipStream_t s)
{
    logs(rec(s), "hipStreamDestroy");
    bound(rec(s)->device, "hipStreamDestroy's stream");
    H.streams[(size_t) rec(s)->id] = nullptr;
    delete rec(s);
    return hipSuccess;
}
hipError_t hipStreamSynchronize(hipStream_t s)
{
    logs(rec(s), "hipStreamSynchronize");
    bound(rec(s)->device, "hipStreamSynchronize's stream");
    return hipSuccess;
}
hipError_t hipEventCreateWithFlags(hipEvent_t * e, unsigned int)
{
    EventRec * r = new EventRec();
    r->id = H.events++;
    r->device = bound_device;
    logh(fmt("hipEventCreateWithFlags device=%d -> event %d", bound_device, r->id));
    *e = reinterpret_cast<hipEvent_t>(r);
    return hipSuccess;
}
hipError_t hipEventDestroy(hipEvent_t e)
{
    logh(fmt("hipEventDestroy event=%d", rec(e)->id));
    bound(rec(e)->device, "hipEventDestroy's event");
    delete rec(e);
    return hipSuccess;
}
hipError_t hipEventRecord(hipEvent_t e, hipStream_t s)
{
    logs(rec(s), fmt("hipEventRecord event=%d", rec(e)->id));
    bound(rec(s)->device, "hipEventRecord's stream");
    if (rec(e)->device != rec(s)->device) violation(fmt("event %d of device %d recorded on a stream of device %d", rec(e)->id, rec(e)->device, rec(s)->device));
    rec(e)->recorded_in = H.call;
    rec(e)->stream = rec(s)->id;
    rec(e)->covers = rec(s)->landed;
    return hipSuccess;
}
hipError_t hipStreamWaitEvent(hipStream_t s, hipEvent_t e, unsigned int)
{
    logs(rec(s), fmt("hipStreamWaitEvent event=%d", rec(e)->id));
    bound(rec(s)->device, "hipStreamWaitEvent's stream");
    named_by_a_wait(rec(e), fmt("stream %d", rec(s)->id).c_str());
    rec(s)->waited = rec(e)->covers;
    return hipSuccess;
}
hipError_t hipMemsetAsync(void * p, int value, size_t bytes, hipStream_t s)
{
    logs(rec(s), fmt("hipMemsetAsync value=%d bytes=%llu", value, (ull) bytes));
    bound(rec(s)->device, "hipMemsetAsync's stream");
    int device = -1;
    size_t offset = 0;
    if (!inside(p, bytes, "hipMemsetAsync", &device, &offset)) return hipSuccess;
    bound(device, "hipMemsetAsync's buffer");
    std::memset(p, value, bytes);
    if (offset == 0 && bytes == H.rows * H.bins * sizeof(float)) rec(s)->landed = H.bins;      // the whole histogram is there
    return hipSuccess;
}
// a block of the histogram, all rows in one call (both histograms on this device)
hipError_t hipMemcpy2DAsync(void * dst, size_t dpitch, const void * src, size_t spitch, size_t width, size_t height, hipMemcpyKind, hipStream_t s)
{
    StreamRec * st = rec(s);
    int dd = -1, sd = -1;
    size_t doff = 0, soff = 0;
    const size_t dspan = height ? (height - 1) * dpitch + width : 0, sspan = height ? (height - 1) * spitch + width : 0;
    const bool ok = inside(dst, dspan, "hipMemcpy2DAsync (dst)", &dd, &doff) && inside(src, sspan, "hipMemcpy2DAsync (src)", &sd, &soff);
    logs(st, fmt("hipMemcpy2DAsync dst=+%llu dpitch=%llu src=+%llu spitch=%llu width=%llu height=%llu", (ull) doff, (ull) dpitch, (ull) soff, (ull) spitch,
                 (ull) width, (ull) height));
    bound(st->device, "hipMemcpy2DAsync's stream");
    if (!ok) return hipSuccess;
    bound(dd, "hipMemcpy2DAsync's dst");
    bound(sd, "hipMemcpy2DAsync's src");
    for (size_t r = 0; r < height; ++r) std::memcpy(static_cast<char *>(dst) + r * dpitch, static_cast<const char *>(src) + r * spitch, width);
    const uint64_t b0 = doff / sizeof(float), b1 = b0 + width / sizeof(float);
    if (doff != soff || dpitch != H.bins * sizeof(float) || spitch != dpitch || height != H.rows) violation("hipMemcpy2DAsync: not a block of all rows of the histogram");
    block_bounds(st->landed, b0, b1, fmt("stream %d's copy", st->id).c_str());
    fetched_behind_its_fold(st, b0, b1);
    st->landed = b1;
    return hipSuccess;
}
// a row's piece of a block, from the histogram of another device
hipError_t hipMemcpyPeerAsync(void * dst, int dst_device, const void * src, int src_device, size_t bytes, hipStream_t s)
{
    StreamRec * st = rec(s);
    int dd = -1, sd = -1;
    size_t doff = 0, soff = 0;
    const bool ok = inside(dst, bytes, "hipMemcpyPeerAsync (dst)", &dd, &doff) && inside(src, bytes, "hipMemcpyPeerAsync (src)", &sd, &soff);
    logs(st, fmt("hipMemcpyPeerAsync dst=%d:+%llu src=%d:+%llu bytes=%llu", dst_device, (ull) doff, src_device, (ull) soff, (ull) bytes));
    bound(st->device, "hipMemcpyPeerAsync's stream");
    if (!ok) return hipSuccess;
    if (dd != dst_device || sd != src_device) violation(fmt("hipMemcpyPeerAsync: buffers of devices %d <- %d named as %d <- %d", dd, sd, dst_device, src_device));
    bound(dd, "hipMemcpyPeerAsync's dst");
    std::memcpy(dst, src, bytes);
    if (bytes == H.rows * H.bins * sizeof(float) && soff == 0) return hipSuccess;      // a whole histogram (the fast mode's gather)
    // a row's piece of a chain block: rows 0 .. rows - 1 of one block, then the next block
    const uint64_t at = doff / sizeof(float), row = at / H.bins, b0 = at % H.bins, b1 = b0 + bytes / sizeof(float);
    if (doff != soff) violation("hipMemcpyPeerAsync: source and destination are different pieces of the histogram");
    if (row == 0) {
        block_bounds(st->landed, b0, b1, fmt("stream %d's copy", st->id).c_str());
        fetched_behind_its_fold(st, b0, b1);
        st->b0 = b0, st->b1 = b1, st->next_row = 0;
    }
    if (row != st->next_row || b0 != st->b0 || b1 != st->b1) violation(fmt("stream %d: row %llu of block [%llu, %llu) out of turn", st->id, (ull) row, (ull) b0, (ull) b1));
    if (++st->next_row == H.rows) st->landed = b1;
    return hipSuccess;
}

// ---- the C-ABI below rvb_multi_* ---------------------------------------------------------------------------------------------------------
const char * rvb_last_error(const rvb_ctx * c) { return c ? c->error.c_str() : H.null_error.c_str(); }
int rvb_create(rvb_ctx ** out, int device, unsigned flags)
{
    logh(fmt("rvb_create device=%d flags=%u -> ctx %d", device, flags, (int) H.ctxs.size()));
    if (++H.creates == H.fail_create) {
        *out = nullptr;
        H.null_error = "rvb_create: the harness's failure switch";
        return RVB_ERR_NO_DEVICE;
    }
    rvb_ctx * c = new rvb_ctx();
    c->slot = (int) H.ctxs.size();
    c->device = device;
    H.ctxs.push_back(c);
    *out = c;
    return RVB_OK;
}
void rvb_destroy(rvb_ctx * c)
{
    if (!c) { logh("rvb_destroy null"); return; }
    logc(c, "rvb_destroy");
    H.ctxs[(size_t) c->slot] = nullptr;
    delete c;
}
int rvb_synchronize(rvb_ctx * c) { logc(c, "rvb_synchronize"); return RVB_OK; }
int rvb_wait_for_event(rvb_ctx * c, void * e)
{
    EventRec * ev = static_cast<EventRec *>(e);
    logc(c, fmt("rvb_wait_for_event event=%d", ev->id));
    named_by_a_wait(ev, fmt("context %d", c->slot).c_str());
    c->waited = e;
    return RVB_OK;
}
int rvb_record_event(rvb_ctx * c, void * e)
{
    EventRec * ev = static_cast<EventRec *>(e);
    logc(c, fmt("rvb_record_event event=%d", ev->id));
    if (ev->device != c->device) violation(fmt("event %d of device %d recorded by a context of device %d", ev->id, ev->device, c->device));
    ev->recorded_in = H.call;
    ev->stream = -1;
    ev->covers = c->next_b0;
    return RVB_OK;
}
int rvb_set_scene(rvb_ctx * c, const rvb_triangle *, uint64_t ntriangles, const rvb_float3 *, uint64_t nvertices, const rvb_surface *, uint64_t nsurfaces)
{
    logc(c, fmt("rvb_set_scene triangles=%llu vertices=%llu surfaces=%llu", (ull) ntriangles, (ull) nvertices, (ull) nsurfaces));
    return RVB_OK;
}
// (the driver numbers the rays in s[0]: the slice must begin at the shard's first ray, which rvb_trace names again)
int rvb_set_directions(rvb_ctx * c, const rvb_float3 * directions, uint64_t nrays)
{
    logc(c, fmt("rvb_set_directions rays=%llu", (ull) nrays));
    c->rays = nrays;
    for (uint64_t k = 1; k < nrays; ++k)
        if (directions[k].s[0] != directions[0].s[0] + (float) k) violation(fmt("context %d: its directions are not consecutive rays", c->slot));
    c->first_ray = nrays ? (uint64_t) directions[0].s[0] : 0;
    return RVB_OK;
}
int rvb_set_source_pattern(rvb_ctx * c, const rvb_source_pattern * patterns, uint64_t n)
{
    logc(c, fmt("rvb_set_source_pattern patterns=%llu null=%d", (ull) n, patterns ? 0 : 1));
    return RVB_OK;
}
int rvb_trace(rvb_ctx * c, const float *, const float *, uint64_t nreflections, const float *, uint64_t ray_offset)
{
    logc(c, fmt("rvb_trace nreflections=%llu ray_offset=%llu", (ull) nreflections, (ull) ray_offset));
    if (c->rays && c->first_ray != ray_offset) violation(fmt("context %d: traced at ray offset %llu with the directions from ray %llu on", c->slot, (ull) ray_offset, (ull) c->first_ray));
    c->nreflections = nreflections;
    if (c->fail_trace) { c->error = "rvb_trace: the harness's failure switch"; return RVB_ERR_HIP; }
    return RVB_OK;
}
int rvb_get_diffuse(rvb_ctx * c, rvb_impulse * out)
{
    logc(c, "rvb_get_diffuse");
    std::memset(out, c->slot + 1, (size_t) (c->rays * c->nreflections) * sizeof(rvb_impulse));      // every byte of the shard's slice
    return RVB_OK;
}
int rvb_get_direct(rvb_ctx * c, rvb_impulse * out) { logc(c, "rvb_get_direct"); std::memset(out, 0, sizeof(*out)); return RVB_OK; }
int rvb_get_image_candidates(rvb_ctx * c, rvb_image_candidate * out, uint64_t capacity, uint64_t * count)
{
    const uint64_t total = c->rays ? 1 + (uint64_t) c->slot % 2 : 0;
    logc(c, fmt("rvb_get_image_candidates capacity=%llu -> %llu", (ull) capacity, (ull) total));
    *count = total;
    if (!out) return RVB_OK;
    if (capacity < total) { c->error = "rvb_get_image_candidates: capacity"; return RVB_ERR_CAPACITY; }
    for (uint64_t k = 0; k < total; ++k) std::memset(out + k, 0, sizeof(*out));
    return RVB_OK;
}
int rvb_merge_images(const rvb_image_candidate * candidates, uint64_t n, const rvb_impulse * direct, int remove_direct, rvb_impulse * out, uint64_t capacity, uint64_t * count)
{
    logh(fmt("rvb_merge_images candidates=%llu direct=%d remove_direct=%d capacity=%llu -> %llu", (ull) n, direct ? 1 : 0, remove_direct, (ull) capacity, (ull) n));
    *count = n;                                   // keeps every candidate
    if (!out) return RVB_OK;
    if (capacity < n) return RVB_ERR_CAPACITY;
    for (uint64_t k = 0; k < n; ++k) out[k] = candidates[k].impulse;
    return RVB_OK;
}
static int configured(rvb_ctx * c, uint64_t nchannels, int which, uint64_t nimages)
{
    c->nchannels = nchannels;
    c->which = which;
    c->nimages = nimages;
    c->prepared = false;
    return RVB_OK;
}
int rvb_ir_configure_speakers(rvb_ctx * c, const float *, const rvb_speaker *, uint64_t nspeakers, int which, const rvb_impulse *, uint64_t nimages)
{
    logc(c, fmt("rvb_ir_configure_speakers speakers=%llu which=%d images=%llu", (ull) nspeakers, which, (ull) nimages));
    return configured(c, nspeakers, which, nimages);
}
int rvb_ir_configure_hrtf(rvb_ctx * c, const float *, const float * table, const float *, const float *, int which, const rvb_impulse *, uint64_t nimages)
{
    logc(c, fmt("rvb_ir_configure_hrtf table=%d which=%d images=%llu", table ? 1 : 0, which, (ull) nimages));
    return configured(c, 2, which, nimages);
}
// the shard's impulses lie between 10 + slot and max_ms milliseconds, the images between 5 and max_ms - 3; a shard without rays has none
int rvb_ir_time_range(rvb_ctx * c, float * lo, float * hi)
{
    logc(c, "rvb_ir_time_range");
    const bool images = c->which == RVB_IR_IMAGES;
    const bool any = images ? c->nimages != 0 : c->rays != 0;
    *lo = !any ? 0.0f : images ? 0.005f : 0.010f + 0.001f * (float) c->slot;
    *hi = !any ? 0.0f : 0.001f * (float) (images ? H.max_ms - 3 : H.max_ms);
    return RVB_OK;
}
uint64_t rvb_ir_bins(float max_time, float predelay, float sample_rate)
{
    H.bins = (uint64_t) std::ceil((max_time - predelay) * sample_rate) + 1;
    logh(fmt("rvb_ir_bins -> %llu", (ull) H.bins));
    return H.bins;
}
// the histogram a context adds to: [rows][nbins] floats inside one allocation of the context's device
static float * histogram_of(rvb_ctx * c, void * d_histogram, uint64_t nbins, const char * who)
{
    int device = -1;
    if (nbins != H.bins) violation(fmt("%s on context %d: %llu bins, the histogram has %llu", who, c->slot, (ull) nbins, (ull) H.bins));
    if (!inside(d_histogram, (size_t) (c->nchannels * 8 * nbins) * sizeof(float), who, &device)) return nullptr;
    if (device != c->device) violation(fmt("%s: a context of device %d adds to a buffer of device %d", who, c->device, device));
    return static_cast<float *>(d_histogram);
}
int rvb_ir_accumulate(rvb_ctx * c, float, float, uint64_t nbins, int mode, void * d_histogram)
{
    logc(c, fmt("rvb_ir_accumulate nbins=%llu mode=%d", (ull) nbins, mode));
    float * hist = histogram_of(c, d_histogram, nbins, "rvb_ir_accumulate");
    if (hist) add_to_rows(hist, c->nchannels * 8, nbins, 0, nbins, c->which == RVB_IR_IMAGES ? IMAGE_SIGNATURE : signature(c->slot));
    return RVB_OK;
}
int rvb_ir_exact_prepare(rvb_ctx * c, float, float, uint64_t nbins)
{
    logc(c, fmt("rvb_ir_exact_prepare nbins=%llu", (ull) nbins));
    if (c->which != RVB_IR_DIFFUSE) violation(fmt("context %d: rvb_ir_exact_prepare while configured for which=%d", c->slot, c->which));
    c->prepared = true;
    c->prepared_bins = nbins;
    c->next_b0 = 0;
    c->folds = 0;
    c->waited = nullptr;
    return RVB_OK;
}
// (b) after the wait for the event behind this block's arrival on the context's device, exactly once, in increasing order
int rvb_ir_exact_fold(rvb_ctx * c, uint64_t nbins, uint64_t b0, uint64_t b1, void * d_histogram)
{
    logc(c, fmt("rvb_ir_exact_fold nbins=%llu b0=%llu b1=%llu", (ull) nbins, (ull) b0, (ull) b1));
    if (!c->prepared || c->prepared_bins != nbins) violation(fmt("context %d: a fold without its rvb_ir_exact_prepare", c->slot));
    block_bounds(c->next_b0, b0, b1, fmt("context %d's fold", c->slot).c_str());
    const EventRec * ev = static_cast<const EventRec *>(c->waited);
    if (!ev || ev->recorded_in != H.call || ev->stream < 0 || ev->device != c->device || ev->covers < b1)
        violation(fmt("context %d folds block [%llu, %llu) without having waited for its arrival", c->slot, (ull) b0, (ull) b1));
    c->waited = nullptr;
    c->next_b0 = b1;
    if (++c->folds > H.asked_blocks) violation(fmt("context %d: more than the %llu blocks asked for", c->slot, (ull) H.asked_blocks));
    if (c->folds == c->fail_fold) { c->error = "rvb_ir_exact_fold: the harness's failure switch"; return RVB_ERR_HIP; }
    float * hist = histogram_of(c, d_histogram, nbins, "rvb_ir_exact_fold");
    if (hist) add_to_rows(hist, c->nchannels * 8, nbins, b0, std::min(b1, nbins), signature(c->slot));
    return RVB_OK;
}
int rvb_copy_to_host(rvb_ctx * c, void * dst, const void * d_src, uint64_t bytes)
{
    logc(c, fmt("rvb_copy_to_host bytes=%llu", (ull) bytes));
    int device = -1;
    if (!inside(d_src, bytes, "rvb_copy_to_host", &device)) return RVB_OK;
    if (device != c->device) violation(fmt("rvb_copy_to_host: a context of device %d reads a buffer of device %d", c->device, device));
    std::memcpy(dst, d_src, bytes);
    return RVB_OK;
}

}  // extern "C"

// ---- the driver --------------------------------------------------------------------------------------------------------------------------
namespace {

const float AIR[8] = {0, 0, 0, 0, 0, 0, 0, 0};
const float MIC[3] = {0, 1, 2}, SRC[3] = {3, 4, 5}, FACING[3] = {0, 0, 1}, UP[3] = {0, 1, 0};
const uint64_t REFLECTIONS = 3;
std::vector<float> table;

const char * which_name(int which) { return which == RVB_IR_ALL ? "all" : which == RVB_IR_DIFFUSE ? "diffuse" : which == RVB_IR_IMAGES ? "images" : "?"; }

struct Scenario {
    rvb_multi * m = nullptr;
    std::vector<int> devices;
    uint64_t rays = 0;
    uint32_t blocks = 8;                          // multi.hip's default
    bool traced = false;

    Scenario(int number, const char * name, const std::vector<int> & devs, int max_ms, int fail_create = 0) : devices(devs)
    {
        std::printf("scenario %d %s\n", number, name);
        H.log.clear();
        H.shard_log.assign(64, std::vector<std::string>());
        H.ctxs.clear();
        H.streams.clear();
        H.events = 0;
        H.creates = 0;
        H.fail_create = fail_create;
        H.max_ms = max_ms;
        H.bins = 0;
        H.asked_blocks = blocks;
        const int rc = rvb_multi_create(&m, devices.data(), (int) devices.size(), 0);
        if (rc != RVB_OK) note(fmt("rvb_multi_create rc=%d error=%s", rc, rvb_multi_last_error(m)));
        else note(fmt("rvb_multi_create rc=0 devices=%d peer_links=%d", rvb_multi_devices(m), rvb_multi_peer_links(m)));
    }

    void note(const std::string & line) { flush_shard_logs(); H.log.push_back("== " + line); }
    void report(const char * call, int rc) { note(fmt("%s rc=%d error=%s", call, rc, rc == RVB_OK ? "" : rvb_multi_last_error(m))); }
    rvb_ctx * ctx(int g)
    {
        rvb_ctx * c = nullptr;
        if (rvb_multi_context(m, g, &c, nullptr, nullptr) != RVB_OK) violation("rvb_multi_context failed");
        return c;
    }

    void chain_blocks(uint32_t n)
    {
        report("rvb_multi_set_chain_blocks", rvb_multi_set_chain_blocks(m, n));
        H.asked_blocks = blocks = n;
    }

    int trace(uint64_t nrays)
    {
        rays = nrays;
        rvb_triangle tri;
        rvb_float3 vert;
        rvb_surface surf;
        std::memset(&tri, 0, sizeof(tri));
        std::memset(&vert, 0, sizeof(vert));
        std::memset(&surf, 0, sizeof(surf));
        int rc = rvb_multi_set_scene(m, &tri, 1, &vert, 1, &surf, 1);
        flush_shard_logs();
        if (rc != RVB_OK) { report("rvb_multi_set_scene", rc); return rc; }
        std::vector<rvb_float3> dirs((size_t) nrays);
        for (uint64_t r = 0; r < nrays; ++r) dirs[(size_t) r].s[0] = (float) r, dirs[(size_t) r].s[1] = dirs[(size_t) r].s[2] = dirs[(size_t) r].s[3] = 0.0f;
        rc = rvb_multi_set_directions(m, dirs.data(), nrays);
        flush_shard_logs();
        if (rc != RVB_OK) { report("rvb_multi_set_directions", rc); return rc; }
        uint64_t next = 0;
        for (int g = 0; g < (int) devices.size(); ++g) {          // contiguous ranges that differ by at most one ray
            uint64_t first = 0, count = 0;
            rvb_ctx * c = nullptr;
            rvb_multi_context(m, g, &c, &first, &count);
            const uint64_t d = devices.size(), due = nrays / d + ((uint64_t) g < nrays % d ? 1 : 0);
            if (first != next || count != due || c->rays != count) violation(fmt("shard %d holds rays [%llu, +%llu), due [%llu, +%llu)", g, (ull) first, (ull) count, (ull) next, (ull) due));
            next += count;
        }
        rc = rvb_multi_trace(m, MIC, SRC, REFLECTIONS, AIR);
        report("rvb_multi_trace", rc);
        traced = rc == RVB_OK;
        return rc;
    }

    // the size query, then the call; the downloaded histogram against the sum of signatures
    int ir(bool hrtf, int which, int mode, int trim = 1, bool query_only = false, uint64_t capacity_less = 0)
    {
        rvb_speaker speakers[2];
        std::memset(speakers, 0, sizeof(speakers));
        const std::string call = fmt("%s which=%s mode=%d", hrtf ? "rvb_multi_ir_hrtf" : "rvb_multi_ir_speakers", which_name(which), mode);
        auto run = [&](float * out, uint64_t capacity, uint64_t * nbins) {
            ++H.call;
            for (StreamRec * s : H.streams) if (s) s->landed = s->b0 = s->b1 = s->next_row = s->waited = 0;
            return hrtf ? rvb_multi_ir_hrtf(m, MIC, table.data(), FACING, UP, which, 0, trim, RATE, mode, out, capacity, nbins)
                        : rvb_multi_ir_speakers(m, MIC, speakers, 2, which, 0, trim, RATE, mode, out, capacity, nbins);
        };
        uint64_t bins = 0;
        int rc = run(nullptr, 0, &bins);
        note(fmt("%s size query rc=%d bins=%llu error=%s", call.c_str(), rc, (ull) bins, rc == RVB_OK ? "" : rvb_multi_last_error(m)));
        if (rc != RVB_OK || query_only) return rc;
        std::vector<float> out((size_t) (H.rows * (bins - capacity_less)), -1.0f);
        uint64_t got = 0;
        rc = run(out.data(), bins - capacity_less, &got);
        note(fmt("%s rc=%d bins=%llu error=%s", call.c_str(), rc, (ull) got, rc == RVB_OK ? "" : rvb_multi_last_error(m)));
        if (rc != RVB_OK) return rc;
        float want = 0.0f;
        uint64_t with_rays = 0;
        for (int g = 0; g < (int) devices.size(); ++g) {
            const rvb_ctx * c = ctx(g);
            if (!c->rays) continue;
            ++with_rays;
            if (which & RVB_IR_DIFFUSE) want += signature(g);
            if (mode == RVB_IR_EXACT && (which & RVB_IR_DIFFUSE) && c->next_b0 != bins) violation(fmt("context %d folded bins [0, %llu) of %llu", g, (ull) c->next_b0, (ull) bins));
        }
        if ((which & RVB_IR_IMAGES) && with_rays) want += IMAGE_SIGNATURE;
        if (got != bins) violation("the call and its size query disagree about the bins");
        for (size_t k = 0; k < out.size(); ++k)
            if (out[k] != want) {
                violation(fmt("%s: row %llu bin %llu holds %d, the signatures add up to %d", call.c_str(), (ull) (k / bins), (ull) (k % bins), (int) out[k], (int) want));
                break;
            }
        return rc;
    }

    void diffuse()
    {
        std::vector<rvb_impulse> out((size_t) (rays * REFLECTIONS));      // (zeroed)
        report("rvb_multi_get_diffuse", rvb_multi_get_diffuse(m, out.data()));
        const uint64_t d = devices.size();
        for (uint64_t r = 0; r < rays && traced; ++r) {
            uint64_t g = 0, first = 0;
            for (; g < d; ++g) {
                const uint64_t count = rays / d + (g < rays % d ? 1 : 0);
                if (r < first + count) break;
                first += count;
            }
            const unsigned char * bytes = reinterpret_cast<const unsigned char *>(&out[(size_t) (r * REFLECTIONS)]);
            for (size_t k = 0; k < REFLECTIONS * sizeof(rvb_impulse); ++k)
                if (bytes[k] != g + 1) { violation(fmt("ray %llu's records were not written by shard %llu", (ull) r, (ull) g)); break; }
        }
    }

    void images()
    {
        uint64_t count = 0;
        int rc = rvb_multi_get_images(m, 0, nullptr, 0, &count);
        note(fmt("rvb_multi_get_images size query rc=%d count=%llu", rc, (ull) count));
        std::vector<rvb_impulse> out((size_t) count);
        uint64_t got = 0;
        rc = rvb_multi_get_images(m, 0, out.data(), count, &got);
        note(fmt("rvb_multi_get_images rc=%d count=%llu", rc, (ull) got));
        if (count > 1) {
            rc = rvb_multi_get_images(m, 1, out.data(), count - 1, &got);
            note(fmt("rvb_multi_get_images capacity=%llu rc=%d error=%s", (ull) (count - 1), rc, rvb_multi_last_error(m)));
        }
    }

    void pattern(bool set)
    {
        rvb_source_pattern p;
        std::memset(&p, 0, sizeof(p));
        report(set ? "rvb_multi_set_source_pattern set" : "rvb_multi_set_source_pattern clear", rvb_multi_set_source_pattern(m, set ? &p : nullptr));
    }

    ~Scenario()
    {
        note("rvb_multi_destroy");
        rvb_multi_destroy(m);
        flush_shard_logs();
        for (const std::string & e : H.log) std::printf("%s\n", e.c_str());
        for (const rvb_ctx * c : H.ctxs) if (c) violation(fmt("context %d was not destroyed", c->slot));
        for (const StreamRec * s : H.streams) if (s) violation(fmt("stream %d was not destroyed", s->id));
        std::lock_guard<std::mutex> lk(H.mu);
        if (!H.blocks.empty()) { std::fprintf(stderr, "VIOLATION: %d device buffer(s) were not freed\n", (int) H.blocks.size()); ++H.violations; }
    }
};

// csrc/bin_blocks.h against the two expressions it replaces, as csrc/ir.hip (export slices) and csrc/multi.hip (chain blocks) spelled them
void check_bin_blocks()
{
    uint64_t cases = 0;
    for (uint64_t bins = 1; bins <= 600; ++bins)
        for (uint64_t parts = 1; parts <= 64; ++parts, ++cases) {
            // ir.hip: for (b0 = 0; b0 < nbins; b0 += per) { b1 = min(nbins, b0 + per); ... }
            const uint64_t per = ((bins + parts - 1) / parts + 15) & ~15ull;
            const BinBlocks ir(bins, parts);
            uint64_t k = 0;
            for (uint64_t b0 = 0; b0 < bins; b0 += per, ++k) {
                const uint64_t b1 = std::min(bins, b0 + per);
                if (k >= ir.count() || ir.range(k).b0 != b0 || ir.range(k).b1 != b1) violation(fmt("bin_blocks: bins=%llu parts=%llu block %llu differs from ir.hip's", (ull) bins, (ull) parts, (ull) k));
            }
            if (k != ir.count() || ir.per != per) violation(fmt("bin_blocks: bins=%llu parts=%llu: count or per differs from ir.hip's", (ull) bins, (ull) parts));
            // multi.hip: the clamp, then per, nblocks and b0 = k * per, b1 = min(bins, b0 + per)
            const uint64_t blocks = std::max<uint64_t>(1, std::min<uint64_t>(parts, (bins + 15) / 16));
            const uint64_t mper = ((bins + blocks - 1) / blocks + 15) & ~15ull;
            const uint64_t nblocks = (bins + mper - 1) / mper;
            const BinBlocks chain(bins, blocks);
            if (chain.per != mper || chain.count() != nblocks) violation(fmt("bin_blocks: bins=%llu parts=%llu: count or per differs from multi.hip's", (ull) bins, (ull) parts));
            for (uint64_t j = 0; j < nblocks; ++j) {
                const uint64_t b0 = j * mper, b1 = std::min<uint64_t>(bins, b0 + mper);
                if (chain.range(j).b0 != b0 || chain.range(j).b1 != b1) violation(fmt("bin_blocks: bins=%llu parts=%llu block %llu differs from multi.hip's", (ull) bins, (ull) parts, (ull) j));
            }
        }
    std::printf("bin_blocks.h: %llu cases equal the expressions of ir.hip and multi.hip\n", (ull) cases);
}

}  // namespace

int main()
{
    caller_thread = true;
    setenv("RVB_MULTI_RCCL", "0", 1);             // ensure_rccl never reaches dlopen (the RCCL sum is the GPU suite's)
    table.assign((size_t) 2 * 360 * 180 * 8, 0.5f);
    check_bin_blocks();
    {
        Scenario s(1, "one_device_exact_then_fast", {0}, 100);
        s.trace(5);
        s.ir(false, RVB_IR_ALL, RVB_IR_EXACT);
        s.ir(false, RVB_IR_ALL, RVB_IR_FAST);
    }
    {
        Scenario s(2, "device_0_twice_speakers_exact_then_fast_peer_copy_and_add", {0, 0}, 100);
        s.trace(7);
        s.ir(false, RVB_IR_ALL, RVB_IR_EXACT);
        s.ir(false, RVB_IR_ALL, RVB_IR_FAST);
    }
    {
        Scenario s(3, "device_0_four_times_3_blocks_hrtf_all_diffuse_images", {0, 0, 0, 0}, 300);
        s.chain_blocks(3);
        s.trace(10);
        for (int which : {RVB_IR_ALL, RVB_IR_DIFFUSE, RVB_IR_IMAGES}) s.ir(true, which, RVB_IR_EXACT);
        for (int which : {RVB_IR_ALL, RVB_IR_DIFFUSE, RVB_IR_IMAGES}) s.ir(true, which, RVB_IR_FAST, 0);
    }
    {
        Scenario s(4, "3_rays_on_4_devices_the_last_shard_is_empty", {0, 0, 0, 0}, 100);
        s.chain_blocks(2);
        s.trace(3);
        s.ir(false, RVB_IR_ALL, RVB_IR_EXACT);
        s.ir(false, RVB_IR_DIFFUSE, RVB_IR_EXACT, 0);
        s.ir(true, RVB_IR_ALL, RVB_IR_FAST);
        s.diffuse();
        s.images();
    }
    {
        Scenario s(5, "distinct_devices_0_1_2_exact_then_fast", {0, 1, 2}, 60);
        if (rvb_multi_peer_links(s.m) != 6) violation("three distinct devices have six directed peer links");
        s.chain_blocks(3);
        s.trace(8);
        s.ir(false, RVB_IR_ALL, RVB_IR_EXACT);
        s.ir(true, RVB_IR_ALL, RVB_IR_EXACT);
        s.ir(false, RVB_IR_ALL, RVB_IR_FAST);
    }
    {
        Scenario s(6, "38_bins_clamp_the_default_8_blocks", {0, 0}, 36);
        s.trace(4);
        s.ir(false, RVB_IR_DIFFUSE, RVB_IR_EXACT, 0);
        s.ir(false, RVB_IR_ALL, RVB_IR_EXACT, 0, true);       // the size query alone
    }
    {
        Scenario s(7, "source_pattern_diffuse_images", {0, 1}, 100);
        s.pattern(true);
        s.trace(6);
        s.diffuse();
        s.images();
        s.pattern(false);
    }
    {
        Scenario s(8, "refused_calls", {0, 0}, 100);
        s.report("rvb_multi_set_chain_blocks 0", rvb_multi_set_chain_blocks(s.m, 0));
        s.ir(false, RVB_IR_ALL, RVB_IR_EXACT);                 // not traced
        s.diffuse();
        s.images();
        s.trace(6);
        s.ir(false, 0, RVB_IR_EXACT);
        s.ir(true, 4, RVB_IR_FAST);
        s.ir(false, RVB_IR_ALL, 2);                            // unknown mode: the size query passes
        s.ir(true, RVB_IR_ALL, RVB_IR_EXACT, 1, false, 1);     // capacity too small
    }
    {
        Scenario s(9, "the_second_fold_of_shard_1_fails", {0, 0, 0}, 100);
        s.chain_blocks(4);
        s.trace(9);
        s.ctx(1)->fail_fold = 2;
        s.ir(false, RVB_IR_ALL, RVB_IR_EXACT);
        s.ctx(1)->fail_fold = 0;
        s.ir(false, RVB_IR_ALL, RVB_IR_EXACT);                 // and the next call is whole again
    }
    {
        Scenario s(10, "the_trace_of_shard_1_fails", {0, 1, 2}, 100);
        s.ctx(1)->fail_trace = true;
        s.trace(9);
        s.ir(false, RVB_IR_ALL, RVB_IR_EXACT);
    }
    {
        std::printf("scenario 11 rvb_create_fails_at_the_second_device\n");
        H.log.clear();
        H.ctxs.clear();
        H.streams.clear();
        H.creates = 0;
        H.fail_create = 2;
        rvb_multi * m = nullptr;
        const int rc = rvb_multi_create(&m, nullptr, 3, 0);
        H.fail_create = 0;
        flush_shard_logs();
        for (const std::string & e : H.log) std::printf("%s\n", e.c_str());
        std::printf("== rvb_multi_create rc=%d multi=%s error=%s\n", rc, m ? "set" : "null", rvb_multi_last_error(m));
        for (const rvb_ctx * c : H.ctxs) if (c) violation(fmt("context %d was not destroyed", c->slot));
        for (const StreamRec * st : H.streams) if (st) violation(fmt("stream %d was not destroyed", st->id));
    }
    if (H.violations) { std::fprintf(stderr, "%d violation(s)\n", H.violations); return 1; }
    return 0;
}
