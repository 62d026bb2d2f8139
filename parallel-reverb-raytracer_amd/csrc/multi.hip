// multi.hip — several GPUs of one node behind the C-ABI (rvb_multi_* of include/rvb_capi.h): one rvb_ctx and one host
// thread per device, contiguous ray shards, image-source candidates merged with the reference's lowest-ray-wins rule
// (rayverb.cpp:654-676), histograms combined on the devices.  The reference is single-device (rayverb.cpp:163, :176-177);
// this is the fan-out SURVEY.md §8(b) / §8(e) ask for, without Python or torch in the way.
//
// Histogram modes over D devices:
//   RVB_IR_EXACT  a CHAIN: device 0 folds its impulses into a zeroed histogram, hands it to device 1 (peer copy), which
//                 continues the same left-to-right float sum with ITS impulses (rvb_ir_accumulate adds on top of what the
//                 histogram holds), and so on; the merged image sources go last.  Shards are consecutive ray ranges, so the
//                 chain is the reference's serial order over all rays: bit-identical to one context (and to flattenImpulses).
//                 The traces — 85 % of the time — still run side by side, and so does every device's keying and sorting
//                 (rvb_ir_exact_prepare: it does not depend on the incoming histogram).  Only the fold is a chain, and it is
//                 SYSTOLIC (round 4): the histogram travels in B bin-range blocks, device g folds block k while device g + 1
//                 folds block k - 1 — (D + B - 1) / B folds and hops instead of D; events, no host waits between devices.
//   RVB_IR_FAST   every device bins its shard at once (float atomics), then ONE sum over devices: RCCL ncclAllReduce over
//                 xGMI, loaded from librccl.so at run time; devices that RCCL cannot put in one communicator (the same GPU
//                 listed twice, as the single-GPU tests do) are summed with peer copies and an add kernel instead.
// Host code only (the add kernel is histogram_kernels.hip's, behind rvb_launch_add; RCCL's binding is rccl_binding.h): the order of
// its calls is pinned without a GPU by tests/cpp/multi_order.cpp, which stands in for everything this file calls.
#include "../../include/rvb_capi.h"
#include "bin_blocks.h"
#include "hip_owned.h"
#include "image_merge.h"
#include "kernels.h"
#include "rccl_binding.h"

#include <algorithm>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <string>
#include <thread>
#include <vector>

namespace {

struct Shard {
    rvb_ctx * ctx = nullptr;
    int device = 0;
    uint64_t first = 0, count = 0;            // ray range
    Stream stream;                            // histogram traffic of this device
    DevBuf hist;
    float * histogram() const { return hist.as<float>(); }
    DevBuf peer;                              // landing buffer for another device's histogram (fallback sum)
    std::vector<Event> arrived, folded;       // exact chain: block k of the histogram has landed on this device / has been folded here
    int rc = RVB_OK;
    std::string error;
    Shard() = default;
    Shard(Shard &&) = default;
    ~Shard()
    {
        (void) hipSetDevice(device);
        if (stream) (void) hipStreamSynchronize(stream);
    }
};

}  // namespace

struct rvb_multi {
    std::vector<Shard> shards;
    std::string error;
    uint64_t nrays = 0, nreflections = 0;
    bool traced = false;
    std::vector<ncclComm_t> comms;            // one per shard when RCCL serves this device list
    bool rccl_tried = false, rccl_used_last = false;
    unsigned flags = 0;
    uint32_t chain_blocks = 8;                // bin-range blocks of the exact chain (rvb_multi_set_chain_blocks)
    int peer_links = 0;                       // directed device pairs with peer access enabled (rvb_multi_create)
    float mic[3] = {0, 0, 0};
    std::vector<rvb_impulse> images;          // merged image sources of the last rvb_multi_ir_* call
    ~rvb_multi()                              // (the contexts go first; then each shard's own stream, buffers and events)
    {
        for (ncclComm_t c : comms)
            if (c) (void) rccl().CommDestroy(c);
        for (Shard & s : shards) rvb_destroy(s.ctx);
    }
};

namespace {

int mfail(rvb_multi * m, int code, const std::string & what)
{
    if (m) m->error = what;
    return code;
}
// fail with this context's last error
int ctx_fail(rvb_multi * m, int code, const rvb_ctx * ctx) { return mfail(m, code, rvb_last_error(ctx)); }

// f(shard) on one host thread per device; the first failure is reported
template <class F>
int for_each_shard(rvb_multi * m, F f)
{
    std::vector<std::thread> pool;
    for (Shard & s : m->shards)
        pool.emplace_back([&s, &f] {
            s.rc = f(s);
            if (s.rc != RVB_OK) s.error = rvb_last_error(s.ctx);
        });
    for (std::thread & t : pool) t.join();
    for (Shard & s : m->shards)
        if (s.rc != RVB_OK) return mfail(m, s.rc, "device " + std::to_string(s.device) + ": " + s.error);
    return RVB_OK;
}

bool distinct_devices(const rvb_multi * m)
{
    for (size_t i = 0; i < m->shards.size(); ++i)
        for (size_t j = i + 1; j < m->shards.size(); ++j)
            if (m->shards[i].device == m->shards[j].device) return false;
    return true;
}

// one communicator over the device list, created on first use
bool ensure_rccl(rvb_multi * m)
{
    if (m->rccl_tried) return !m->comms.empty();
    m->rccl_tried = true;
    static const bool off = getenv("RVB_MULTI_RCCL") && getenv("RVB_MULTI_RCCL")[0] == '0';
    if (off || !rccl().ok() || !distinct_devices(m)) return false;
    std::vector<int> devs;
    for (const Shard & s : m->shards) devs.push_back(s.device);
    std::vector<ncclComm_t> comms(devs.size(), nullptr);
    if (rccl().CommInitAll(comms.data(), (int) devs.size(), devs.data()) != 0) return false;
    m->comms.swap(comms);
    return true;
}

}  // namespace

extern "C" {

int rvb_multi_create(rvb_multi ** out, const int * devices, int ndevices, unsigned flags)
{
    if (!out || ndevices <= 0 || ndevices > 64) return RVB_ERR_INVALID;
    *out = nullptr;
    std::unique_ptr<rvb_multi> m(new rvb_multi());
    m->flags = flags;
    m->shards.reserve((size_t) ndevices);
    for (int i = 0; i < ndevices; ++i) {
        m->shards.emplace_back();
        Shard & s = m->shards.back();
        s.device = devices ? devices[i] : i;
        const int rc = rvb_create(&s.ctx, s.device, 0);
        if (rc != RVB_OK) return rc;           // rvb_last_error(NULL) holds the text
        if (hipSetDevice(s.device) != hipSuccess || hipStreamCreateWithFlags(&s.stream.h, hipStreamNonBlocking) != hipSuccess) return RVB_ERR_HIP;
    }
    // peer access between every pair of distinct devices (the chain's hops, the fallback sum's gathers): without it the runtime stages a
    // peer copy through the host.  A refusal is not an error — the copies still work, staged.
    for (const Shard & a : m->shards)
        for (const Shard & b : m->shards) {
            if (a.device == b.device) continue;
            int can = 0;
            if (hipDeviceCanAccessPeer(&can, a.device, b.device) != hipSuccess || !can) { (void) hipGetLastError(); continue; }
            if (hipSetDevice(a.device) != hipSuccess) { (void) hipGetLastError(); continue; }
            const hipError_t e = hipDeviceEnablePeerAccess(b.device, 0);
            if (e == hipSuccess || e == hipErrorPeerAccessAlreadyEnabled) ++m->peer_links;
            (void) hipGetLastError();
        }
    *out = m.release();
    return RVB_OK;
}

int rvb_multi_set_chain_blocks(rvb_multi * m, uint32_t blocks)
{
    if (!m) return RVB_ERR_INVALID;
    if (blocks == 0 || blocks > 64) return mfail(m, RVB_ERR_INVALID, "rvb_multi_set_chain_blocks: 1 .. 64");
    m->chain_blocks = blocks;
    return RVB_OK;
}

int rvb_multi_peer_links(const rvb_multi * m) { return m ? m->peer_links : 0; }

void rvb_multi_destroy(rvb_multi * m) { delete m; }

const char * rvb_multi_last_error(const rvb_multi * m) { return m ? m->error.c_str() : rvb_last_error(nullptr); }

int rvb_multi_devices(const rvb_multi * m) { return m ? (int) m->shards.size() : 0; }

int rvb_multi_context(rvb_multi * m, int index, rvb_ctx ** ctx, uint64_t * first_ray, uint64_t * nrays)
{
    if (!m || index < 0 || index >= (int) m->shards.size()) return RVB_ERR_INVALID;
    if (ctx) *ctx = m->shards[(size_t) index].ctx;
    if (first_ray) *first_ray = m->shards[(size_t) index].first;
    if (nrays) *nrays = m->shards[(size_t) index].count;
    return RVB_OK;
}

int rvb_multi_used_rccl(const rvb_multi * m) { return m && m->rccl_used_last ? 1 : 0; }

int rvb_multi_set_scene(rvb_multi * m, const rvb_triangle * triangles, uint64_t ntriangles, const rvb_float3 * vertices, uint64_t nvertices,
                        const rvb_surface * surfaces, uint64_t nsurfaces)
{
    if (!m) return RVB_ERR_INVALID;
    m->traced = false;
    // replicated (MBs); every device builds the same tree from the same input
    return for_each_shard(m, [&](Shard & s) { return rvb_set_scene(s.ctx, triangles, ntriangles, vertices, nvertices, surfaces, nsurfaces); });
}

int rvb_multi_set_directions(rvb_multi * m, const rvb_float3 * directions, uint64_t nrays)
{
    if (!m) return RVB_ERR_INVALID;
    if (nrays && !directions) return mfail(m, RVB_ERR_INVALID, "rvb_multi_set_directions: null directions");
    const uint64_t d = m->shards.size(), base = nrays / d, extra = nrays % d;
    for (uint64_t g = 0; g < d; ++g) {         // contiguous ranges that differ by at most one ray (distributed.shard_range)
        m->shards[g].first = g * base + std::min(g, extra);
        m->shards[g].count = base + (g < extra ? 1 : 0);
    }
    m->nrays = nrays;
    m->traced = false;
    return for_each_shard(m, [&](Shard & s) { return rvb_set_directions(s.ctx, directions + s.first, s.count); });
}

int rvb_multi_set_source_pattern(rvb_multi * m, const rvb_source_pattern * pattern)
{
    if (!m) return RVB_ERR_INVALID;
    // every device scales its own shard: the records' rays are the shard's own direction slice
    for (Shard & s : m->shards) {
        const int rc = rvb_set_source_pattern(s.ctx, pattern, pattern ? 1 : 0);
        if (rc != RVB_OK) return mfail(m, rc, "device " + std::to_string(s.device) + ": " + rvb_last_error(s.ctx));
    }
    return RVB_OK;
}

int rvb_multi_trace(rvb_multi * m, const float mic[3], const float source[3], uint64_t nreflections, const float air_coefficient[8])
{
    if (!m) return RVB_ERR_INVALID;
    if (!mic || !source || !air_coefficient) return mfail(m, RVB_ERR_INVALID, "rvb_multi_trace: null argument");
    for (int i = 0; i < 3; ++i) m->mic[i] = mic[i];
    m->nreflections = nreflections;
    const int rc = for_each_shard(m, [&](Shard & s) {
        int r = rvb_trace(s.ctx, mic, source, nreflections, air_coefficient, s.first);       // ray numbers stay global
        return r != RVB_OK ? r : rvb_synchronize(s.ctx);
    });
    m->traced = rc == RVB_OK;
    return rc;
}

int rvb_multi_get_diffuse(rvb_multi * m, rvb_impulse * out)
{
    if (!m) return RVB_ERR_INVALID;
    if (!m->traced) return mfail(m, RVB_ERR_STATE, "rvb_multi_get_diffuse: nothing traced");
    if (m->nrays * m->nreflections && !out) return mfail(m, RVB_ERR_INVALID, "rvb_multi_get_diffuse: null output");
    // every device writes its slice of the ray-major array: D links at once
    return for_each_shard(m, [&](Shard & s) { return s.count ? rvb_get_diffuse(s.ctx, out + s.first * m->nreflections) : (int) RVB_OK; });
}

static int merged_images(rvb_multi * m, int remove_direct, std::vector<rvb_impulse> & images)
{
    std::vector<rvb_image_candidate> all;
    int rc;
    for (Shard & s : m->shards)
        if ((rc = append_image_candidates(s.ctx, all)) != RVB_OK) return ctx_fail(m, rc, s.ctx);
    rvb_impulse direct;
    std::memset(&direct, 0, sizeof(direct));
    rc = rvb_get_direct(m->shards[0].ctx, &direct);           // the same on every device
    if (rc != RVB_OK) return ctx_fail(m, rc, m->shards[0].ctx);
    // (no rays, no direct path)
    if ((rc = merge_images(all.data(), all.size(), m->nrays ? &direct : nullptr, remove_direct, images)) != RVB_OK) return mfail(m, rc, "rvb_merge_images");
    return RVB_OK;
}

int rvb_multi_get_images(rvb_multi * m, int remove_direct, rvb_impulse * out, uint64_t capacity, uint64_t * count)
{
    if (!m || !count) return RVB_ERR_INVALID;
    if (!m->traced) return mfail(m, RVB_ERR_STATE, "rvb_multi_get_images: nothing traced");
    std::vector<rvb_impulse> images;
    const int rc = merged_images(m, remove_direct, images);
    if (rc != RVB_OK) return rc;
    *count = images.size();
    if (!out) return RVB_OK;
    if (capacity < images.size()) return mfail(m, RVB_ERR_CAPACITY, "rvb_multi_get_images: capacity too small");
    if (!images.empty()) std::memcpy(out, images.data(), images.size() * sizeof(rvb_impulse));
    return RVB_OK;
}

// One rvb_multi_ir_* call: the model (speakers != NULL -> speaker channels, else HRTF: table, facing, up) and what to bin how
struct IrRequest {
    const float * mic;
    const rvb_speaker * speakers;
    uint64_t nspeakers;
    const float * table, * facing, * up;
    int which, remove_direct, trim_predelay, mode;
    float sample_rate;
    uint32_t nchannels() const { return speakers ? (uint32_t) nspeakers : 2u; }
    bool diffuse() const { return (which & RVB_IR_DIFFUSE) != 0; }
    int configure(rvb_ctx * ctx, int w, const rvb_impulse * images, uint64_t nimages) const
    {
        return speakers ? rvb_ir_configure_speakers(ctx, mic, speakers, nspeakers, w, images, nimages)
                        : rvb_ir_configure_hrtf(ctx, mic, table, facing, up, w, images, nimages);
    }
};
// what the time range of all shards makes of it: [nchannels][8][bins] floats on every device
struct IrLayout {
    float predelay = 0.0f;
    uint64_t bins = 0, rows = 0;
    size_t count() const { return (size_t) (bins * rows); }
    size_t bytes() const { return count() * sizeof(float); }
};

// 1. merged image sources (host, a few dozen records); time range of every shard and of the images -> predelay, bins
static int images_and_range(rvb_multi & m, const IrRequest & q, IrLayout & l)
{
    m.images.clear();
    if (q.which & RVB_IR_IMAGES) {
        const int rc = merged_images(&m, q.remove_direct, m.images);
        if (rc != RVB_OK) return rc;
    }
    std::vector<float> lo(m.shards.size() + 1, 0.0f), hi(m.shards.size() + 1, 0.0f);
    if (q.diffuse()) {
        const int rc = for_each_shard(&m, [&](Shard & s) {
            const size_t g = (size_t) (&s - m.shards.data());
            int r = q.configure(s.ctx, RVB_IR_DIFFUSE, nullptr, 0);
            return r != RVB_OK ? r : rvb_ir_time_range(s.ctx, &lo[g], &hi[g]);
        });
        if (rc != RVB_OK) return rc;
    }
    Shard & last = m.shards.back();
    if (!m.images.empty()) {
        int rc = q.configure(last.ctx, RVB_IR_IMAGES, m.images.data(), m.images.size());
        if (rc == RVB_OK) rc = rvb_ir_time_range(last.ctx, &lo.back(), &hi.back());
        if (rc != RVB_OK) return ctx_fail(&m, rc, last.ctx);
    }
    float min_nonzero = 0.0f, max_time = 0.0f;                 // findPredelay / MAX_SAMPLE inputs over all shards
    for (size_t i = 0; i < lo.size(); ++i) {
        if (lo[i] > 0.0f && (min_nonzero == 0.0f || lo[i] < min_nonzero)) min_nonzero = lo[i];
        max_time = std::max(max_time, hi[i]);
    }
    l.predelay = q.trim_predelay ? min_nonzero : 0.0f;
    l.bins = rvb_ir_bins(max_time, l.predelay, q.sample_rate);
    l.rows = (uint64_t) q.nchannels() * 8;
    return RVB_OK;
}

static int ensure_histograms(rvb_multi & m, size_t bytes)
{
    for (Shard & s : m.shards) { RVB_HIP(mfail, &m, hipSetDevice(s.device)); RVB_HIP(mfail, &m, s.hist.ensure(bytes)); }
    return RVB_OK;
}

// 2a. RVB_IR_EXACT, the systolic chain of the banner.  The blocks are whole 64-byte segments of every [channel][band] row.  Everything
// is enqueued from the caller's thread in dependency order: an event is recorded before the wait that names it is enqueued
// (tests/cpp/multi_order.cpp checks that, and that every device folds every block once, in order, behind its arrival).  The host
// waits once, at the end.
static int ensure_chain_events(rvb_multi & m, uint64_t nblocks)
{
    for (Shard & s : m.shards) {
        RVB_HIP(mfail, &m, hipSetDevice(s.device));
        for (std::vector<Event> * events : {&s.arrived, &s.folded})
            while (events->size() < nblocks) { Event e; RVB_HIP(mfail, &m, hipEventCreateWithFlags(&e.h, hipEventDisableTiming)); events->push_back(std::move(e)); }
    }
    return RVB_OK;
}

// (configured again: the range step may have left the last shard configured for the images)
static int prepare_shards(rvb_multi & m, const IrRequest & q, const IrLayout & l)
{
    return for_each_shard(&m, [&](Shard & s) {
        if (!q.diffuse() || !s.count) return (int) RVB_OK;
        int r = q.configure(s.ctx, RVB_IR_DIFFUSE, nullptr, 0);
        return r != RVB_OK ? r : rvb_ir_exact_prepare(s.ctx, l.predelay, q.sample_rate, l.bins);
    });
}

// device g: block by block, wait for the device before, fetch the block, fold this shard's impulses on top, say so
static int enqueue_device(rvb_multi & m, const IrRequest & q, const IrLayout & l, const BinBlocks & blocks, size_t g)
{
    Shard & s = m.shards[g];
    const uint64_t bins = l.bins;
    const bool folds = q.diffuse() && s.count;
    RVB_HIP(mfail, &m, hipSetDevice(s.device));
    if (g == 0) RVB_HIP(mfail, &m, hipMemsetAsync(s.histogram(), 0, l.bytes(), s.stream));
    for (uint64_t k = 0; k < blocks.count(); ++k) {
        const uint64_t b0 = blocks.range(k).b0, b1 = blocks.range(k).b1;
        if (g > 0) {
            Shard & prev = m.shards[g - 1];
            RVB_HIP(mfail, &m, hipStreamWaitEvent(s.stream, prev.folded[k], 0));
            if (prev.device == s.device) {
                RVB_HIP(mfail, &m, hipMemcpy2DAsync(s.histogram() + b0, bins * sizeof(float), prev.histogram() + b0, bins * sizeof(float), (b1 - b0) * sizeof(float), l.rows,
                                                    hipMemcpyDeviceToDevice, s.stream));
            } else {
                for (uint64_t r = 0; r < l.rows; ++r)     // (a row's piece of the block is contiguous: one peer copy each)
                    RVB_HIP(mfail, &m, hipMemcpyPeerAsync(s.histogram() + r * bins + b0, s.device, prev.histogram() + r * bins + b0, prev.device, (b1 - b0) * sizeof(float), s.stream));
            }
        }
        RVB_HIP(mfail, &m, hipEventRecord(s.arrived[k], s.stream));
        if (folds) {
            int rc = rvb_wait_for_event(s.ctx, s.arrived[k]);
            if (rc == RVB_OK) rc = rvb_ir_exact_fold(s.ctx, bins, b0, b1, s.histogram());
            if (rc == RVB_OK) rc = rvb_record_event(s.ctx, s.folded[k]);
            if (rc != RVB_OK) return ctx_fail(&m, rc, s.ctx);
        } else {
            RVB_HIP(mfail, &m, hipEventRecord(s.folded[k], s.stream));          // nothing to add here: the block passes through
        }
    }
    return RVB_OK;
}

static int exact_chain(rvb_multi & m, const IrRequest & q, const IrLayout & l)
{
    const BinBlocks blocks(l.bins, std::max<uint64_t>(1, std::min<uint64_t>(m.chain_blocks, (l.bins + 15) / 16)));
    int rc = ensure_chain_events(m, blocks.count());
    if (rc == RVB_OK) rc = prepare_shards(m, q, l);
    for (size_t g = 0; g < m.shards.size() && rc == RVB_OK; ++g) rc = enqueue_device(m, q, l, blocks, g);
    if (rc != RVB_OK) return rc;
    // the last device's folds are the end of the chain (a device without impulses only passed blocks on its own stream)
    Shard & last = m.shards.back();
    RVB_HIP(mfail, &m, hipSetDevice(last.device));
    RVB_HIP(mfail, &m, hipStreamSynchronize(last.stream));
    rc = rvb_synchronize(last.ctx);
    return rc == RVB_OK ? rc : ctx_fail(&m, rc, last.ctx);
}

// 2b. RVB_IR_FAST: all shards at once, then one sum over the devices
static int fast_bin_all(rvb_multi & m, const IrRequest & q, const IrLayout & l)
{
    return for_each_shard(&m, [&](Shard & s) {
        if (hipSetDevice(s.device) != hipSuccess || hipMemsetAsync(s.histogram(), 0, l.bytes(), s.stream) != hipSuccess ||
            hipStreamSynchronize(s.stream) != hipSuccess)
            return (int) RVB_ERR_HIP;
        if (!q.diffuse() || !s.count) return (int) RVB_OK;
        int r = q.configure(s.ctx, RVB_IR_DIFFUSE, nullptr, 0);
        if (r == RVB_OK) r = rvb_ir_accumulate(s.ctx, l.predelay, q.sample_rate, l.bins, RVB_IR_FAST, s.histogram());
        return r != RVB_OK ? r : rvb_synchronize(s.ctx);
    });
}

// RCCL over xGMI: [channels][8][nbins] floats, in place on every device (rccl.h:611)
static int sum_rccl(rvb_multi & m, size_t count)
{
    int e = rccl().GroupStart();
    for (size_t g = 0; g < m.shards.size() && e == 0; ++g) {
        RVB_HIP(mfail, &m, hipSetDevice(m.shards[g].device));
        e = rccl().AllReduce(m.shards[g].histogram(), m.shards[g].histogram(), count, kNcclFloat, kNcclSum, m.comms[g], m.shards[g].stream);
    }
    const int e2 = rccl().GroupEnd();
    if (e != 0 || e2 != 0) return mfail(&m, RVB_ERR_HIP, std::string("ncclAllReduce: ") + rccl().GetErrorString(e ? e : e2));
    for (Shard & s : m.shards) { RVB_HIP(mfail, &m, hipSetDevice(s.device)); RVB_HIP(mfail, &m, hipStreamSynchronize(s.stream)); }
    m.rccl_used_last = true;
    return RVB_OK;
}

// no communicator for this device list: gather on shard 0 with peer copies, add there
static int sum_peer(rvb_multi & m, const IrLayout & l)
{
    Shard & root = m.shards[0];
    RVB_HIP(mfail, &m, hipSetDevice(root.device));
    RVB_HIP(mfail, &m, root.peer.ensure(l.bytes()));
    for (size_t g = 1; g < m.shards.size(); ++g) {
        RVB_HIP(mfail, &m, hipMemcpyPeerAsync(root.peer.as<float>(), root.device, m.shards[g].histogram(), m.shards[g].device, l.bytes(), root.stream));
        rvb_launch_add(root.histogram(), root.peer.as<float>(), (uint64_t) l.count(), root.stream);
        RVB_HIP(mfail, &m, hipGetLastError());
    }
    RVB_HIP(mfail, &m, hipStreamSynchronize(root.stream));
    return RVB_OK;
}

// one sum over the devices: RCCL where it serves the device list, else peer copies; a single device has nothing to sum
static int sum_over_devices(rvb_multi & m, const IrLayout & l)
{
    const bool force = (m.flags & RVB_MULTI_REHEARSE_RCCL) != 0;
    if ((m.shards.size() > 1 || force) && ensure_rccl(&m)) return sum_rccl(m, l.count());
    return m.shards.size() > 1 ? sum_peer(m, l) : (int) RVB_OK;
}

// 3. the merged image sources go last (reference order: diffuse, then images — rayverb.cpp:708-714)
static int images_last(rvb_multi & m, const IrRequest & q, const IrLayout & l, Shard & result)
{
    if (m.images.empty()) return RVB_OK;
    int rc = q.configure(result.ctx, RVB_IR_IMAGES, m.images.data(), m.images.size());
    if (rc == RVB_OK) rc = rvb_ir_accumulate(result.ctx, l.predelay, q.sample_rate, l.bins, q.mode, result.histogram());
    if (rc == RVB_OK) rc = rvb_synchronize(result.ctx);
    return rc == RVB_OK ? rc : ctx_fail(&m, rc, result.ctx);
}

static int download(rvb_multi & m, Shard & result, float * out, size_t bytes)
{
    return rvb_copy_to_host(result.ctx, out, result.histogram(), bytes) == RVB_OK ? (int) RVB_OK : ctx_fail(&m, RVB_ERR_HIP, result.ctx);
}

static int multi_ir(rvb_multi * m, const IrRequest & q, float * out, uint64_t capacity_bins, uint64_t * nbins)
{
    if (!m || !nbins) return RVB_ERR_INVALID;
    if (!m->traced) return mfail(m, RVB_ERR_STATE, "rvb_multi_ir: nothing traced");
    if (q.which < 1 || q.which > 3) return mfail(m, RVB_ERR_INVALID, "rvb_multi_ir: which must be 1..3");
    IrLayout l;
    int rc = images_and_range(*m, q, l);
    if (rc != RVB_OK) return rc;
    *nbins = l.bins;
    if (!out) return RVB_OK;
    if (capacity_bins < l.bins) return mfail(m, RVB_ERR_CAPACITY, "rvb_multi_ir: capacity_bins too small");
    rc = ensure_histograms(*m, l.bytes());
    if (rc != RVB_OK) return rc;
    m->rccl_used_last = false;
    if (q.mode == RVB_IR_EXACT) {
        rc = exact_chain(*m, q, l);
    } else if (q.mode == RVB_IR_FAST) {
        rc = fast_bin_all(*m, q, l);
        if (rc == RVB_OK) rc = sum_over_devices(*m, l);
    } else {
        return mfail(m, RVB_ERR_INVALID, "rvb_multi_ir: unknown mode");
    }
    Shard & result = q.mode == RVB_IR_EXACT ? m->shards.back() : m->shards[0];      // the end of the chain / the root of the sum
    if (rc == RVB_OK) rc = images_last(*m, q, l, result);
    return rc == RVB_OK ? download(*m, result, out, l.bytes()) : rc;
}

int rvb_multi_ir_speakers(rvb_multi * m, const float mic[3], const rvb_speaker * speakers, uint64_t nspeakers, int which, int remove_direct,
                          int trim_predelay, float sample_rate, int mode, float * out, uint64_t capacity_bins, uint64_t * nbins)
{
    if (!m) return RVB_ERR_INVALID;
    if (!mic || !speakers || nspeakers == 0 || nspeakers > RVB_MAX_SPEAKERS) return mfail(m, RVB_ERR_INVALID, "rvb_multi_ir_speakers: 1.." RVB_STR(RVB_MAX_SPEAKERS) " speakers required");
    return multi_ir(m, IrRequest{mic, speakers, nspeakers, nullptr, nullptr, nullptr, which, remove_direct, trim_predelay, mode, sample_rate}, out, capacity_bins, nbins);
}

int rvb_multi_ir_hrtf(rvb_multi * m, const float mic[3], const float * table, const float facing[3], const float up[3], int which, int remove_direct,
                      int trim_predelay, float sample_rate, int mode, float * out, uint64_t capacity_bins, uint64_t * nbins)
{
    if (!m) return RVB_ERR_INVALID;
    if (!mic || !table || !facing || !up) return mfail(m, RVB_ERR_INVALID, "rvb_multi_ir_hrtf: null argument");
    return multi_ir(m, IrRequest{mic, nullptr, 0, table, facing, up, which, remove_direct, trim_predelay, mode, sample_rate}, out, capacity_bins, nbins);
}

}  // extern "C"
