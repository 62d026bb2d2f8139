// ctx.h — the context behind include/rvb_capi.h and what its translation units share:
//   context.hip  life cycle, scene (ContextScene below), directions, timings, diagnostics
//   trace.hip    the trace in three steps (TraceStage below, over trace_state.h), the tail steps a kept trace replays, its results, rvb_merge_images
//   source.hip   source directivity (SourceDirectivity below, over source_state.h / source_state.hip): setters, upload, launches
//   kept.hip     behind a kept trace (KeptTrace below, over kept_state.h): re-shading, its material gradients per surface and per
//                triangle, a new microphone
//   memory.hip   caller-owned device / pinned memory, staged host copies, the export stream
//   sort.hip     the sorts the other stages call, their buffers (SortBuffers below), "sorted list and bin boundaries"
//   ir.hip       the fused impulse-response stage (IrStage below, over ir_state.h): configure, time range, binning, download / export
//   flatten.hip  the materialised steps of the reference: attenuate per channel, fix the predelay, flatten
//   decay.hip    decay curves, reverberation times and the decay loss on the caller's device arrays
//   images.hip   include/rvb_capi_images.h: the merged image list made on the device (MergedImages below, over merged_state.h), the
//                image-source part of the material gradient
//   speech.hip   include/rvb_capi_speech.h: modulation transfer, its adjoint and the speech transmission index (speech_kernels.hip, speech_index.h)
//   window.hip   include/rvb_capi_window.h: the strongest records behind a time window and their paths (window_kernels.hip, over window_select.h)
// No compute happens in them and nothing falls back to the CPU: every entry point that produces results launches HIP kernels:
//   the trace         trace_kernels.hip, image_kernels.hip, shadow_kernels.hip, source_kernels.hip
//   a kept trace      reshade_kernels.hip, reshade_grad_kernels.hip, relisten_kernels.hip (the three over kept_tiles.h),
//                     reshade_grad_map_kernels.hip
//   the image list    image_grad_kernels.hip
//   the IR stage      attenuate_kernels.hip, histogram_kernels.hip, exact_kernels.hip, decay_kernels.hip
//   the sorts         rocprim_sort.hip, radix_sort.hip
#pragma once

#include "../../include/rvb_capi.h"
#include "hip_owned.h"
#include "ir_state.h"
#include "kept_state.h"
#include "kernels.h"
#include "merged_state.h"
#include "source_state.h"
#include "trace_state.h"

#include <cmath>
#include <cstddef>
#include <cstring>
#include <memory>
#include <string>
#include <utility>
#include <vector>

#pragma GCC visibility push(hidden)

// The scene's device buffers: built and uploaded once (rvb_set_scene), read by every context that holds the store (rvb_share_scene) —
// one copy in HBM, and ONE copy for the L2s to keep, however many contexts trace in it side by side.  Freed with its last holder.
struct SceneStore {
    int device = 0;
    DevBuf nodes, tris, shade, corners, surfaces;
    ~SceneStore() { (void) hipSetDevice(device); }
};

// A context's scene as one value: the store it holds (its own after rvb_set_scene, another context's after rvb_share_scene, which
// copies the whole value), where the kernels find it, and its counts.  Nothing of it is read while have() is false.
struct ContextScene {
    std::shared_ptr<SceneStore> store;
    SceneDev dev;
    uint64_t nnodes = 0, kept_triangles = 0;
    uint32_t depth = 0;
    uint32_t stack_need = RVB_BVH_STACK;
    uint64_t nsurfaces = 0;
    uint64_t ntriangles = 0;                     // as passed to rvb_set_scene: the index space of a record's triangle
    bool have() const { return have_; }
    // rvb_set_scene begins: no scene until set() — what a failure midway leaves.  The store stays, to be reused if held alone.
    void drop() { have_ = false; }
    // rvb_set_scene has uploaded into the store
    void set(const SceneDev & on_device, uint64_t nodes, uint64_t kept, uint32_t tree_depth, uint32_t stack, uint64_t surfaces, uint64_t triangles)
    {
        dev = on_device;
        nnodes = nodes; kept_triangles = kept; depth = tree_depth; stack_need = stack; nsurfaces = surfaces; ntriangles = triangles;
        have_ = true;
    }

private:
    bool have_ = false;
};

// The small result block of a trace: one per context on the device, fetched into its pinned host mirror once per trace (fetch_small).
struct SmallBlock {
    uint32_t candidate_count;           // image-source candidates (image kernels)
    uint32_t pad0_;
    unsigned long long executed;        // bounces executed
    uint32_t range[2];                  // float bits: time range of the HRTF model's attenuated impulses (time_range_kernel)
    uint32_t max_time_bits;             // rvb_flatten: latest attenuated time
    uint32_t pad1_;
    uint32_t trace_range[2];            // float bits: time range of the traced diffuse impulses (shadow_kernel)
    uint32_t live_count;                // traced diffuse impulses that carry volume (live_sum_kernel behind the shadow kernel; right behind the range)
    uint32_t image_item_count;          // entries of the image-source work list (image_plan_kernel)
    uint32_t pad2_[4];
    rvb_impulse direct;
};
static_assert(offsetof(SmallBlock, candidate_count) == 0 && offsetof(SmallBlock, executed) == 8, "small block layout");
static_assert(offsetof(SmallBlock, range) == 16 && offsetof(SmallBlock, max_time_bits) == 24, "small block layout");
static_assert(offsetof(SmallBlock, trace_range) == 32 && offsetof(SmallBlock, live_count) == 40, "small block layout");
static_assert(offsetof(SmallBlock, image_item_count) == 44, "small block layout");
static_assert(offsetof(SmallBlock, direct) == 64 && sizeof(SmallBlock) == 128, "small block layout");
const size_t kFirstCandidates = 32;

// The host mirror of `small`, fetched once per trace together with the first few image-source candidates (usually all of them).
// One PINNED block: a device-to-host copy into pageable memory is staged by the runtime and blocks the host per call (three
// round trips of 30-160 us between the shadow kernel and the binning stage in a kernel trace); into pinned memory the copies
// are asynchronous and the host waits once.
struct TraceHostBlock {
    SmallBlock small;
    rvb_image_candidate first[kFirstCandidates];
    uint32_t hrtf_range[2];                     // where the HRTF time-range pass lands (rvb_ir_time_range_begin)
    // set by live_compact_kernel, straight into this pinned word, if a live list ever held more than its count allowed
    // (the excess was dropped); fetch_small reports it
    uint32_t live_overflow;
};
static_assert(offsetof(TraceHostBlock, first) == sizeof(SmallBlock), "host block layout: the candidates right behind the small block");
static_assert(offsetof(TraceHostBlock, hrtf_range) == sizeof(SmallBlock) + kFirstCandidates * sizeof(rvb_image_candidate), "host block layout");
static_assert(offsetof(TraceHostBlock, live_overflow) == offsetof(TraceHostBlock, hrtf_range) + 8, "host block layout: the word handed to live_compact_kernel");

// Source directivity, the device half over SourceState (source_state.h): what the last upload put on the device — it stays there
// whatever is set afterwards, until the next trace or re-shade uploads: a kept trace may reflect it —, and the staging blocks it went through.
struct SourceDirectivity : SourceState {
    DevBuf patterns_dev;                        // [npatterns] SourcePatternDev
    StagedBlock patterns_stage;
    DevBuf table_dev;                           // [RVB_HRTF_ROWS][8] floats (the zero row last), then the bases, in one block
    DevBuf gains;                               // ray_gains of the last launch that applied the table (apply_source_patterns sizes it)
    StagedBlock table_stage;
    // source.hip: whatever has changed since the last upload, up in stream order
    hipError_t upload(hipStream_t stream);
    const SourcePatternDev * patterns_on_device() const { return patterns_dev.as<SourcePatternDev>(); }
    // the table on the device as the launchers take it, for `orientations` (SourceShading::table_orientations) of them
    SourceTableDev table_on_device(uint32_t orientations) const
    {
        SourceTableDev d;
        d.table = table_dev.as<const float>();
        d.bases = reinterpret_cast<const float4 *>(d.table + (size_t) RVB_HRTF_ROWS * 8);
        d.basis_stride = orientations > 1 ? 3u : 0u;
        d.ray_gains = gains.as<float>();
        return d;
    }
    // the gain rows of pair `pair`'s rays, as source_table_rays_kernel left them
    const float * gains_of_pair(uint64_t pair, uint64_t rays_per_pair) const { return gains.as<const float>() + pair * rays_per_pair * 8; }
};

// The pinned staging block of a launch of several pairs, 40 * npairs bytes: [npairs] float4 microphones (x y z 0), [npairs] float4
// sources, then [npairs][2] initial time-range words, 0xFFFFFFFF / 0.  The layout is written here and nowhere else.
struct PairBlock {
    static size_t mic_bytes(uint64_t npairs) { return 4 * npairs * sizeof(float); }
    static size_t geom_bytes(uint64_t npairs) { return 2 * mic_bytes(npairs); }          // microphones, then sources
    static size_t range_bytes(uint64_t npairs) { return 2 * npairs * sizeof(uint32_t); }
    static size_t bytes(uint64_t npairs) { return geom_bytes(npairs) + range_bytes(npairs); }
    static const void * ranges(const void * block, uint64_t npairs) { return static_cast<const char *>(block) + geom_bytes(npairs); }
    // mics, sources: [npairs][3]
    static void fill_mics(void * block, const float * mics, uint64_t npairs)
    {
        float * geom = static_cast<float *>(block);
        for (uint64_t p = 0; p < npairs; ++p)
            for (int i = 0; i < 3; ++i) geom[4 * p + i] = mics[3 * p + i];
    }
    static void fill(void * block, const float * mics, const float * sources, uint64_t npairs)
    {
        std::memset(block, 0, geom_bytes(npairs));
        fill_mics(block, mics, npairs);
        fill_mics(static_cast<char *>(block) + mic_bytes(npairs), sources, npairs);
        uint32_t * init = static_cast<uint32_t *>(const_cast<void *>(ranges(block, npairs)));
        for (uint64_t p = 0; p < npairs; ++p) { init[2 * p] = 0xFFFFFFFFu; init[2 * p + 1] = 0u; }
    }
};

// The per-pair arrays of a launch of several pairs (rvb_trace_pairs; a launch of one pair uses the small block and stages nothing):
// geometry, direct path and time range per pair live in arrays of their own, staged through pinned memory and copied in stream
// order — no host synchronisation in front of the launch; the block is written again only after the copies of the previous launch
// have left it.  Beside them their host mirrors and, for any number of pairs, the microphones of the last launch.
struct PairLaunch {
    // mics + sources [2 * npairs] float4, direct [npairs] rvb_impulse, ranges [npairs][2] and behind them the live counts [npairs]
    // (live_sum_kernel, shadow_kernels.hip)
    DevBuf geom, direct, range;
    StagedBlock block;                          // PairBlock
    std::vector<float> mics_host;               // [npairs][3]
    std::vector<rvb_impulse> direct_mirror;     // fetched once per trace (fetch_small)
    std::vector<uint32_t> range_mirror;         // ranges, then live counts
    static size_t live_bytes(uint64_t npairs) { return npairs * sizeof(uint32_t); }

    // A launch of npairs > 1 pairs: the block filled and copied up, and the four pointers of `a` that then point here.
    hipError_t stage(const float * mics, const float * sources, uint64_t npairs, hipStream_t stream, TraceArgs & a)
    {
        if (npairs <= 1) return hipSuccess;
        hipError_t e = block.acquire(PairBlock::bytes(npairs), stream);
        if (e != hipSuccess) return e;
        PairBlock::fill(block.block.p, mics, sources, npairs);
        if ((e = geom.ensure(PairBlock::geom_bytes(npairs))) != hipSuccess) return e;
        if ((e = direct.ensure(npairs * sizeof(rvb_impulse))) != hipSuccess) return e;
        if ((e = range.ensure(PairBlock::range_bytes(npairs) + live_bytes(npairs))) != hipSuccess) return e;
        if ((e = hipMemcpyAsync(geom.p, block.block.p, PairBlock::geom_bytes(npairs), hipMemcpyHostToDevice, stream)) != hipSuccess) return e;
        if ((e = reset_ranges(npairs, stream)) != hipSuccess) return e;
        if ((e = hipMemsetAsync(range.as<char>() + PairBlock::range_bytes(npairs), 0, live_bytes(npairs), stream)) != hipSuccess) return e;
        a.pair_mics = geom.as<float4>();
        a.pair_sources = geom.as<float4>() + npairs;
        a.direct = direct.as<rvb_impulse>();
        a.time_range = range.as<uint32_t>();
        return hipSuccess;
    }
    // rvb_relisten on a kept launch of npairs > 1 pairs: new microphones through the block — stage() sized it for this many pairs, and
    // its sources and initial ranges stay —, copied in stream order (a kernel of the previous call may still read `geom`), and the
    // direct slots back at zero.  reset_ranges, which follows, records the event.
    hipError_t restage_mics(const float * mics, uint64_t npairs, hipStream_t stream)
    {
        hipError_t e = block.acquire(PairBlock::mic_bytes(npairs), stream);
        if (e != hipSuccess) return e;
        PairBlock::fill_mics(block.block.p, mics, npairs);
        if ((e = hipMemcpyAsync(geom.p, block.block.p, PairBlock::mic_bytes(npairs), hipMemcpyHostToDevice, stream)) != hipSuccess) return e;
        return hipMemsetAsync(direct.p, 0, npairs * sizeof(rvb_impulse), stream);
    }
    // the time ranges back at "nothing seen", from the initial ranges that are still in the block: its next writer waits for the event recorded here
    hipError_t reset_ranges(uint64_t npairs, hipStream_t stream)
    {
        hipError_t e = hipMemcpyAsync(range.p, PairBlock::ranges(block.block.p, npairs), PairBlock::range_bytes(npairs), hipMemcpyHostToDevice, stream);
        return e == hipSuccess ? block.record(stream) : e;
    }
    // direct paths, time ranges and live counts into their host mirrors; the caller synchronises
    hipError_t fetch(uint64_t npairs, hipStream_t stream)
    {
        direct_mirror.resize(npairs);
        range_mirror.resize(3 * npairs);
        hipError_t e = hipMemcpyAsync(direct_mirror.data(), direct.p, npairs * sizeof(rvb_impulse), hipMemcpyDeviceToHost, stream);
        return e == hipSuccess ? hipMemcpyAsync(range_mirror.data(), range.p, PairBlock::range_bytes(npairs) + live_bytes(npairs), hipMemcpyDeviceToHost, stream) : e;
    }
    const rvb_impulse & direct_of(uint64_t pair) const { return direct_mirror[pair]; }
    const uint32_t * range_of(uint64_t pair) const { return range_mirror.data() + 2 * pair; }
    uint32_t live_of(uint64_t npairs, uint64_t pair) const { return range_mirror[2 * npairs + pair]; }
    const float * mic_of(uint64_t pair) const { return mics_host.data() + 3 * pair; }
};

// The trace stage, the device half over TraceState (trace_state.h): the buffers a trace writes, those of its record grouping, the
// per-pair arrays, the pinned host mirror, and the selected pair's results — the fork between the small block (one pair) and the
// per-pair arrays (several) is written here, once per quantity.
struct TraceStage : TraceState {
    DevBuf impulses, early, candidates, small, stamps;          // small: one SmallBlock
    DevBuf image_items;                         // work list of the image-source check kernel
    DevBuf live_stripes;                        // TraceArgs::live_stripes: zeroed when allocated, put back to zero by every launch that adds to it
    DevBuf sort_keys, sort_scratch, sort_order, group_temp;     // the record grouping of a trace
    bool stamps_cleared = false;
    PairLaunch pairs;                           // the per-pair arrays of the last launch, their host mirrors, its microphones
    PinnedBuf host_block;
    TraceHostBlock * host = nullptr;            // host_block, zeroed (rvb_create)

    SmallBlock * small_dev() const { return small.as<SmallBlock>(); }
    hipError_t create()
    {
        hipError_t e = small.ensure(sizeof(SmallBlock));
        if (e == hipSuccess) e = host_block.ensure(sizeof(TraceHostBlock));
        if (e == hipSuccess) std::memset(host = host_block.as<TraceHostBlock>(), 0, sizeof(TraceHostBlock));
        return e;
    }
    static size_t early_bytes(uint64_t nrays) { return (size_t) nrays * 9 * sizeof(uint32_t); }
    // entries of the image work list: a (ray, bounce) per candidate slot and one per pair
    static size_t image_entries(uint64_t nrays, uint64_t npairs) { return (size_t) nrays * 9 + npairs; }
    // The buffers of a launch of nrays rays in npairs pairs; new stripes start at zero.
    hipError_t ensure_launch(uint64_t nrays, uint64_t npairs, uint64_t nreflections, hipStream_t stream)
    {
        hipError_t e;
        if ((e = impulses.ensure((size_t) nrays * nreflections * sizeof(rvb_impulse))) != hipSuccess) return e;
        if ((e = early.ensure(early_bytes(nrays))) != hipSuccess) return e;
        if ((e = candidates.ensure((size_t) nrays * 9 * sizeof(rvb_image_candidate))) != hipSuccess) return e;
        if ((e = image_items.ensure(image_entries(nrays, npairs) * 3 * sizeof(uint32_t))) != hipSuccess) return e;      // (ray, bounce) entries, then a state word each
        const size_t stripe_bytes = (size_t) RVB_LIVE_STRIPES * npairs * sizeof(uint32_t);
        if (stripe_bytes <= live_stripes.cap) return hipSuccess;
        if ((e = hipStreamSynchronize(stream)) != hipSuccess) return e;          // (a launch that still adds to the old block)
        if ((e = live_stripes.ensure(stripe_bytes)) != hipSuccess) return e;
        return hipMemsetAsync(live_stripes.p, 0, stripe_bytes, stream);
    }
    // ... and where its kernels find them: one pair's results in the small block (PairLaunch::stage repoints those of several pairs)
    void point(TraceArgs & a, uint64_t nrays, uint64_t npairs) const
    {
        SmallBlock * s = small_dev();
        a.impulses = impulses.as<rvb_impulse>();
        a.early = early.as<uint32_t>();
        a.candidates = candidates.as<rvb_image_candidate>();
        a.candidate_count = &s->candidate_count;
        a.image_items = reinterpret_cast<ImageItem *>(image_items.p);
        a.image_state = image_items.as<uint32_t>() + image_entries(nrays, npairs) * 2;
        a.image_item_count = &s->image_item_count;
        a.direct = &s->direct;
        a.pair_mics = nullptr;
        a.pair_sources = nullptr;
        a.executed = &s->executed;
        a.time_range = s->trace_range;
        a.live_stripes = live_stripes.as<uint32_t>();
    }

    // The selected pair's results.  The host's need fetch_small first.
    const rvb_impulse & direct() const { return npairs() > 1 ? pairs.direct_of(pair()) : host->small.direct; }
    const rvb_impulse * direct_slot() const { return npairs() > 1 ? pairs.direct.as<rvb_impulse>() + pair() : &small_dev()->direct; }
    const uint32_t * diffuse_range() const { return npairs() > 1 ? pairs.range_of(pair()) : host->small.trace_range; }     // float bits [2]
    uint32_t live_count() const { return npairs() > 1 ? pairs.live_of(npairs(), pair()) : host->small.live_count; }
    const float * mic() const { return pairs.mic_of(pair()); }
};

struct Timing { std::string name; hipEvent_t start, stop; };       // (events of the context's pool)

// A kept trace, the device half over KeptState (kept_state.h; rvb_keep_paths; kept.hip works from it).  While keeping is on a trace
// leaves, beside its results, a 16-byte side record per (ray, bounce) (SideRecord of csrc/kept_tiles.h) and the INIT_DIST of every
// image impulse (csrc/reshade_kernels.hip), and trace_args() remembers its kernel arguments:
// microphones, sources, air, ray offset and every buffer of the launch.  With RVB_KEEP_LISTENER it leaves an 8-byte listener record per
// (ray, bounce) too, {own-plane threshold, triangle} (csrc/relisten_kernels.hip).  The buffers exist only while keeping is on.
// The kept state is valid while TraceState::traced() holds and nothing has voided it: a trace voids it first (trace_begins) and takes it last (take).
// The grouping order of the records is kept where the trace left it: `sort_order` is written by the record grouping of a trace and by
// nothing else (the binning stages sort in SortBuffers), and the next trace voids the kept state before it
// regroups; trace_args().sort_order points there (null: the trace grouped nothing).
struct KeptTrace : KeptState {
    static_assert(kListenerBit == RVB_KEEP_LISTENER, "KeptState::ask reads the listener bit of rvb_keep_paths");
    // everything on the device that keeping owns.  `surfaces` is the table of the last rvb_reshade: the scene (which may be shared)
    // keeps its own; uploaded in stream order through surfaces_stage, as the source patterns are.  `grad_scratch`: the result and the
    // partial tables of rvb_reshade_grad (csrc/reshade_grad_kernels.hip).  `map_scratch`: the term rows of rvb_reshade_grad_map, 64 bytes per
    // record of a pair, and behind them the fold's partials (csrc/reshade_grad_map_kernels.hip); allocated by its first call.
    // `source_scratch`: the binary64 sums, departure vectors, partials and result of rvb_source_grad / rvb_source_grad_images
    // (csrc/source_grad.hip); allocated by the first call that asks for a pattern gradient or takes images.
    struct Buffers {
        DevBuf paths, image_dist, listen, surfaces, grad_scratch, map_scratch, source_scratch;
        bool any() const { return paths.p || image_dist.p || listen.p || surfaces.p || grad_scratch.p || map_scratch.p || source_scratch.p; }
    } dev;
    static_assert(sizeof(Buffers) == 7 * sizeof(DevBuf), "any() names every buffer");
    StagedBlock surfaces_stage;

    // What a launch of nrays rays in npairs pairs keeps beside its results (nothing while keeping is off), and where its kernels put it.
    hipError_t ensure_launch(uint64_t nrays, uint64_t npairs, uint64_t nreflections)
    {
        if (!keeping()) return hipSuccess;
        hipError_t e;
        if ((e = dev.paths.ensure((size_t) nrays * nreflections * sizeof(float4))) != hipSuccess) return e;
        if ((e = dev.image_dist.ensure(TraceStage::image_entries(nrays, npairs) * sizeof(float))) != hipSuccess) return e;
        return keeping_listener() ? dev.listen.ensure((size_t) nrays * nreflections * sizeof(uint2)) : hipSuccess;
    }
    float * image_dist_for_launch() const { return keeping() ? dev.image_dist.as<float>() : nullptr; }
    uint2 * listen_for_launch() const { return keeping_listener() ? dev.listen.as<uint2>() : nullptr; }

    // `a` with `source` wrote the records last: a trace's shadow kernel, the re-shade kernels
    void note_shading(const TraceArgs & a, const SourceShading & source)
    {
        shaded_surfaces_ = a.scene.surfaces;
        for (int i = 0; i < 8; ++i) shaded_air_[i] = a.air[i];
        shaded_source_ = source;
    }
    // a trace with the arguments `a` is complete
    void take(const TraceArgs & a, const SourceShading & source)
    {
        trace_taken();
        if (valid()) { args_ = a; note_shading(a, source); }
    }
    // rvb_relisten has rewritten the records for this microphone: "the kept trace stays valid and is now that of the new microphone(s)"
    // (those of several pairs are in PairLaunch::geom)
    void relistened(const float mic[3]) { for (int i = 0; i < 3; ++i) args_.mic[i] = mic[i]; }
    // the kept trace's own arguments ...
    const TraceArgs & trace_args() const { return args_; }
    // ... and under the table and the air that the records reflect now
    TraceArgs shaded_args() const
    {
        TraceArgs a = args_;
        a.scene.surfaces = shaded_surfaces_;
        for (int i = 0; i < 8; ++i) a.air[i] = shaded_air_[i];
        return a;
    }
    // the source directivity that the records reflect now (pattern, table or nothing) ...
    const SourceShading & shaded_source() const { return shaded_source_; }
    // ... and its pattern for pair `pair`: one pattern serves every pair, several are one per pair.  false: no pattern shaded the records.
    bool shaded_pattern(uint64_t pair, SourcePatternDev & out) const
    {
        const std::vector<SourcePatternDev> & patterns = shaded_source_.patterns;
        out = patterns.empty() ? SourcePatternDev{} : patterns[patterns.size() > 1 ? pair : 0];
        return !patterns.empty();
    }
    // frees the device buffers (the caller has synchronised the streams whose work may still use them)
    void release() { Buffers freed(std::move(dev)); }

private:
    TraceArgs args_ = {};
    // what the records reflect right now — the kept trace's table, air and source directivity, or those of the last rvb_reshade —:
    // where rvb_reshade_grad takes its derivatives and what rvb_relisten shades with
    const rvb_surface * shaded_surfaces_ = nullptr;
    float shaded_air_[8] = {};
    SourceShading shaded_source_;
};

// The merged image list made on the device, the device half over MergedState (merged_state.h; rvb_ir_configure_*_merged, images.hip).
// Which candidate wins each key of rvb_merge_images depends on geometry and microphone only: `winners` holds, per output impulse in the merge's order, the device position of the candidate
// it is copied from, or RVB_IMAGE_WINNER_DIRECT for the pair's direct slot.  Made once per (trace or relisten, pair, remove_direct) from
// one download of the candidates, uploaded once; a re-shade, a source setter and rvb_ir_select_pair leave it alone.
struct MergedImages : MergedState {
    DevBuf winners;                              // [count()] uint32_t
    DevBuf grad_scratch;                         // rvb_reshade_grad_images: the term rows, then the result
};

// The impulse-response stage, the device half over IrState (ir_state.h): the model and the image list of the configuration, the HRTF
// table image, and the stage's scratch.
struct IrStage : IrState {
    AttenuationModel model;
    DevBuf images;                               // [nimages()] rvb_impulse
    std::vector<rvb_impulse> images_host;        // its host copy; of a list gathered on the device once a reader has asked (ir_images_on_host)
    DevBuf hrtf_table;
    DevBuf speakers;                             // more than 8 speakers: AttenuationModel::speaker_table, uploaded in stream order at configure
    std::vector<float4> speakers_host;
    DevBuf acc, hist, scratch_in, scratch_out;
    DevBuf flat_in;                              // rvb_flatten's upload: a buffer of its own, so that no other entry point overwrites it between a size query and the fill
};

// sort.hip's: the (key, value) list of a binning pass in keys_a / vals_a, sorted into keys_b / vals_b with bin_starts beside it
// (sort_and_bin).  Whoever fills them calls ensure_sort_buffers first; what they hold is IrState::tenant.  own_*: csrc/radix_sort.hip's
// tile counters and intermediate (key, value) pair.
// live: the exact mode's live list (live_list below) — LiveHeader, then a word per tile of RVB_LIVE_TILE records.
struct SortBuffers {
    DevBuf keys_a, keys_b, vals_a, vals_b, temp, bin_starts;
    DevBuf own_temp, own_keys, own_values;
    DevBuf live;
};

struct rvb_ctx {
    int device = 0;
    // (declared first: destroyed last, after everything that work on them may use)
    Stream stream;
    Stream side_stream;                         // image_kernel runs here, beside the record grouping
    Stream export_stream;                       // rvb_copy_to_pinned_host_async: results leave for the host beside the next trace
    Event export_ready;
    Event path_done, side_done;
    Event prep_done, group_done;                // rvb_trace_group: this context's fills are enqueued / the group's path kernel is
    std::string error;
    std::string arch;
    int compute_units = 0;
    uint64_t hbm_bytes = 0;

    ContextScene scene;

    // rays + trace results
    DevBuf directions_own;
    const float4 * directions = nullptr;
    uint64_t nrays = 0;
    uint32_t concurrent_traces = 1;             // rvb_set_concurrent_traces
    uint32_t path_lanes = 0;                    // rvb_set_path_lanes: 0 = chosen per launch (rvb_path_lanes_for)
    // the last trace: npairs() (source, microphone) pairs x nrays rays each; the IR stage works on one pair's slice at a time
    TraceStage trace;
    SourceDirectivity source;                   // rvb_set_source_pattern / rvb_set_source_table: what is set and what is on the device
    KeptTrace kept;                              // rvb_keep_paths: what rvb_reshade, rvb_reshade_grad and rvb_relisten work from
    // rvb_decay_* (csrc/decay.hip): per-tile sums and carries, per-row windows and results; nothing else lives here, so the decay calls
    // leave the sort buffers, the IR configuration and a prepared exact list alone
    DevBuf decay_scratch;
    // rvb_window_* (csrc/window.hip): the select's state and tables, the listed entries, a key per record; a block of its own for the
    // same reason
    DevBuf window_scratch;
    // rvb_mtf* (csrc/speech.hip): per-tile sums, per-row results and coefficients; a block of its own for the same reason
    DevBuf speech_scratch;
    std::vector<Timing> timings;
    std::vector<Event> event_pool;
    size_t events_used = 0;
    bool timing_failed = false;                 // an event could not be created: timings are dropped, the work itself is unaffected
    bool timing_open = false;

    IrStage ir;                                 // the impulse-response stage: configuration, model, image list, what the sort buffers hold
    MergedImages merged;
    SortBuffers sort;

    // staged host copies (rvb_copy_to_host / rvb_copy_to_device): per worker thread a stream and two pinned bounce buffers
    struct CopyLane { Stream stream; PinnedBuf pinned[2]; Event done[2]; };
    std::vector<CopyLane> copy_lanes;

    ~rvb_ctx()
    {
        (void) hipSetDevice(device);
        for (hipStream_t s : {stream.h, side_stream.h, export_stream.h})
            if (s) (void) hipStreamSynchronize(s);
    }

    hipEvent_t next_event()
    {
        if (events_used == event_pool.size()) {
            Event e;
            if (hipEventCreate(&e.h) != hipSuccess) { timing_failed = true; return nullptr; }
            event_pool.push_back(std::move(e));
        }
        return event_pool[events_used++];
    }
    void begin_timing(const char * name, hipStream_t on = nullptr)
    {
        Timing t;
        t.name = name;
        t.start = next_event();
        t.stop = next_event();
        timing_open = t.start && t.stop;
        if (!timing_open) return;
        (void) hipEventRecord(t.start, on ? on : stream.h);
        timings.push_back(t);
    }
    void end_timing(hipStream_t on = nullptr) { if (timing_open) (void) hipEventRecord(timings.back().stop, on ? on : stream.h); timing_open = false; }
    void reset_timings() { timings.clear(); events_used = 0; }
    // From here on the results are no longer the last trace's (rvb_reshade or rvb_relisten is about to rewrite them): what the host
    // has fetched of them, their live count and what the IR stage has prepared from them is void, and the first pair is selected.
    void void_fetched_results() { trace.records_rewritten(); ir.drop_configuration(); }
    // The trace is gone (rvb_set_scene, rvb_share_scene, rvb_set_directions*, a trace that begins): nrays or the scene no longer describe
    // the records in `impulses`, so an IR configuration or a prepared exact list made for them must not be used either.
    void void_trace() { trace.inputs_changed(); ir.drop_configuration(); merged.void_list(); }
};

// ctx == NULL: the text of a failed rvb_create, per thread (rvb_last_error(NULL))
int fail(rvb_ctx * ctx, int code, const std::string & what);
#define RVB_BIND(ctx) RVB_HIP(fail, ctx, hipSetDevice((ctx)->device))

// the diffuse impulses the IR stage works on: the slice of the pair chosen with rvb_ir_select_pair (pair 0 of 1 otherwise)
inline const rvb_impulse * ir_diffuse(const rvb_ctx * ctx)
{
    return ctx->trace.impulses.as<rvb_impulse>() + ctx->trace.pair() * ctx->nrays * ctx->trace.nreflections();
}
// ... and how many of them, and of the images, the configuration's `which` takes
struct IrCounts { uint64_t ndiffuse, nimages; };
inline IrCounts ir_counts(const rvb_ctx * ctx)
{
    return {(ctx->ir.which() & RVB_IR_DIFFUSE) ? ctx->nrays * ctx->trace.nreflections() : 0, (ctx->ir.which() & RVB_IR_IMAGES) ? ctx->ir.nimages() : 0};
}

inline uint64_t bins_for(float max_time, float predelay, float sample_rate)
{
    const float t = max_time > predelay ? max_time - predelay : 0.0f;   // rayverb.h:89
    return (uint64_t) (roundf(t * sample_rate) + 1);                    // rayverb.cpp:57
}

inline int key_bits_for(uint64_t nbins)
{
    int bits = 1;
    while (bits < 32 && (1ull << bits) < nbins + 1)
        ++bits;
    return bits;
}

// runs of 2^shift neighbouring keys ("coarse bins") that cover the keys 0 .. nkeys-1
inline uint64_t coarse_keys(uint64_t nkeys, int shift)
{
    return (nkeys + (1ull << shift) - 1) >> shift;
}

// trace.hip: one synchronising 128-byte read per trace serves candidate count, direct path, time range, bounce count
int fetch_small(rvb_ctx * ctx);
// trace.hip: the steps of a trace that kept.hip replays (described where they are defined)
int reset_time_ranges(rvb_ctx * ctx, const TraceArgs & a);
int launch_images_beside(rvb_ctx * ctx, TraceArgs & a);
int launch_shadow_behind_images(rvb_ctx * ctx, const TraceArgs & a, const SourceShading & source, bool gains_stand = false);
// source.hip: what a trace and a re-shade do about the source directivity (described where they are defined)
int check_source_counts(rvb_ctx * ctx, const char * who, uint64_t npairs);
int apply_source_patterns(rvb_ctx * ctx, const TraceArgs & a, const SourceShading & source, bool gains_stand = false);
// kept.hip: what the gradient passes over the kept records share (described where they are defined) — `a` for such a pass, what a pass
// takes beside it, and the refusals of rvb_reshade_grad under the name of the call `who` (its own null arguments are that call's to refuse)
TraceArgs for_record_pass(const rvb_ctx * ctx, TraceArgs a);
ReshadeGradArgs grad_args(const rvb_ctx * ctx, float predelay, float sample_rate, uint64_t nbins);
int reshade_grad_refusals(rvb_ctx * ctx, const char * who, float predelay, float sample_rate, uint64_t nbins);
// images.hip: the same for rvb_reshade_grad_images — its refusals, and what its kernel takes (the weights read in place)
int reshade_grad_images_refusals(rvb_ctx * ctx, const char * who, float predelay, float sample_rate, uint64_t nbins);
ImageGradArgs image_grad_args(const rvb_ctx * ctx, const TraceArgs & a, float predelay, float sample_rate, uint64_t nbins, const void * d_weights);
// kept.hip: the tail of a per-surface gradient — waits for the stream, then the nsurfaces * 16 + 8 floats at d_out into the caller's arrays
int download_surface_gradient(rvb_ctx * ctx, const float * d_out, rvb_surface * grad_surfaces, float grad_air[8]);

// trace.hip: the merge rule of rvb_merge_images on its own — per output impulse, in the merge's (std::map key) order, the position in
// `candidates` of the candidate it is copied from, or RVB_IMAGE_WINNER_DIRECT for the direct slot.  RVB_ERR_INVALID for a slot out of range.
int merge_image_winners(const rvb_image_candidate * candidates, uint64_t ncandidates, bool have_direct, bool remove_direct, std::vector<uint32_t> & winners);
// ir.hip: the halves of rvb_ir_configure_speakers / rvb_ir_configure_hrtf — the model; what both refuse; the image list and the
// configuration's state (gathered: the caller enqueues the gather into ctx->ir.images, no host list is uploaded) — and the host copy of the
// image list for the readers that need one; the HRTF table image and the model over it, which flatten.hip's one-ear calls use too
int ir_speaker_model(rvb_ctx * ctx, const float mic[3], const rvb_speaker * speakers, uint64_t nspeakers);
int ir_hrtf_model(rvb_ctx * ctx, const float mic[3], const float * table, const float facing[3], const float up[3]);
int ir_configure_refusals(rvb_ctx * ctx, int which);
int ir_configure_images(rvb_ctx * ctx, int which, const rvb_impulse * images, uint64_t nimages, bool gathered);
int ir_images_on_host(rvb_ctx * ctx);
int upload_hrtf_table(rvb_ctx * ctx, const float * table, int first_ear, int ears);
AttenuationModel hrtf_model(const rvb_ctx * ctx, const float mic[3], const float facing[3], const float up[3]);

// sort.hip
bool own_sort_enabled();
int own_sort(rvb_ctx * ctx, const uint32_t * keys, uint32_t value_base, uint64_t n, int begin_bit, int end_bit,
             uint32_t * keys_out, uint32_t * values_out, bool want_keys);
int ensure_sort_buffers(rvb_ctx * ctx, uint64_t n);
int sort_and_bin(rvb_ctx * ctx, uint64_t n, uint64_t nkeys, int key_bits, bool may_sort_own, int coarse_shift = 0);

#pragma GCC visibility pop
