// trace.hip — the trace of include/rvb_capi.h: buffers, fills and kernel arguments; the path kernel; everything after it; then what a
// trace leaves for the host (diffuse impulses, direct path, image-source candidates) and the image-source merge (its rule on its own:
// merge_image_winners, which images.hip shares).  The steps that a kept
// trace replays (kept.hip) come first: they are declared in ctx.h.  The source directivity is source.hip's; the stage's state, its
// buffers and the per-pair arrays of a launch are TraceStage's (ctx.h, over trace_state.h).
#include "ctx.h"

#include <algorithm>
#include <cstdlib>
#include <cstring>
#include <map>

// The diffuse time range(s) of a launch back at "nothing seen": 0xFFFFFFFF / 0, per pair.
int reset_time_ranges(rvb_ctx * ctx, const TraceArgs & a)
{
    if (a.npairs > 1) {
        RVB_HIP(fail, ctx, ctx->trace.pairs.reset_ranges(a.npairs, ctx->stream));
    } else {
        RVB_HIP(fail, ctx, hipMemsetAsync(a.time_range, 0xFF, 4, ctx->stream));
        RVB_HIP(fail, ctx, hipMemsetAsync(a.time_range + 1, 0, 4, ctx->stream));
    }
    return RVB_OK;
}

// The tail of a trace behind the kernel that left the work records (a path kernel; relisten_records_kernel of rvb_relisten), in two steps.
// image_kernel depends on that kernel only: it (latency-bound) runs on the side stream beside whatever the caller enqueues between the
// two steps; shadow_kernel, which rewrites the records image_kernel reads, waits for it.
int launch_images_beside(rvb_ctx * ctx, TraceArgs & a)
{
    RVB_HIP(fail, ctx, hipEventRecord(ctx->path_done, ctx->stream));
    RVB_HIP(fail, ctx, hipStreamWaitEvent(ctx->side_stream, ctx->path_done, 0));
    ctx->begin_timing("image_kernel", ctx->side_stream);
    a.scene.stamps = nullptr;
    rvb_launch_images(a, ctx->side_stream);
    ctx->end_timing(ctx->side_stream);
    RVB_HIP(fail, ctx, hipEventRecord(ctx->side_done, ctx->side_stream));
    a.scene.stamps = ctx->trace.stamps.as<unsigned long long>() + 16;
    return RVB_OK;
}

int launch_shadow_behind_images(rvb_ctx * ctx, const TraceArgs & a, const SourceShading & source, bool gains_stand)
{
    RVB_HIP(fail, ctx, hipStreamWaitEvent(ctx->stream, ctx->side_done, 0));
    ctx->begin_timing(rvb_shadow_lanes() == 2 ? "shadow_pair_kernel" : (rvb_shadow_lanes() == 1 ? "shadow_lane_kernel" : "shadow_kernel"));
    rvb_launch_shadow(a, ctx->stream);
    ctx->end_timing();
    RVB_HIP(fail, ctx, hipGetLastError());
    return apply_source_patterns(ctx, a, source, gains_stand);
}

namespace {

// A trace in three steps — buffers, fills and kernel arguments; the path kernel; everything after it — so that rvb_trace_group can put
// the path kernels of several contexts into ONE launch.
struct TracePlan {
    TraceArgs a;
    uint64_t npairs = 1, nrays = 0, nreflections = 0;
    int key_bits = 1;
};

int trace_prepare(rvb_ctx * ctx, const float * mics, const float * sources, uint64_t npairs, uint64_t nreflections,
                  const float air_coefficient[8], uint64_t ray_offset, uint64_t rays_in_flight, TracePlan & plan)
{
    if (!ctx->scene.have()) return fail(ctx, RVB_ERR_STATE, "rvb_trace: rvb_set_scene has not been called");
    if (!ctx->directions && ctx->nrays) return fail(ctx, RVB_ERR_STATE, "rvb_trace: no directions");
    if (nreflections >= (1ull << 31) || ctx->nrays * npairs * 9 >= (1ull << 32))
        return fail(ctx, RVB_ERR_CAPACITY, "rvb_trace: too many reflections or rays for one context");
    if (check_source_counts(ctx, "rvb_trace", npairs) != RVB_OK) return RVB_ERR_INVALID;
    const float * mic = mics, * source = sources;
    RVB_BIND(ctx);
    ctx->void_trace();                                // (until trace_finish: a failure below must not leave the last trace's results half reset)
    TraceStage & trace = ctx->trace;
    trace.begin();
    KeptTrace & kept = ctx->kept;
    kept.trace_begins();
    const uint64_t nrays = ctx->nrays * npairs;       // rays of this launch
    RVB_HIP(fail, ctx, trace.ensure_launch(nrays, npairs, nreflections, ctx->stream));
    RVB_HIP(fail, ctx, kept.ensure_launch(nrays, npairs, nreflections));       // rvb_keep_paths: what rvb_reshade and rvb_relisten need beside the results

    // reference rayverb.cpp:600-616: outputs start zero-filled — path_kernel writes every slot of the
    // impulse array itself (work record or zeros), so no 819 MB fill is needed here
    // (a probe that skips this 3.6 MB fill — the kernel trace of the pipeline shows it stretched to 0.7 ms beside a histogram's host copy, right in
    // front of the next path kernel — made the pipeline 2 % SLOWER, 4.52 -> 4.62 ms per IR, three alternating runs: the fills stay)
    SmallBlock * small = trace.small_dev();
    if (nrays) RVB_HIP(fail, ctx, hipMemsetAsync(trace.early.p, 0xFF, TraceStage::early_bytes(nrays), ctx->stream));
    RVB_HIP(fail, ctx, hipMemsetAsync(small, 0, sizeof(SmallBlock), ctx->stream));
    RVB_HIP(fail, ctx, hipMemsetAsync(&small->trace_range[0], 0xFF, 4, ctx->stream));

    TraceArgs & a = plan.a;
    a.scene = ctx->scene.dev;
    a.directions = ctx->directions;
    trace.point(a, nrays, npairs);
    a.npairs = (uint32_t) npairs;
    a.rays_per_pair = (uint32_t) ctx->nrays;
    a.image_dist = kept.image_dist_for_launch();
    RVB_HIP(fail, ctx, trace.pairs.stage(mics, sources, npairs, ctx->stream, a));       // several pairs per launch: four of them point to arrays per pair
    // record bucketing for coherent shadow rays (RVB_SHADOW_SORT=0 turns it off)
    static const bool sort_records = !(getenv("RVB_SHADOW_SORT") && getenv("RVB_SHADOW_SORT")[0] == '0');
    const uint64_t nrecords = nrays * nreflections;
    a.sort_keys = nullptr; a.sort_keys16 = nullptr; a.key_shift = 0; a.sort_order = nullptr;
    int key_bits = 1;
    while (key_bits < 32 && (1ull << key_bits) < ctx->scene.dev.ntris) ++key_bits;
    // The grouping only has to bring neighbouring triangles together: the top 16 bits of the leaf position are two
    // onesweep passes instead of three (C2, 17 key bits: grouping 0.66 -> 0.51 ms beside image_kernel, shadow_kernel +0.02 ms).
    if (sort_records && nrecords && nrecords < (1ull << 32) && ctx->scene.dev.ntris) {
        RVB_HIP(fail, ctx, trace.sort_keys.ensure(nrecords * 4));
        RVB_HIP(fail, ctx, trace.sort_scratch.ensure(nrecords * 4));
        RVB_HIP(fail, ctx, trace.sort_order.ensure(nrecords * 4));
        const size_t group_bytes = rvb_group_records_temp_bytes(ctx->nrays * nreflections);
        if (group_bytes == 0) return fail(ctx, RVB_ERR_HIP, "rvb_trace: radix sort size query failed");
        RVB_HIP(fail, ctx, trace.group_temp.ensure(group_bytes));
        // slots of escaped rays get key 0xFFFFFFFF from path_kernel: they land in the last bucket and the
        // shadow kernel skips them by their valid flag
        // 16-bit keys in 64-byte runs (the path stage, trace_kernels.hip: flush_key_run) whenever a ray's row divides into whole runs and rocPRIM sorts;
        // 32-bit keys, one store per record, otherwise (and for RVB_SORT=own)
        if (nreflections % 32 == 0 && !own_sort_enabled()) {
            a.sort_keys16 = trace.sort_keys.as<uint16_t>();
            a.key_shift = (uint32_t) std::max(0, key_bits - 16);
        } else {
            a.sort_keys = trace.sort_keys.as<uint32_t>();
        }
    }
    a.nrays = nrays;
    a.nreflections = (uint32_t) nreflections;
    a.stack_entries = ctx->scene.stack_need;
    a.lds_surfaces = rvb_lds_surfaces(ctx->scene.stack_need, ctx->scene.nsurfaces);
    // (rays_in_flight: what a group launch carries in all; 0 = this trace alone, times the caller's hint)
    a.path_lanes = ctx->path_lanes ? ctx->path_lanes : (rays_in_flight ? rvb_path_lanes_for(rays_in_flight, 1) : rvb_path_lanes_for(nrays, ctx->concurrent_traces));
    a.ray_offset = ray_offset;
    for (int i = 0; i < 3; ++i) { a.mic[i] = mic[i]; a.source[i] = source[i]; }
    for (int i = 0; i < 8; ++i) a.air[i] = air_coefficient[i];

    RVB_HIP(fail, ctx, ctx->source.upload(ctx->stream));

    // diagnostic builds (RVB_STAMPS): [0..15] path_kernel, [16..31] shadow_kernel
    RVB_HIP(fail, ctx, trace.stamps.ensure(32 * sizeof(unsigned long long)));
    // (zeroed per trace only where a diagnostic build may write them: one tiny fill kernel less on the stream of every shipped trace)
    static const bool stamps_on = getenv("RVB_STAMPS") != nullptr;
    if (stamps_on || !trace.stamps_cleared) {
        RVB_HIP(fail, ctx, hipMemsetAsync(trace.stamps.p, 0, 32 * sizeof(unsigned long long), ctx->stream));
        trace.stamps_cleared = true;
    }
    a.scene.stamps = trace.stamps.as<unsigned long long>();

    ctx->reset_timings();
    plan.npairs = npairs;
    plan.nrays = nrays;
    plan.nreflections = nreflections;
    plan.key_bits = key_bits;
    return RVB_OK;
}

int trace_finish(rvb_ctx * ctx, TracePlan & plan, const float * mics)
{
    TraceArgs & a = plan.a;
    const uint64_t npairs = plan.npairs, nrays = plan.nrays, nreflections = plan.nreflections;
    const int key_bits = plan.key_bits;
    static const int group_bits = getenv("RVB_SHADOW_SORT_BITS") ? atoi(getenv("RVB_SHADOW_SORT_BITS")) : 16;
    // image_kernel and the record grouping both depend on path_kernel only: the first (latency-bound) runs on the
    // side stream beside the second (bandwidth-bound); shadow_kernel, which rewrites the records image_kernel
    // reads, waits for both.
    int rc = launch_images_beside(ctx, a);
    if (rc != RVB_OK) return rc;
    if (ctx->kept.keeping()) {
        // rvb_keep_paths: what the shadow kernel is about to overwrite, while the image kernels read the same records on the side stream
        ctx->begin_timing("path_keep_kernel");
        rvb_launch_path_keep(a, ctx->kept.dev.paths.as<float4>(), ctx->kept.listen_for_launch(), ctx->stream);
        ctx->end_timing();
        RVB_HIP(fail, ctx, hipGetLastError());
    }
    if (a.sort_keys || a.sort_keys16) {
        ctx->begin_timing("record_sort_kernels");
        a.sort_order = ctx->trace.sort_order.as<uint32_t>();
        RVB_HIP(fail, ctx, hipGetLastError());
        // one grouping per pair (a pair's shadow rays share a microphone; records are [pair][ray][bounce])
        const uint64_t per_pair = ctx->nrays * nreflections;
        for (uint64_t p = 0; p < npairs; ++p) {
            if (a.sort_keys16) {
                // key16 = leaf position >> key_shift: its top group_bits bits are bits [end - group_bits, end) with end = min(16, key_bits)
                const int end = std::min(16, key_bits);
                RVB_HIP(fail, ctx, rvb_group_records16(ctx->trace.group_temp.p, ctx->trace.group_temp.cap, a.sort_keys16 + p * per_pair,
                                                       ctx->trace.sort_scratch.as<uint16_t>() + p * per_pair, a.sort_order + p * per_pair, per_pair,
                                                       (uint32_t) (p * per_pair), std::max(0, end - group_bits), end, ctx->stream));
            } else if (own_sort_enabled()) {
                const int rc = own_sort(ctx, a.sort_keys + p * per_pair, (uint32_t) (p * per_pair), per_pair, std::max(0, key_bits - group_bits), key_bits,
                                        ctx->trace.sort_scratch.as<uint32_t>() + p * per_pair, a.sort_order + p * per_pair, false);
                if (rc != RVB_OK) return rc;
            } else {
                RVB_HIP(fail, ctx, rvb_group_records(ctx->trace.group_temp.p, ctx->trace.group_temp.cap, a.sort_keys + p * per_pair,
                                                     ctx->trace.sort_scratch.as<uint32_t>() + p * per_pair, a.sort_order + p * per_pair, per_pair,
                                                     (uint32_t) (p * per_pair), std::max(0, key_bits - group_bits), key_bits, ctx->stream));
            }
        }
        ctx->end_timing();
    }
    const SourceShading source = ctx->source.shading();
    if ((rc = launch_shadow_behind_images(ctx, a, source)) != RVB_OK) return rc;
    ctx->kept.take(a, source);
    // the shadow stage leaves the live count; a directivity pass behind it (apply_source_patterns) may silence a record or turn it
    // into NaNs, and the count no longer bounds the live ones
    ctx->trace.finished(npairs, nrays, nreflections, a.ray_offset, source.off());
    ctx->ir.drop_configuration();
    ctx->trace.pairs.mics_host.assign(mics, mics + 3 * npairs);
    return RVB_OK;
}

// the name a path launch is timed under: the kernel that ran (the path stage, csrc/trace_kernels.hip: rvb_path_lanes_for)
const char * path_kernel_name(uint32_t lanes) { return lanes == 1 ? "path_lane_kernel" : (lanes == 2 ? "path_pair_kernel" : "path_kernel"); }

int trace_common(rvb_ctx * ctx, const float * mics, const float * sources, uint64_t npairs, uint64_t nreflections,
                 const float air_coefficient[8], uint64_t ray_offset)
{
    TracePlan plan;
    int rc = trace_prepare(ctx, mics, sources, npairs, nreflections, air_coefficient, ray_offset, 0, plan);
    if (rc != RVB_OK) return rc;
    ctx->begin_timing(path_kernel_name(plan.a.path_lanes));
    rvb_launch_path(plan.a, ctx->stream);
    ctx->end_timing();
    return trace_finish(ctx, plan, mics);
}

bool by_ray_and_slot(const rvb_image_candidate & x, const rvb_image_candidate & y) { return x.ray != y.ray ? x.ray < y.ray : x.slot < y.slot; }

}  // namespace

// one synchronising 128-byte read per trace serves candidate count, direct path, time range, bounce count
int fetch_small(rvb_ctx * ctx)
{
    TraceStage & trace = ctx->trace;
    if (trace.fetched())
        return RVB_OK;
    RVB_HIP(fail, ctx, hipMemcpyAsync(&trace.host->small, trace.small.p, sizeof(SmallBlock), hipMemcpyDeviceToHost, ctx->stream));
    if (trace.rays())          // capacity rays * 9 >= 32 entries unless there are fewer than 4 rays
        RVB_HIP(fail, ctx, hipMemcpyAsync(trace.host->first, trace.candidates.p,
                                          std::min(sizeof(trace.host->first), (size_t) trace.rays() * 9 * sizeof(rvb_image_candidate)),
                                          hipMemcpyDeviceToHost, ctx->stream));
    if (trace.npairs() > 1)    // per-pair direct paths and time ranges
        RVB_HIP(fail, ctx, trace.pairs.fetch(trace.npairs(), ctx->stream));
    RVB_HIP(fail, ctx, hipStreamSynchronize(ctx->stream));
    if (trace.host->live_overflow) {           // (the lists behind this point are sound again: the word is reported once)
        trace.host->live_overflow = 0;
        return fail(ctx, RVB_ERR_HIP, "internal error: an exact-mode list held more live impulses than the trace had counted; the histogram made from it lacks the excess");
    }
    trace.small_fetched();
    return RVB_OK;
}

int merge_image_winners(const rvb_image_candidate * candidates, uint64_t ncandidates, bool have_direct, bool remove_direct, std::vector<uint32_t> & winners)
{
    // reference rayverb.cpp:654-676: for each ray j and k = 1..10 the key is the first k entries of
    // the ray's index row; inserted if absent when k == 1 or the last entry is non-zero.  Entries
    // are zero except where a candidate exists, so rows are rebuilt from the candidates alone.
    std::vector<uint32_t> sorted((size_t) ncandidates);
    for (size_t i = 0; i < sorted.size(); ++i) sorted[i] = (uint32_t) i;
    std::sort(sorted.begin(), sorted.end(), [&](uint32_t x, uint32_t y) { return by_ray_and_slot(candidates[x], candidates[y]); });
    std::map<std::vector<unsigned long>, uint32_t> tally;
    if (have_direct)
        tally[std::vector<unsigned long>(1, 0)] = RVB_IMAGE_WINNER_DIRECT;      // k == 1: key {0} from ray 0
    size_t i = 0;
    while (i < sorted.size()) {
        size_t j = i;
        unsigned long row[RVB_NUM_IMAGE_SOURCE] = {0};
        while (j < sorted.size() && candidates[sorted[j]].ray == candidates[sorted[i]].ray) {
            const rvb_image_candidate & c = candidates[sorted[j]];
            if (c.slot == 0 || c.slot >= RVB_NUM_IMAGE_SOURCE)
                return RVB_ERR_INVALID;
            row[c.slot] = c.index;
            ++j;
        }
        for (size_t c = i; c < j; ++c) {
            std::vector<unsigned long> key(row, row + candidates[sorted[c]].slot + 1);
            if (tally.find(key) == tally.end())
                tally[key] = sorted[c];
        }
        i = j;
    }
    if (remove_direct)
        tally.erase(std::vector<unsigned long>(1, 0));          // rayverb.cpp:695-696
    winners.clear();
    winners.reserve(tally.size());
    for (const auto & kv : tally)
        winners.push_back(kv.second);
    return RVB_OK;
}

extern "C" {

int rvb_trace_group(rvb_ctx ** ctxs, uint64_t count, const float * mics, const float * sources, uint64_t nreflections,
                    const float air_coefficient[8], const uint64_t * ray_offsets)
{
    if (!ctxs || count == 0 || count > RVB_MAX_GROUP) return RVB_ERR_INVALID;
    for (uint64_t i = 0; i < count; ++i)
        if (!ctxs[i]) return RVB_ERR_INVALID;
    if (!mics || !sources || !air_coefficient) return fail(ctxs[0], RVB_ERR_INVALID, "rvb_trace_group: null argument");
    for (uint64_t i = 0; i < count; ++i)
        for (uint64_t j = 0; j < i; ++j)
            if (ctxs[i] == ctxs[j]) return fail(ctxs[0], RVB_ERR_INVALID, "rvb_trace_group: a context is listed twice");
    uint64_t total_rays = 0;
    for (uint64_t i = 0; i < count; ++i) total_rays += ctxs[i]->nrays;
    TracePlan plans[RVB_MAX_GROUP];
    for (uint64_t i = 0; i < count; ++i) {
        const int rc = trace_prepare(ctxs[i], mics + 3 * i, sources + 3 * i, 1, nreflections, air_coefficient, ray_offsets ? ray_offsets[i] : 0,
                                     total_rays, plans[i]);
        if (rc != RVB_OK) return rc;
    }
    // one launch for all of them when they can share a kernel: one or two lanes per ray, one device, one LDS layout (stack depth, surfaces
    // staged, key runs or not: the launch's LDS is laid out once for all its workgroups)
    bool fused = count > 1 && plans[0].a.path_lanes <= 2;
    for (uint64_t i = 1; i < count && fused; ++i)
        fused = ctxs[i]->device == ctxs[0]->device && plans[i].a.path_lanes == plans[0].a.path_lanes && plans[i].a.stack_entries == plans[0].a.stack_entries
                && plans[i].a.lds_surfaces == plans[0].a.lds_surfaces && (plans[i].a.sort_keys16 != nullptr) == (plans[0].a.sort_keys16 != nullptr);
    for (uint64_t i = 0; i < count && fused; ++i) fused = plans[i].nrays > 0;
    if (fused) {
        rvb_ctx * lead = ctxs[0];
        RVB_BIND(lead);
        for (uint64_t i = 1; i < count; ++i) {                      // the others' fills come first
            RVB_HIP(fail, ctxs[i], hipEventRecord(ctxs[i]->prep_done, ctxs[i]->stream));
            RVB_HIP(fail, lead, hipStreamWaitEvent(lead->stream, ctxs[i]->prep_done, 0));
        }
        TraceArgs args[RVB_MAX_GROUP];
        for (uint64_t i = 0; i < count; ++i) args[i] = plans[i].a;
        lead->begin_timing(path_kernel_name(args[0].path_lanes));
        rvb_launch_path_group(args, (uint32_t) count, lead->stream);
        lead->end_timing();
        RVB_HIP(fail, lead, hipEventRecord(lead->group_done, lead->stream));
        for (uint64_t i = 1; i < count; ++i) {
            ctxs[i]->begin_timing(path_kernel_name(args[0].path_lanes));   // (elapsed: from this stream's arrival to the end of the group's kernel)
            RVB_HIP(fail, ctxs[i], hipStreamWaitEvent(ctxs[i]->stream, lead->group_done, 0));
            ctxs[i]->end_timing();
        }
    } else {
        for (uint64_t i = 0; i < count; ++i) {
            RVB_BIND(ctxs[i]);
            ctxs[i]->begin_timing(path_kernel_name(plans[i].a.path_lanes));
            rvb_launch_path(plans[i].a, ctxs[i]->stream);
            ctxs[i]->end_timing();
        }
    }
    for (uint64_t i = 0; i < count; ++i) {
        RVB_BIND(ctxs[i]);
        const int rc = trace_finish(ctxs[i], plans[i], mics + 3 * i);
        if (rc != RVB_OK) return rc;
    }
    return RVB_OK;
}

int rvb_trace(rvb_ctx * ctx, const float mic[3], const float source[3], uint64_t nreflections,
              const float air_coefficient[8], uint64_t ray_offset)
{
    if (!ctx) return RVB_ERR_INVALID;
    if (!mic || !source || !air_coefficient) return fail(ctx, RVB_ERR_INVALID, "rvb_trace: null argument");
    return trace_common(ctx, mic, source, 1, nreflections, air_coefficient, ray_offset);
}

int rvb_trace_pairs(rvb_ctx * ctx, const float * mics, const float * sources, uint64_t npairs, uint64_t nreflections,
                    const float air_coefficient[8], uint64_t ray_offset)
{
    if (!ctx) return RVB_ERR_INVALID;
    if (!mics || !sources || !air_coefficient || npairs == 0) return fail(ctx, RVB_ERR_INVALID, "rvb_trace_pairs: null argument or no pairs");
    return trace_common(ctx, mics, sources, npairs, nreflections, air_coefficient, ray_offset);
}

int rvb_ir_select_pair(rvb_ctx * ctx, uint64_t pair)
{
    if (!ctx) return RVB_ERR_INVALID;
    if (!ctx->trace.traced()) return fail(ctx, RVB_ERR_STATE, "rvb_ir_select_pair: nothing traced");
    if (pair >= ctx->trace.npairs()) return fail(ctx, RVB_ERR_INVALID, "rvb_ir_select_pair: pair out of range");
    ctx->trace.select_pair(pair);
    ctx->ir.drop_configuration();             // (a prepared list names the records of the pair it was made for; the fold reads ir_diffuse)
    return RVB_OK;
}

int rvb_get_diffuse(rvb_ctx * ctx, rvb_impulse * out)
{
    if (!ctx) return RVB_ERR_INVALID;
    if (!ctx->trace.traced()) return fail(ctx, RVB_ERR_STATE, "rvb_get_diffuse: nothing traced");
    RVB_BIND(ctx);
    RVB_HIP(fail, ctx, hipStreamSynchronize(ctx->stream));
    const size_t bytes = (size_t) ctx->trace.rays() * ctx->trace.nreflections() * sizeof(rvb_impulse);
    if (bytes) {
        if (!out) return fail(ctx, RVB_ERR_INVALID, "rvb_get_diffuse: null output");
        return rvb_copy_to_host(ctx, out, ctx->trace.impulses.p, bytes);
    }
    return RVB_OK;
}

int rvb_diffuse_device(rvb_ctx * ctx, const void ** d_impulses, uint64_t * count)
{
    if (!ctx) return RVB_ERR_INVALID;
    if (!ctx->trace.traced()) return fail(ctx, RVB_ERR_STATE, "rvb_diffuse_device: nothing traced");
    if (d_impulses) *d_impulses = ctx->trace.impulses.p;
    if (count) *count = ctx->trace.rays() * ctx->trace.nreflections();
    return RVB_OK;
}

int rvb_get_direct(rvb_ctx * ctx, rvb_impulse * out)
{
    if (!ctx || !out) return RVB_ERR_INVALID;
    if (!ctx->trace.traced()) return fail(ctx, RVB_ERR_STATE, "rvb_get_direct: nothing traced");
    RVB_BIND(ctx);
    int rc = fetch_small(ctx);
    if (rc != RVB_OK) return rc;
    *out = ctx->trace.direct();               // of the pair chosen with rvb_ir_select_pair
    return RVB_OK;
}

int rvb_get_image_candidates(rvb_ctx * ctx, rvb_image_candidate * out, uint64_t capacity, uint64_t * count)
{
    if (!ctx || !count) return RVB_ERR_INVALID;
    if (!ctx->trace.traced()) return fail(ctx, RVB_ERR_STATE, "rvb_get_image_candidates: nothing traced");
    RVB_BIND(ctx);
    int rc = fetch_small(ctx);
    if (rc != RVB_OK) return rc;
    const uint32_t n = ctx->trace.host->small.candidate_count;
    *count = n;
    if (!out)
        return RVB_OK;                       // size query
    if (capacity < n)
        return fail(ctx, RVB_ERR_CAPACITY, "rvb_get_image_candidates: capacity too small");
    if (n) {
        if (n <= kFirstCandidates)
            std::memcpy(out, ctx->trace.host->first, (size_t) n * sizeof(rvb_image_candidate));     // came with the small block
        else
            RVB_HIP(fail, ctx, hipMemcpy(out, ctx->trace.candidates.p, (size_t) n * sizeof(rvb_image_candidate), hipMemcpyDeviceToHost));
        std::sort(out, out + n, by_ray_and_slot);
    }
    return RVB_OK;
}

int rvb_merge_images(const rvb_image_candidate * candidates, uint64_t ncandidates,
                     const rvb_impulse * direct, int remove_direct,
                     rvb_impulse * out, uint64_t capacity, uint64_t * count)
{
    if (!count || (ncandidates && !candidates))
        return RVB_ERR_INVALID;
    std::vector<uint32_t> winners;
    const int rc = merge_image_winners(candidates, ncandidates, direct != nullptr, remove_direct != 0, winners);
    if (rc != RVB_OK) return rc;
    *count = winners.size();
    if (!out)
        return RVB_OK;
    if (capacity < winners.size())
        return RVB_ERR_CAPACITY;
    for (size_t w = 0; w < winners.size(); ++w)
        out[w] = winners[w] == RVB_IMAGE_WINNER_DIRECT ? *direct : candidates[winners[w]].impulse;
    return RVB_OK;
}

}  // extern "C"
