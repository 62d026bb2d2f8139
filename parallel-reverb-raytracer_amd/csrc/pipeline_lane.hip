// pipeline_lane.hip — the device work of one lane of the impulse-response pipeline (csrc/pipeline_lane.h): traces unit by unit, staging
// group by group, results through the ring.  How far, how many and where is csrc/pipeline_schedule.h's; the calls and their order are here.
// Nothing but the public C-ABI underneath (plus HIP for the histogram buffers, their zero fill and a few events).
#include "pipeline_lane.h"
#include "image_merge.h"

#include <algorithm>
#include <cstring>

namespace {
int cfail(Lane * l, int code, rvb_ctx * ctx, const char * where) { return pfail(l, code, std::string(where) + ": " + rvb_last_error(ctx)); }

Job & job_at(Lane * l, uint64_t id) { return l->jobs[(size_t) (id - l->returned)]; }
Slot & slot_of(Lane * l, uint64_t id) { return l->slots[(size_t) sched::context_of(l->shape, sched::unit_of(l->shape, id))]; }

// the source pattern(s) of the trace that follows on `ctx`: jobs [first, first + count) of ONE launch (the per-pair form for count > 1)
int set_source_patterns(Lane * l, rvb_ctx * ctx, uint64_t first, uint64_t count)
{
    const Config & c = *l->cfg;
    if (!c.source_managed) return RVB_OK;
    rvb_source_pattern pats[RVB_PIPELINE_MAX_PAIRS];
    for (uint64_t k = 0; k < count && c.source_on; ++k) {
        const Job & j = job_at(l, first + k);
        for (int i = 0; i < 3; ++i) pats[k].direction[i] = j.source_direction[i];
        pats[k].direction[3] = 0.0f;
        std::memcpy(pats[k].shape, c.source_shape, sizeof(c.source_shape));
    }
    const int rc = c.source_on ? rvb_set_source_pattern(ctx, pats, count) : rvb_set_source_pattern(ctx, nullptr, 0);
    return rc != RVB_OK ? cfail(l, rc, ctx, "rvb_pipeline: source pattern") : (int) RVB_OK;
}

// the traces of jobs [first, last) in ONE launch: a unit (or the part of it that is submitted) on its context, or a group of one-pair
// units over their contexts (one path-kernel launch where the contexts allow it: rvb_trace_group decides)
int begin_jobs(Lane * l, uint64_t first, uint64_t last)
{
    static_assert(RVB_PIPELINE_MAX_GROUP <= RVB_PIPELINE_MAX_PAIRS, "one array size serves both kinds of launch");
    const uint64_t count = last - first;
    const Config & c = *l->cfg;
    rvb_ctx * ctxs[RVB_PIPELINE_MAX_PAIRS];
    float mics[3 * RVB_PIPELINE_MAX_PAIRS], sources[3 * RVB_PIPELINE_MAX_PAIRS];
    for (uint64_t k = 0; k < count; ++k) {
        const Job & j = job_at(l, first + k);
        ctxs[k] = slot_of(l, first + k).ctx;
        std::memcpy(mics + 3 * k, j.mic, sizeof(j.mic));
        std::memcpy(sources + 3 * k, j.source, sizeof(j.source));
    }
    int rc = RVB_OK;
    for (uint64_t k = 0; k < (l->several ? 1 : count) && rc == RVB_OK; ++k) rc = set_source_patterns(l, ctxs[k], first + k, l->several ? count : 1);
    if (rc != RVB_OK) return rc;
    if (l->several) rc = rvb_trace_pairs(ctxs[0], mics, sources, count, c.nreflections, c.air, 0);
    else if (count > 1) rc = rvb_trace_group(ctxs, count, mics, sources, c.nreflections, c.air, nullptr);
    else rc = rvb_trace(ctxs[0], mics, sources, c.nreflections, c.air, 0);
    if (rc != RVB_OK) return cfail(l, rc, ctxs[0], "rvb_pipeline: trace");
    for (uint64_t k = 0; k < count; ++k) {
        job_at(l, first + k).pair = l->several ? k : 0;
        job_at(l, first + k).launch_pairs = l->several ? count : 1;
    }
    return RVB_OK;
}

// begins jobs in submission order, group by group, up to (not including) job `limit`
int begin_upto(Lane * l, uint64_t limit)
{
    const sched::Shape & s = l->shape;
    limit = std::min(limit, std::min(l->submitted, l->allow));
    auto handed_over = [l](uint64_t job) { return job < l->returned || job_at(l, job).staged; };
    for (uint64_t id = l->begun_upto; id < limit; ++id) {
        const uint64_t unit = sched::unit_of(s, id);
        const bool free = (!sched::has_predecessor(s, unit) || handed_over(sched::predecessor_last_job(s, unit))) &&
                          (id != l->begun_upto || !sched::continues_partial_unit(s, id) || handed_over(id - 1));
        if (!free) { limit = id; break; }
    }
    while (l->begun_upto < limit) {
        const uint64_t last = std::min(sched::group_end(s, l->begun_upto), limit);
        const int rc = begin_jobs(l, l->begun_upto, last);
        if (rc != RVB_OK) return rc;
        l->begun_upto = last;
    }
    return RVB_OK;
}

// l->candidates = the image-source candidates of the context's last trace
int fetch_candidates(Lane * l, rvb_ctx * ctx)
{
    l->candidates.clear();
    const int rc = append_image_candidates(ctx, l->candidates);
    return rc != RVB_OK ? cfail(l, rc, ctx, "rvb_pipeline: candidates") : (int) RVB_OK;
}

// Staging of a traced job in two phases, so that a group's jobs overlap their device work: (1) image-source merge and configuration — the
// only host wait is the one for the trace's small result block (image-source candidates, time range of the speaker model) — and the HRTF
// model's time-range pass ENQUEUED; (2) the time range read, the histogram sized and zeroed, binning + export enqueued.
int stage_configure(Lane * l, Job & j)
{
    const Config & c = *l->cfg;
    Slot & s = slot_of(l, j.id);
    rvb_ctx * ctx = s.ctx;
    int rc;
    const std::vector<rvb_image_candidate> * cand = &l->candidates;
    if (!l->several) {
        if ((rc = fetch_candidates(l, ctx)) != RVB_OK) return rc;
    } else {
        if ((rc = rvb_ir_select_pair(ctx, j.pair)) != RVB_OK) return cfail(l, rc, ctx, "rvb_pipeline: select pair");
        l->pair_candidates.clear();
        cand = &l->pair_candidates;
        if (c.which & RVB_IR_IMAGES) {
            // this pair's share of the launch's candidates (l->candidates, global ray numbers: pair = ray / rays per pair), its ray numbers
            // made relative to the pair — what distributed.generate_pair_irs merges (Context.get_pair_candidates)
            const void * d = nullptr;
            uint64_t count = 0;
            if ((rc = rvb_diffuse_device(ctx, &d, &count)) != RVB_OK) return cfail(l, rc, ctx, "rvb_pipeline: rays per pair");
            const uint64_t nrays = count / (c.nreflections * j.launch_pairs);
            for (const rvb_image_candidate & x : l->candidates)
                if (nrays && x.ray / nrays == j.pair) {
                    l->pair_candidates.push_back(x);
                    l->pair_candidates.back().ray -= j.pair * nrays;
                }
        }
    }
    l->images.clear();
    if (c.which & RVB_IR_IMAGES) {
        rvb_impulse direct;
        if ((rc = rvb_get_direct(ctx, &direct)) != RVB_OK) return cfail(l, rc, ctx, "rvb_pipeline: direct path");
        if ((rc = merge_images(cand->data(), cand->size(), &direct, c.remove_direct, l->images)) != RVB_OK) return pfail(l, rc, "rvb_pipeline: rvb_merge_images");
    }
    const uint64_t nimages = l->images.size();
    if (c.hrtf) {
        // (the table goes up with a context's first job only: rvb_ir_configure_hrtf keeps it for table == NULL)
        rc = rvb_ir_configure_hrtf(ctx, j.mic, s.has_table ? nullptr : c.table.data(), j.facing, j.up, c.which, l->images.data(), nimages);
        s.has_table = rc == RVB_OK;
    }
    else rc = rvb_ir_configure_speakers(ctx, j.mic, c.speakers.data(), c.speakers.size(), c.which, l->images.data(), nimages);
    if (rc != RVB_OK) return cfail(l, rc, ctx, "rvb_pipeline: configure");
    j.nimages = nimages;
    if ((rc = rvb_ir_time_range_begin(ctx)) != RVB_OK) return cfail(l, rc, ctx, "rvb_pipeline: time range");
    return RVB_OK;
}

int stage_bin(Lane * l, Job & j)
{
    const Config & c = *l->cfg;
    Slot & s = slot_of(l, j.id);
    rvb_ctx * ctx = s.ctx;
    float lo = 0.0f, hi = 0.0f;
    int rc = rvb_ir_time_range(ctx, &lo, &hi);
    if (rc != RVB_OK) return cfail(l, rc, ctx, "rvb_pipeline: time range");
    j.predelay = c.trim_predelay ? lo : 0.0f, j.max_time = hi;
    j.nbins = rvb_ir_bins(hi, j.predelay, c.sample_rate);
    const size_t bytes = (size_t) j.nbins * c.nchannels() * 8 * sizeof(float);
    RVB_HIP(pfail, l, hipSetDevice(l->device));
    // (each pair of a unit has a histogram of its own: pair k's export must not read what pair k + 1's zero fill and binning write)
    DevBuf & hist = s.hist[(size_t) (j.id % l->shape.pairs)];
    // (the previous histogram of this context left for the host before its result was handed out: nothing reads it any more;
    // an eighth of head-room, so that slowly growing histograms do not reallocate every time)
    if (bytes > hist.cap) RVB_HIP(pfail, l, hist.ensure(bytes + bytes / 8));
    PinnedBuf & hb = l->ring[(size_t) (j.id % l->ring.size())];
    if (bytes > hb.cap) RVB_HIP(pfail, l, hb.ensure(bytes + bytes / 8));
    j.host = hb.as<float>();
    RVB_HIP(pfail, l, hipMemsetAsync(hist.p, 0, bytes, l->fill_stream));
    RVB_HIP(pfail, l, hipEventRecord(s.zeroed, l->fill_stream));
    if ((rc = rvb_wait_for_event(ctx, s.zeroed)) != RVB_OK) return cfail(l, rc, ctx, "rvb_pipeline: wait for the zero fill");
    if ((rc = rvb_ir_accumulate_export(ctx, j.predelay, c.sample_rate, j.nbins, c.mode, hist.p, j.host, 0)) != RVB_OK) return cfail(l, rc, ctx, "rvb_pipeline: binning");
    j.staged = true;
    return RVB_OK;
}

// The begun jobs [first, last) of the front group, round by round: the r-th pair of every unit configured, then binned — so the binning
// stages of ALL units of a group are enqueued before the host waits for any of them, and the pairs of a unit follow one another on its
// context.  Then the host waits for the group's binning (not for the histograms' way to the host), once per context.
int stage_group(Lane * l, uint64_t first, uint64_t last)
{
    const sched::Shape & s = l->shape;
    const uint64_t P = s.pairs, unit_begin = sched::unit_of(s, first), unit_end = sched::unit_of(s, last - 1) + 1;
    int rc;
    // all pairs of the launch, global ray numbers (several pairs put a group of one unit: `first` names its context)
    if (l->several) l->candidates.clear();
    if (l->several && (l->cfg->which & RVB_IR_IMAGES) && (rc = fetch_candidates(l, slot_of(l, first).ctx)) != RVB_OK) return rc;
    for (uint64_t r = 0; r < P; ++r)
        for (int phase = 0; phase < 2; ++phase)
            for (uint64_t u = unit_begin; u < unit_end; ++u) {
                const uint64_t id = std::max(first, u * P) + r;
                if (id >= std::min(last, (u + 1) * P)) continue;
                Slot & slot = slot_of(l, id);
                if (phase == 1) rc = stage_bin(l, job_at(l, id));
                else {
                    // rvb_ir_configure_* uploads the merged images from the context's host copy, which the next configuration overwrites:
                    // the previous pair's upload must be done (stream order protects the device buffer, not that host copy)
                    if (r > 0) RVB_HIP(pfail, l, hipEventSynchronize(slot.uploaded));
                    rc = stage_configure(l, job_at(l, id));
                    if (rc == RVB_OK && l->several && (rc = rvb_record_event(slot.ctx, slot.uploaded)) != RVB_OK) return cfail(l, rc, slot.ctx, "rvb_pipeline: record");
                }
                if (rc != RVB_OK) return rc;
            }
    for (uint64_t u = unit_begin; u < unit_end; ++u) {
        rvb_ctx * ctx = l->slots[(size_t) sched::context_of(s, u)].ctx;
        if ((rc = rvb_synchronize(ctx)) != RVB_OK) return cfail(l, rc, ctx, "rvb_pipeline_next: wait");
    }
    return RVB_OK;
}
}  // namespace

int lane_submit(Lane * l, const Job & in)
{
    l->jobs.push_back(in);
    l->jobs.back().id = l->submitted++;
    // keep the device busy without waiting for the caller's next call
    return begin_upto(l, sched::ahead_on_submit(l->shape, l->returned, l->submitted));
}

int lane_next(Lane * l, rvb_pipeline_result * out)
{
    Job & j = l->jobs.front();
    int rc = begin_upto(l, sched::ahead_before_staging(l->shape, j.id));
    if (rc != RVB_OK) return rc;
    if (!j.staged) {
        // the group's begun jobs from the front on (all of one launch with several pairs: the rest of a unit waits for its first part)
        if ((rc = stage_group(l, j.id, std::min(sched::group_end(l->shape, j.id), l->begun_upto))) != RVB_OK) return rc;
        // With the binning done, the group's contexts take the traces of the group after next — enqueued before this call waits for
        // the link, so the copy runs beside them.
        // (measured: enqueuing those traces in stream order behind the binning, BEFORE the wait in stage_group, costs 4.45 -> 5.6 ms per
        // IR at workload C2: a third group's path kernel then competes with this group's binning for the SIMDs;
        // and enqueuing them LATER costs as well: a host delay of 100 / 300 / 600 / 1000 us here: 4.45 -> 4.53 / 4.57 / 4.69 / 4.96 ms per IR)
        if ((rc = begin_upto(l, sched::ahead_after_staging(l->shape, j.id, l->submitted))) != RVB_OK) return rc;
    }
    rvb_ctx * ctx = slot_of(l, j.id).ctx;
    if ((rc = rvb_synchronize_exports(ctx)) != RVB_OK) return cfail(l, rc, ctx, "rvb_pipeline_next: wait");
    *out = rvb_pipeline_result{j.id, j.host, l->cfg->nchannels(), j.nbins, j.predelay, j.max_time, j.nimages};
    l->jobs.pop_front();
    ++l->returned;
    return rc;
}

int lane_init(Lane * l, uint64_t group, uint64_t pairs, uint64_t ring)
{
    const uint64_t count = l->slots.size();
    l->shape = sched::Shape{count, sched::group_size(group, count, pairs, RVB_PIPELINE_MAX_GROUP), pairs};
    l->several = pairs > 1;
    l->ring.resize((size_t) ring);
    auto refuse = [l](int rc) { l->slots.clear(); return rc; };      // (lane_drain then leaves the contexts alone: nothing was set on them)
    for (uint64_t i = 0; i < count; ++i) {
        int d = 0;
        if (rvb_device_index(l->slots[i].ctx, &d) != RVB_OK || (i && d != l->device)) return refuse(RVB_ERR_INVALID);
        l->device = d;
    }
    if (hipSetDevice(l->device) != hipSuccess) return refuse(RVB_ERR_HIP);
    if (hipStreamCreateWithFlags(&l->fill_stream.h, hipStreamNonBlocking) != hipSuccess) return refuse(RVB_ERR_HIP);
    for (Slot & s : l->slots) {
        if (hipEventCreateWithFlags(&s.zeroed.h, hipEventDisableTiming) != hipSuccess) return RVB_ERR_HIP;
        if (l->several && hipEventCreateWithFlags(&s.uploaded.h, hipEventDisableTiming) != hipSuccess) return RVB_ERR_HIP;
        (void) rvb_set_concurrent_traces(s.ctx, (uint32_t) l->shape.group);     // the traces of a group run side by side: the path kernel is sized for them
    }
    return RVB_OK;
}

void lane_drain(Lane * l)
{
    (void) hipSetDevice(l->device);
    for (Slot & s : l->slots) { (void) rvb_synchronize(s.ctx); (void) rvb_synchronize_exports(s.ctx); (void) rvb_set_concurrent_traces(s.ctx, 1); }
    if (l->fill_stream) (void) hipStreamSynchronize(l->fill_stream);
}
