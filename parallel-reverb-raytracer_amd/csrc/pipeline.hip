// pipeline.hip — impulse responses back to back behind the C-ABI (rvb_pipeline_* of include/rvb_capi.h): the schedule that
// bench.py times, for a C / C++ caller.  What it replaces for a batch caller is the reference's cmd/main.cpp:241-298 in a loop — one
// Raytracer::raytrace, one Attenuator::attenuate per channel, fixPredelay, flattenImpulses per impulse response, each stage blocking.
//
// The trace of an impulse response is bound by vector issue, its record grouping and binning by memory, its image-source merge and its
// configuration by the host.  So several contexts of one GPU (the caller's: same scene, same rays on each) take turns — a LANE:
//   * jobs are traced in GROUPS of `group` contexts — one path-kernel launch for the group (rvb_trace_group): more waves per SIMD for
//     the latency-bound bounce chains;
//   * the traces of the group after next are enqueued before the current group is finished, so a path kernel is (nearly) always
//     resident and the other stages of the previous group run beside it;
//   * the binning stages of ALL impulse responses of a group are enqueued — each behind its own trace's image-source candidates —
//     before the host waits for any of them;
//   * every finished histogram leaves for a pinned host buffer of the lane's ring on the context's export stream, bin range by bin
//     range (rvb_ir_accumulate_export); the lane's next result is there when the oldest job's histogram has landed.
// With `pairs` > 1 a lane's UNIT is that many consecutive jobs, traced by ONE rvb_trace_pairs launch on one context (group 1); its pairs
// are staged one after another (rvb_ir_select_pair: the configuration is the context's), each into a device histogram of its own.
//
// rvb_pipeline_create drives one lane in the caller's thread.  rvb_pipeline_create_lanes drives several, each from a host thread of its
// own (the only thread that touches the lane's contexts); unit u goes to lane u % lanes, results come back in submission order.
// Nothing but the public C-ABI underneath (plus HIP for the histogram buffers, their zero fill and a few events).
#include "../../include/rvb_capi.h"
#include "hip_owned.h"

#include <algorithm>
#include <cmath>
#include <condition_variable>
#include <cstdlib>
#include <cstring>
#include <deque>
#include <memory>
#include <mutex>
#include <string>
#include <thread>
#include <vector>

namespace {

struct Job {
    uint64_t id = 0;                          // the lane's submission number (the pipeline's for rvb_pipeline_create)
    uint64_t pair = 0, launch_pairs = 1;      // pairs > 1: this job's pair in its rvb_trace_pairs launch, and that launch's pair count
    float mic[3] = {0, 0, 0}, source[3] = {0, 0, 0}, facing[3] = {0, 0, 0}, up[3] = {0, 0, 0};
    float source_direction[3] = {0, 0, 0};    // the way this job's source faces (Config::source_on)
    bool begun = false, staged = false;
    uint64_t nbins = 0, nimages = 0;
    float predelay = 0.0f, max_time = 0.0f;
    float * host = nullptr;
};

struct Slot {                                 // per context
    rvb_ctx * ctx = nullptr;
    bool has_table = false;                   // the pipeline's HRTF table is on this context's device (uploaded with its first HRTF job)
    DevBuf hist[RVB_PIPELINE_MAX_PAIRS];      // device [nchannels][8][nbins], one per pair of a unit
    Event zeroed;
    Event uploaded;                           // pairs > 1: behind a pair's rvb_ir_configure_* (its image upload reads the context's host copy)
};

// model + binning configuration (rvb_pipeline_configure_*): the pipeline's, read by its lanes while jobs are pending
struct Config {
    bool configured = false, hrtf = false;
    std::vector<rvb_speaker> speakers;
    std::vector<float> table;                 // [2][360*180*8]
    float facing[3] = {0, 0, 1}, up[3] = {0, 1, 0};
    int which = RVB_IR_ALL, remove_direct = 0, trim_predelay = 1, mode = RVB_IR_EXACT;
    float sample_rate = 44100.0f;
    uint64_t nreflections = 0;
    float air[8] = {0, 0, 0, 0, 0, 0, 0, 0};
    // directional sources (rvb_pipeline_set_source_pattern): from its first call on the pipeline sets or clears its contexts' patterns
    bool source_managed = false, source_on = false;
    float source_shape[8] = {0, 0, 0, 0, 0, 0, 0, 0}, source_direction[3] = {0, 0, 1};
};

struct Lane {
    const Config * cfg = nullptr;
    uint64_t index = 0;
    std::vector<Slot> slots;
    uint64_t group = 1, pairs = 1;
    int device = 0;
    Stream fill_stream;                       // zero fills of the histograms (the contexts' streams wait for them by an event)
    std::string error;
    // jobs: [returned, submitted); jobs.front() is the oldest not yet returned
    std::deque<Job> jobs;
    uint64_t submitted = 0, returned = 0, begun_upto = 0;
    uint64_t allow = UINT64_MAX;              // jobs [0, allow) may be traced (a lane thread holds back an incomplete last unit / group)
    std::vector<PinnedBuf> ring;              // pinned result buffers, job id % ring.size()
    std::vector<rvb_image_candidate> candidates, pair_candidates;
    std::vector<rvb_impulse> images;
    // rvb_pipeline_create_lanes: the lane's thread and what it shares with the caller's (guarded by rvb_pipeline::mu)
    std::thread worker;
    std::vector<rvb_ctx *> init_ctxs;
    bool initialised = false;
    int init_rc = RVB_OK;
    std::condition_variable wake;
    std::deque<Job> inbox;                    // submitted by the caller, not yet handed to the lane
    std::deque<uint64_t> ids;                 // pipeline job numbers of the lane's jobs [returned, submitted) and of the inbox
    bool quit = false;
    int failed = RVB_OK;                      // a stage failed: every pending and later job of the lane returns this code
    std::string failure;
    ~Lane() { (void) hipSetDevice(device); }  // (lane_drain has run: nothing uses what the members release)
};

struct Outcome {                              // a job of rvb_pipeline_create_lanes, as its lane's thread finished it
    bool ready = false;
    int rc = RVB_OK;
    std::string error;
    rvb_pipeline_result result{};
};

}  // namespace

struct rvb_pipeline {
    Config cfg;
    std::vector<std::unique_ptr<Lane>> lanes;
    bool threaded = false;                    // rvb_pipeline_create_lanes
    uint64_t pairs = 1, ncontexts = 0, limit = 0;
    std::string error;
    // rvb_pipeline_create_lanes: the caller's side
    std::mutex mu;
    std::condition_variable done;
    std::deque<Outcome> outcomes;             // jobs [returned, submitted)
    uint64_t submitted = 0, returned = 0, wanted = 0;    // wanted: rvb_pipeline_next waits for the jobs below it
};

namespace {

template <class Owner>                        // a Lane or the pipeline: each has its own last error
int pfail(Owner * o, int code, const std::string & what)
{
    if (o) o->error = what;
    return code;
}
int cfail(Lane * l, int code, rvb_ctx * ctx, const char * where)
{
    return pfail(l, code, std::string(where) + ": " + rvb_last_error(ctx));
}

Job & job_at(Lane * l, uint64_t id) { return l->jobs[(size_t) (id - l->returned)]; }
// job i runs on context (i / pairs) % contexts: units go round-robin over the lane's contexts
Slot & slot_of(Lane * l, uint64_t id) { return l->slots[(size_t) ((id / l->pairs) % l->slots.size())]; }

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

// the traces of jobs [first, last): one launch for the group where the contexts allow it (rvb_trace_group decides); pairs > 1: one unit
// (or the part of it that is submitted) in ONE rvb_trace_pairs launch on the unit's context
int begin_jobs(Lane * l, uint64_t first, uint64_t last)
{
    const uint64_t n = l->slots.size(), count = last - first;
    const Config & c = *l->cfg;
    if (l->pairs > 1) {
        rvb_ctx * ctx = slot_of(l, first).ctx;
        float mics[3 * RVB_PIPELINE_MAX_PAIRS], sources[3 * RVB_PIPELINE_MAX_PAIRS];
        for (uint64_t k = 0; k < count; ++k) {
            const Job & j = job_at(l, first + k);
            std::memcpy(mics + 3 * k, j.mic, sizeof(j.mic));
            std::memcpy(sources + 3 * k, j.source, sizeof(j.source));
        }
        int rc = set_source_patterns(l, ctx, first, count);
        if (rc != RVB_OK) return rc;
        rc = rvb_trace_pairs(ctx, mics, sources, count, c.nreflections, c.air, 0);
        if (rc != RVB_OK) return cfail(l, rc, ctx, "rvb_pipeline: trace");
        for (uint64_t k = 0; k < count; ++k) {
            Job & j = job_at(l, first + k);
            j.pair = k;
            j.launch_pairs = count;
            j.begun = true;
        }
        return RVB_OK;
    }
    rvb_ctx * ctxs[RVB_PIPELINE_MAX_GROUP];
    float mics[3 * RVB_PIPELINE_MAX_GROUP], sources[3 * RVB_PIPELINE_MAX_GROUP];
    for (uint64_t k = 0; k < count; ++k) {
        const Job & j = job_at(l, first + k);
        ctxs[k] = l->slots[(size_t) ((first + k) % n)].ctx;
        std::memcpy(mics + 3 * k, j.mic, sizeof(j.mic));
        std::memcpy(sources + 3 * k, j.source, sizeof(j.source));
        const int rs = set_source_patterns(l, ctxs[k], first + k, 1);
        if (rs != RVB_OK) return rs;
    }
    int rc;
    if (count > 1) rc = rvb_trace_group(ctxs, count, mics, sources, c.nreflections, c.air, nullptr);
    else rc = rvb_trace(ctxs[0], mics, sources, c.nreflections, c.air, 0);
    if (rc != RVB_OK) return cfail(l, rc, ctxs[0], "rvb_pipeline: trace");
    for (uint64_t k = 0; k < count; ++k) job_at(l, first + k).begun = true;
    return RVB_OK;
}

// begins jobs in submission order, group by group (unit by unit), up to (not including) job `limit`
int begin_upto(Lane * l, uint64_t limit)
{
    limit = std::min(limit, std::min(l->submitted, l->allow));
    // job i runs on context (i / pairs) % contexts: it may go out once the unit that used the context before has handed it over —
    // returned, or at least staged (its binning is enqueued; the new trace follows it in stream order and touches none of its buffers)
    const uint64_t n = l->slots.size(), P = l->pairs;
    for (uint64_t id = l->begun_upto; id < limit; ++id) {
        const uint64_t unit = id / P;
        if (unit >= n) {
            const uint64_t prev = (unit - n) * P + P - 1;      // the last job of that unit
            if (prev >= l->returned && !job_at(l, prev).staged) { limit = id; break; }
        }
        // (pairs: the rest of a unit whose first part went out in a launch of its own waits until that part is staged — the new launch
        // replaces the context's trace results)
        if (P > 1 && id == l->begun_upto && id % P != 0 && id - 1 >= l->returned && !job_at(l, id - 1).staged) { limit = id; break; }
    }
    const uint64_t gj = l->group * P;
    while (l->begun_upto < limit) {
        const uint64_t group_end = (l->begun_upto / gj + 1) * gj;
        const uint64_t last = std::min(group_end, limit);
        const int rc = begin_jobs(l, l->begun_upto, last);
        if (rc != RVB_OK) return rc;
        l->begun_upto = last;
    }
    return RVB_OK;
}

// l->candidates = the image-source candidates of the context's last trace
int fetch_candidates(Lane * l, rvb_ctx * ctx)
{
    uint64_t ncand = 0;
    int rc = rvb_get_image_candidates(ctx, nullptr, 0, &ncand);
    if (rc != RVB_OK) return cfail(l, rc, ctx, "rvb_pipeline: candidates");
    l->candidates.resize(ncand);
    if (ncand && (rc = rvb_get_image_candidates(ctx, l->candidates.data(), ncand, &ncand)) != RVB_OK) return cfail(l, rc, ctx, "rvb_pipeline: candidates");
    return RVB_OK;
}

// Staging of a traced job in two phases, so that a group's jobs overlap their device work: (1) image-source merge and configuration — the
// only host wait is the one for the trace's small result block (image-source candidates, time range of the speaker model) — and the HRTF
// model's time-range pass ENQUEUED; (2) the time range read, the histogram sized and zeroed, binning + export enqueued.
int stage_configure(Lane * l, Job & j)
{
    const Config & c = *l->cfg;
    Slot & s = slot_of(l, j.id);
    rvb_ctx * ctx = s.ctx;
    uint64_t ncand = 0, nimages = 0;
    int rc;
    const rvb_image_candidate * cand = l->candidates.data();
    if (l->pairs > 1) {
        if ((rc = rvb_ir_select_pair(ctx, j.pair)) != RVB_OK) return cfail(l, rc, ctx, "rvb_pipeline: select pair");
        if (c.which & RVB_IR_IMAGES) {
            // this pair's share of the launch's candidates (l->candidates, global ray numbers: pair = ray / rays per pair), its ray numbers
            // made relative to the pair — what distributed.generate_pair_irs merges (Context.get_pair_candidates)
            const void * d = nullptr;
            uint64_t count = 0;
            if ((rc = rvb_diffuse_device(ctx, &d, &count)) != RVB_OK) return cfail(l, rc, ctx, "rvb_pipeline: rays per pair");
            const uint64_t nrays = count / (c.nreflections * j.launch_pairs);
            l->pair_candidates.clear();
            for (const rvb_image_candidate & x : l->candidates)
                if (nrays && x.ray / nrays == j.pair) {
                    l->pair_candidates.push_back(x);
                    l->pair_candidates.back().ray -= j.pair * nrays;
                }
            cand = l->pair_candidates.data();
            ncand = l->pair_candidates.size();
        }
    } else {
        if ((rc = fetch_candidates(l, ctx)) != RVB_OK) return rc;
        cand = l->candidates.data();
        ncand = l->candidates.size();
    }
    l->images.clear();
    if (c.which & RVB_IR_IMAGES) {
        rvb_impulse direct;
        if ((rc = rvb_get_direct(ctx, &direct)) != RVB_OK) return cfail(l, rc, ctx, "rvb_pipeline: direct path");
        if ((rc = rvb_merge_images(cand, ncand, &direct, c.remove_direct, nullptr, 0, &nimages)) != RVB_OK) return pfail(l, rc, "rvb_pipeline: rvb_merge_images");
        l->images.resize(nimages);
        if (nimages && (rc = rvb_merge_images(cand, ncand, &direct, c.remove_direct, l->images.data(), nimages, &nimages)) != RVB_OK)
            return pfail(l, rc, "rvb_pipeline: rvb_merge_images");
    }
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
    j.predelay = c.trim_predelay ? lo : 0.0f;
    j.max_time = hi;
    j.nbins = rvb_ir_bins(hi, j.predelay, c.sample_rate);
    const uint64_t nch = c.hrtf ? 2 : c.speakers.size();
    const size_t bytes = (size_t) j.nbins * nch * 8 * sizeof(float);
    RVB_HIP(pfail, l, hipSetDevice(l->device));
    // (each pair of a unit has a histogram of its own: pair k's export must not read what pair k + 1's zero fill and binning write)
    DevBuf & hist = s.hist[(size_t) (j.id % l->pairs)];
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

// the pairs [first, last) of ONE launch, staged one after another on its context
int stage_pairs(Lane * l, uint64_t first, uint64_t last)
{
    const Config & c = *l->cfg;
    Slot & s = slot_of(l, first);
    rvb_ctx * ctx = s.ctx;
    int rc;
    l->candidates.clear();
    if ((c.which & RVB_IR_IMAGES) && (rc = fetch_candidates(l, ctx)) != RVB_OK) return rc;      // all pairs of the launch, global ray numbers
    for (uint64_t id = first; id < last; ++id) {
        // rvb_ir_configure_* uploads the merged images from the context's host copy, which the next configuration overwrites: the
        // previous pair's upload must be done (stream order protects the device buffer, not that host copy)
        if (id > first) RVB_HIP(pfail, l, hipEventSynchronize(s.uploaded));
        if ((rc = stage_configure(l, job_at(l, id))) != RVB_OK) return rc;
        if ((rc = rvb_record_event(ctx, s.uploaded)) != RVB_OK) return cfail(l, rc, ctx, "rvb_pipeline: record");
        if ((rc = stage_bin(l, job_at(l, id))) != RVB_OK) return rc;
    }
    return RVB_OK;
}

int lane_submit(Lane * l, const Job & in)
{
    Job j = in;
    j.id = l->submitted;
    l->jobs.push_back(j);
    ++l->submitted;
    // keep the device busy without waiting for the caller's next call: the traces of COMPLETE groups (units) go out as soon as contexts
    // are free for them (job i runs on context (i / pairs) % contexts; the contexts of jobs that have not been returned yet are taken);
    // an incomplete last group is traced when rvb_pipeline_next gets to it
    const uint64_t gj = l->group * l->pairs;
    return begin_upto(l, std::min(l->returned / gj * gj + l->slots.size() * l->pairs, l->submitted / gj * gj));
}

int lane_next(Lane * l, rvb_pipeline_result * out)
{
    const Config & c = *l->cfg;
    const uint64_t n = l->slots.size(), P = l->pairs, gj = l->group * P;
    Job & j = l->jobs.front();
    const uint64_t group_first = j.id / gj * gj;
    // the traces of the groups after this one, as far as contexts are free: every context holds one job (unit)
    int rc = begin_upto(l, group_first + n * P);
    if (rc != RVB_OK) return rc;
    if (!j.staged && P > 1) {
        // the unit's pairs (all of one launch: the rest of a unit waits for its first part's staging), then its binning, then the
        // traces that take the context next
        const uint64_t last = std::min(group_first + gj, l->begun_upto);
        if ((rc = stage_pairs(l, j.id, last)) != RVB_OK) return rc;
        rvb_ctx * ctx = slot_of(l, j.id).ctx;
        if ((rc = rvb_synchronize(ctx)) != RVB_OK) return cfail(l, rc, ctx, "rvb_pipeline_next: wait");
        if ((rc = begin_upto(l, std::min(group_first + gj + n * P, l->submitted / gj * gj))) != RVB_OK) return rc;
    } else if (!j.staged) {
        // the binning stages of all (begun) jobs of this group, before the host waits for any of them
        const uint64_t last = std::min(group_first + l->group, l->begun_upto);
        for (uint64_t id = j.id; id < last; ++id)
            if ((rc = stage_configure(l, job_at(l, id))) != RVB_OK) return rc;
        for (uint64_t id = j.id; id < last; ++id)
            if ((rc = stage_bin(l, job_at(l, id))) != RVB_OK) return rc;
        // ... then for their binning (not for their histograms' way to the host): with it done, the group's contexts take the traces of
        // the group after next — enqueued before this call waits for the link, so the copy runs beside them
        // (measured: enqueuing those traces in stream order behind the binning, BEFORE this wait, costs 4.45 -> 5.6 ms per
        // IR at workload C2: a third group's path kernel then competes with this group's binning for the SIMDs)
        for (uint64_t id = j.id; id < last; ++id) {
            rvb_ctx * cx = l->slots[(size_t) (id % n)].ctx;
            if ((rc = rvb_synchronize(cx)) != RVB_OK) return cfail(l, rc, cx, "rvb_pipeline_next: wait");
        }
        // (and enqueuing them LATER costs as well: a host delay of 100 / 300 / 600 / 1000 us here: 4.45 -> 4.53 / 4.57 / 4.69 / 4.96 ms per IR)
        if ((rc = begin_upto(l, std::min(group_first + l->group + n, l->submitted / l->group * l->group))) != RVB_OK) return rc;
    }
    rvb_ctx * ctx = slot_of(l, j.id).ctx;
    if ((rc = rvb_synchronize_exports(ctx)) != RVB_OK) return cfail(l, rc, ctx, "rvb_pipeline_next: wait");
    out->job = j.id;
    out->histogram = j.host;
    out->nchannels = c.hrtf ? 2 : c.speakers.size();
    out->nbins = j.nbins;
    out->predelay = j.predelay;
    out->max_time = j.max_time;
    out->nimages = j.nimages;
    l->jobs.pop_front();
    ++l->returned;
    return rc;
}

// a lane's streams and events, its contexts' hint; the contexts are the caller's (scene and rays set, all on one device)
int lane_init(Lane * l, rvb_ctx ** ctxs, uint64_t count, uint64_t group, uint64_t pairs)
{
    // groups of half the contexts (two groups in flight), as measured best at workload C2 (4 contexts in groups of 2); at most what one
    // launch takes; units of several pairs go out one per launch
    uint64_t g = group ? group : std::max<uint64_t>(1, count / 2);
    g = std::min<uint64_t>(std::min<uint64_t>(g, count), RVB_PIPELINE_MAX_GROUP);
    l->group = pairs > 1 ? 1 : g;
    l->pairs = pairs;
    int device = 0;
    for (uint64_t i = 0; i < count; ++i) {
        int d = 0;
        if (rvb_device_index(ctxs[i], &d) != RVB_OK || (i && d != device)) return RVB_ERR_INVALID;
        device = d;
    }
    l->device = device;
    if (hipSetDevice(device) != hipSuccess) return RVB_ERR_HIP;
    if (hipStreamCreateWithFlags(&l->fill_stream.h, hipStreamNonBlocking) != hipSuccess) return RVB_ERR_HIP;
    for (uint64_t i = 0; i < count; ++i) {
        Slot s;
        s.ctx = ctxs[i];
        if (hipEventCreateWithFlags(&s.zeroed.h, hipEventDisableTiming) != hipSuccess) return RVB_ERR_HIP;
        if (pairs > 1 && hipEventCreateWithFlags(&s.uploaded.h, hipEventDisableTiming) != hipSuccess) return RVB_ERR_HIP;
        l->slots.push_back(std::move(s));
        (void) rvb_set_concurrent_traces(ctxs[i], (uint32_t) l->group);     // the traces of a group run side by side: the path kernel is sized for them
    }
    return RVB_OK;
}

// the end of a lane's work: its contexts and its fill stream idle, the contexts' hint withdrawn (~Lane then releases buffers and events)
void lane_drain(Lane * l)
{
    (void) hipSetDevice(l->device);
    for (Slot & s : l->slots) { (void) rvb_synchronize(s.ctx); (void) rvb_synchronize_exports(s.ctx); (void) rvb_set_concurrent_traces(s.ctx, 1); }
    if (l->fill_stream) (void) hipStreamSynchronize(l->fill_stream);
}

// ---- rvb_pipeline_create_lanes: one host thread per lane -------------------------------------------------------------------------------

// (p->mu held) a job's result or failure for the caller
void finish(rvb_pipeline * p, uint64_t id, int rc, const std::string & error, const rvb_pipeline_result * r)
{
    Outcome & o = p->outcomes[(size_t) (id - p->returned)];
    o.ready = true;
    o.rc = rc;
    o.error = error;
    if (r) { o.result = *r; o.result.job = id; }
}

void lane_thread(rvb_pipeline * p, Lane * l)
{
    std::unique_lock<std::mutex> lk(p->mu);
    for (;;) {
        if (l->quit) return;
        if (l->failed != RVB_OK) {
            // every pending and later job of a failed lane returns its failure; the other lanes go on
            for (uint64_t id : l->ids) finish(p, id, l->failed, l->failure, nullptr);
            l->ids.clear();
            l->inbox.clear();
            p->done.notify_all();
            l->wake.wait(lk);
            continue;
        }
        if (!l->inbox.empty()) {
            std::deque<Job> in;
            in.swap(l->inbox);
            l->allow = UINT64_MAX;                // (lane_submit itself traces complete units / groups only)
            lk.unlock();
            int rc = RVB_OK;
            for (const Job & j : in)
                if ((rc = lane_submit(l, j)) != RVB_OK) break;
            lk.lock();
            if (rc != RVB_OK) { l->failed = rc; l->failure = "lane " + std::to_string(l->index) + ": " + l->error; }
            continue;
        }
        if (l->submitted > l->returned) {
            // the oldest job goes on when its group / unit is complete, or when the caller waits for it (or for a later job): an incomplete
            // last unit is traced then, not as soon as its first job arrives
            const uint64_t gj = l->group * l->pairs;
            uint64_t waited = 0;
            while (waited < l->ids.size() && l->ids[(size_t) waited] < p->wanted) ++waited;
            l->allow = std::min(l->submitted, std::max(l->submitted / gj * gj, (l->returned + waited + gj - 1) / gj * gj));
            if (l->returned < l->allow) {
                lk.unlock();
                rvb_pipeline_result r;
                const int rc = lane_next(l, &r);
                lk.lock();
                if (rc != RVB_OK) { l->failed = rc; l->failure = "lane " + std::to_string(l->index) + ": " + l->error; continue; }
                finish(p, l->ids.front(), RVB_OK, std::string(), &r);
                l->ids.pop_front();
                p->done.notify_all();
                continue;
            }
        }
        l->wake.wait(lk);
    }
}

// a lane's thread: sets the lane up, serves it, drains it — every call on the lane's contexts is made here
void lane_main(rvb_pipeline * p, Lane * l, uint64_t group)
{
    const int rc = lane_init(l, l->init_ctxs.data(), l->init_ctxs.size(), group, p->pairs);
    {
        std::unique_lock<std::mutex> lk(p->mu);
        l->init_rc = rc;
        l->initialised = true;
        p->done.notify_all();
        if (rc != RVB_OK) l->wake.wait(lk, [l] { return l->quit; });
    }
    if (rc == RVB_OK) lane_thread(p, l);
    lane_drain(l);
}

int configure_common(rvb_pipeline * p, int which, int remove_direct, int trim_predelay, float sample_rate, int mode, uint64_t nreflections,
                     const float air[8])
{
    if (rvb_pipeline_pending(p) != 0) return pfail(p, RVB_ERR_STATE, "rvb_pipeline_configure: jobs are pending");
    if (which < 1 || which > 3) return pfail(p, RVB_ERR_INVALID, "rvb_pipeline_configure: which must be 1..3");
    if (mode != RVB_IR_FAST && mode != RVB_IR_EXACT) return pfail(p, RVB_ERR_INVALID, "rvb_pipeline_configure: unknown mode");
    if (!air || nreflections == 0 || !(sample_rate > 0.0f)) return pfail(p, RVB_ERR_INVALID, "rvb_pipeline_configure: reflections, sample rate, air coefficients");
    Config & c = p->cfg;
    c.which = which; c.remove_direct = remove_direct; c.trim_predelay = trim_predelay; c.sample_rate = sample_rate; c.mode = mode;
    c.nreflections = nreflections;
    std::memcpy(c.air, air, sizeof(c.air));
    c.configured = true;
    return RVB_OK;
}

// rvb_pipeline_create: the lane's failure is the pipeline's
int inline_rc(rvb_pipeline * p, int rc)
{
    if (rc != RVB_OK) p->error = p->lanes[0]->error;
    return rc;
}

}  // namespace

extern "C" {

int rvb_pipeline_create(rvb_pipeline ** out, rvb_ctx ** ctxs, uint64_t count, uint64_t group)
{
    if (!out || !ctxs || count == 0 || count > 64) return RVB_ERR_INVALID;
    *out = nullptr;
    for (uint64_t i = 0; i < count; ++i) {
        if (!ctxs[i]) return RVB_ERR_INVALID;
        for (uint64_t k = 0; k < i; ++k)
            if (ctxs[k] == ctxs[i]) return RVB_ERR_INVALID;
    }
    rvb_pipeline * p = new rvb_pipeline();
    p->lanes.emplace_back(new Lane());
    Lane * l = p->lanes[0].get();
    l->cfg = &p->cfg;
    const int rc = lane_init(l, ctxs, count, group, 1);
    if (rc != RVB_OK) { rvb_pipeline_destroy(p); return rc; }
    l->ring.resize((size_t) (2 * count));
    p->ncontexts = count;
    p->limit = 4 * count;
    *out = p;
    return RVB_OK;
}

int rvb_pipeline_create_lanes(rvb_pipeline ** out, rvb_ctx ** ctxs, uint64_t count, const uint64_t * lane_sizes, uint64_t nlanes,
                              const rvb_pipeline_options * options)
{
    if (!out) return RVB_ERR_INVALID;
    *out = nullptr;
    if (!ctxs || !lane_sizes || count == 0 || count > 64 || nlanes == 0 || nlanes > count) return RVB_ERR_INVALID;
    uint64_t total = 0;
    for (uint64_t i = 0; i < nlanes; ++i) {
        if (lane_sizes[i] == 0) return RVB_ERR_INVALID;
        total += lane_sizes[i];
    }
    if (total != count) return RVB_ERR_INVALID;
    for (uint64_t i = 0; i < count; ++i) {
        if (!ctxs[i]) return RVB_ERR_INVALID;
        for (uint64_t k = 0; k < i; ++k)
            if (ctxs[k] == ctxs[i]) return RVB_ERR_INVALID;
    }
    const uint64_t group = options ? options->group : 0;
    const uint64_t pairs = options ? options->pairs_per_launch : 1;
    if (pairs == 0 || pairs > RVB_PIPELINE_MAX_PAIRS || (pairs > 1 && group > 1)) return RVB_ERR_INVALID;
    rvb_pipeline * p = new rvb_pipeline();
    p->threaded = true;
    p->pairs = pairs;
    p->ncontexts = count;
    p->limit = 2 * count * pairs;
    // a result stays valid until count x pairs further results have been taken; a lane's ring slot is used again RING x lanes jobs later
    // (units go round-robin over the lanes): RING x lanes >= pending limit + that window
    const uint64_t window = count * pairs;
    const uint64_t ring = ((p->limit + window + nlanes - 1) / nlanes + pairs - 1) / pairs * pairs;
    uint64_t first = 0;
    for (uint64_t i = 0; i < nlanes; ++i) {
        p->lanes.emplace_back(new Lane());
        Lane * l = p->lanes.back().get();
        l->cfg = &p->cfg;
        l->index = i;
        l->init_ctxs.assign(ctxs + first, ctxs + first + lane_sizes[i]);
        l->ring.resize((size_t) ring);
        first += lane_sizes[i];
    }
    for (std::unique_ptr<Lane> & l : p->lanes) l->worker = std::thread(lane_main, p, l.get(), group);
    int rc = RVB_OK;
    {
        std::unique_lock<std::mutex> lk(p->mu);
        for (std::unique_ptr<Lane> & l : p->lanes) {
            Lane * lp = l.get();
            p->done.wait(lk, [lp] { return lp->initialised; });
            if (lp->init_rc != RVB_OK && rc == RVB_OK) rc = lp->init_rc;
        }
    }
    if (rc != RVB_OK) { rvb_pipeline_destroy(p); return rc; }
    *out = p;
    return RVB_OK;
}

void rvb_pipeline_destroy(rvb_pipeline * p)
{
    if (!p) return;
    if (p->threaded) {
        // the lane threads finish the stage they are in, wait for their contexts and free their buffers
        {
            std::lock_guard<std::mutex> lk(p->mu);
            for (std::unique_ptr<Lane> & l : p->lanes) { l->quit = true; l->wake.notify_all(); }
        }
        for (std::unique_ptr<Lane> & l : p->lanes)
            if (l->worker.joinable()) l->worker.join();
    } else {
        for (std::unique_ptr<Lane> & l : p->lanes) lane_drain(l.get());
    }
    delete p;
}

const char * rvb_pipeline_last_error(const rvb_pipeline * p) { return p ? p->error.c_str() : ""; }

int rvb_pipeline_configure_speakers(rvb_pipeline * p, const rvb_speaker * speakers, uint64_t nspeakers, int which, int remove_direct,
                                    int trim_predelay, float sample_rate, int mode, uint64_t nreflections, const float air_coefficient[8])
{
    if (!p) return RVB_ERR_INVALID;
    if (!speakers || nspeakers == 0 || nspeakers > RVB_MAX_SPEAKERS) return pfail(p, RVB_ERR_INVALID, "rvb_pipeline_configure_speakers: 1.." RVB_STR(RVB_MAX_SPEAKERS) " speakers required");
    std::lock_guard<std::mutex> lk(p->mu);        // (the lane threads read the configuration while jobs are pending: none are)
    const int rc = configure_common(p, which, remove_direct, trim_predelay, sample_rate, mode, nreflections, air_coefficient);
    if (rc != RVB_OK) return rc;
    p->cfg.hrtf = false;
    p->cfg.speakers.assign(speakers, speakers + nspeakers);
    return RVB_OK;
}

int rvb_pipeline_configure_hrtf(rvb_pipeline * p, const float * table, const float facing[3], const float up[3], int which, int remove_direct,
                                int trim_predelay, float sample_rate, int mode, uint64_t nreflections, const float air_coefficient[8])
{
    if (!p) return RVB_ERR_INVALID;
    if (!table || !facing || !up) return pfail(p, RVB_ERR_INVALID, "rvb_pipeline_configure_hrtf: null argument");
    std::lock_guard<std::mutex> lk(p->mu);
    const int rc = configure_common(p, which, remove_direct, trim_predelay, sample_rate, mode, nreflections, air_coefficient);
    if (rc != RVB_OK) return rc;
    p->cfg.hrtf = true;
    p->cfg.table.assign(table, table + (size_t) 2 * 360 * 180 * 8);
    for (std::unique_ptr<Lane> & l : p->lanes)
        for (Slot & s : l->slots) s.has_table = false;
    std::memcpy(p->cfg.facing, facing, sizeof(p->cfg.facing));
    std::memcpy(p->cfg.up, up, sizeof(p->cfg.up));
    return RVB_OK;
}

static bool usable_direction(const float d[3])
{
    // what rvb_set_source_pattern accepts: finite, and a length binary32 can normalise
    for (int i = 0; i < 3; ++i)
        if (!std::isfinite(d[i])) return false;
    const float len = std::sqrt(d[0] * d[0] + d[1] * d[1] + d[2] * d[2]);
    return len > 0.0f && std::isfinite(len);
}

int rvb_pipeline_set_source_pattern(rvb_pipeline * p, const float shape[8], const float direction[3])
{
    if (!p) return RVB_ERR_INVALID;
    std::lock_guard<std::mutex> lk(p->mu);        // (the lane threads read the configuration while jobs are pending: none are)
    if (p->threaded ? p->submitted != p->returned : p->lanes[0]->submitted != p->lanes[0]->returned)
        return pfail(p, RVB_ERR_STATE, "rvb_pipeline_set_source_pattern: jobs are pending");
    Config & c = p->cfg;
    if (shape) {
        if (!direction) return pfail(p, RVB_ERR_INVALID, "rvb_pipeline_set_source_pattern: a shape needs a direction");
        for (int b = 0; b < 8; ++b)
            if (!std::isfinite(shape[b])) return pfail(p, RVB_ERR_INVALID, "rvb_pipeline_set_source_pattern: a shape is not finite");
        if (!usable_direction(direction)) return pfail(p, RVB_ERR_INVALID, "rvb_pipeline_set_source_pattern: the direction is not finite or has zero length");
        std::memcpy(c.source_shape, shape, sizeof(c.source_shape));
        std::memcpy(c.source_direction, direction, sizeof(c.source_direction));
    }
    c.source_on = shape != nullptr;
    c.source_managed = true;
    return RVB_OK;
}

int rvb_pipeline_submit_oriented(rvb_pipeline * p, const float mic[3], const float source[3], const float facing[3], const float up[3])
{
    return rvb_pipeline_submit_directed(p, mic, source, facing, up, nullptr);
}

int rvb_pipeline_submit_directed(rvb_pipeline * p, const float mic[3], const float source[3], const float facing[3], const float up[3],
                                 const float source_direction[3])
{
    if (!p) return RVB_ERR_INVALID;
    if (!p->cfg.configured) return pfail(p, RVB_ERR_STATE, "rvb_pipeline_submit: rvb_pipeline_configure_* first");
    if (!mic || !source) return pfail(p, RVB_ERR_INVALID, "rvb_pipeline_submit: null argument");
    if (source_direction && !p->cfg.source_on) return pfail(p, RVB_ERR_STATE, "rvb_pipeline_submit_directed: rvb_pipeline_set_source_pattern first");
    if (source_direction && !usable_direction(source_direction))
        return pfail(p, RVB_ERR_INVALID, "rvb_pipeline_submit_directed: the source direction is not finite or has zero length");
    if (rvb_pipeline_pending(p) >= p->limit)
        return pfail(p, RVB_ERR_CAPACITY, p->threaded ? "rvb_pipeline_submit: take results first (2 x contexts x pairs per launch jobs are pending)"
                                                      : "rvb_pipeline_submit: take results first (4 x contexts jobs are pending)");
    Job j;
    std::memcpy(j.mic, mic, sizeof(j.mic));
    std::memcpy(j.source, source, sizeof(j.source));
    std::memcpy(j.facing, facing ? facing : p->cfg.facing, sizeof(j.facing));
    std::memcpy(j.up, up ? up : p->cfg.up, sizeof(j.up));
    std::memcpy(j.source_direction, source_direction ? source_direction : p->cfg.source_direction, sizeof(j.source_direction));
    if (!p->threaded) return inline_rc(p, lane_submit(p->lanes[0].get(), j));
    // unit u (pairs per launch consecutive jobs) goes to lane u % lanes; the lane's thread takes it from there
    std::lock_guard<std::mutex> lk(p->mu);
    const uint64_t id = p->submitted;
    Lane * l = p->lanes[(size_t) ((id / p->pairs) % p->lanes.size())].get();
    p->outcomes.emplace_back();
    l->inbox.push_back(j);
    l->ids.push_back(id);
    ++p->submitted;
    l->wake.notify_all();
    return RVB_OK;
}

int rvb_pipeline_submit(rvb_pipeline * p, const float mic[3], const float source[3])
{
    return rvb_pipeline_submit_oriented(p, mic, source, nullptr, nullptr);
}

uint64_t rvb_pipeline_pending(const rvb_pipeline * p)
{
    if (!p) return 0;
    if (p->threaded) return p->submitted - p->returned;
    return p->lanes[0]->submitted - p->lanes[0]->returned;
}

int rvb_pipeline_next(rvb_pipeline * p, rvb_pipeline_result * out)
{
    if (!p || !out) return RVB_ERR_INVALID;
    if (rvb_pipeline_pending(p) == 0) return pfail(p, RVB_ERR_STATE, "rvb_pipeline_next: nothing is pending");
    if (!p->threaded) return inline_rc(p, lane_next(p->lanes[0].get(), out));
    std::unique_lock<std::mutex> lk(p->mu);
    if (p->wanted <= p->returned) {
        p->wanted = p->returned + 1;
        for (std::unique_ptr<Lane> & l : p->lanes) l->wake.notify_all();
    }
    p->done.wait(lk, [p] { return p->outcomes.front().ready; });
    const Outcome o = p->outcomes.front();
    p->outcomes.pop_front();
    ++p->returned;
    if (o.rc != RVB_OK) return pfail(p, o.rc, o.error);
    *out = o.result;
    return RVB_OK;
}

}  // extern "C"
