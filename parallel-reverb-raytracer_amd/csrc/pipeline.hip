// pipeline.hip — impulse responses back to back behind the C-ABI (rvb_pipeline_* of include/rvb_capi.h): the schedule that
// bench.py times, for a C / C++ caller.  What it replaces for a batch caller is the reference's cmd/main.cpp:241-298 in a loop — one
// Raytracer::raytrace, one Attenuator::attenuate per channel, fixPredelay, flattenImpulses per impulse response, each stage blocking.
//
// The trace of an impulse response is bound by vector issue, its record grouping and binning by memory, its image-source merge and its
// configuration by the host.  So several contexts of one GPU (the caller's: same scene, same rays on each) take turns — a LANE
// (csrc/pipeline_lane.h, csrc/pipeline_lane.hip), whose schedule counts in UNITS (csrc/pipeline_schedule.h):
//   * a unit is `pairs` consecutive jobs traced by ONE launch on one context (rvb_trace_pairs; one job and rvb_trace where pairs is 1),
//     staged pair by pair (rvb_ir_select_pair), each into a device histogram of its own; units go round-robin over the contexts;
//   * units of one pair are traced in GROUPS of `group` contexts — one path-kernel launch for the group (rvb_trace_group): more waves
//     per SIMD for the latency-bound bounce chains;
//   * the traces of the group after next are enqueued before the current group is finished, so a path kernel is (nearly) always
//     resident and the other stages of the previous group run beside it;
//   * the binning stages of ALL impulse responses of a group are enqueued — each behind its own trace's image-source candidates —
//     before the host waits for any of them;
//   * every finished histogram leaves for a pinned host buffer of the lane's ring on the context's export stream, bin range by bin
//     range (rvb_ir_accumulate_export); the lane's next result is there when the oldest job's histogram has landed.
// This file: the entry points, the configuration, and who drives a lane.  rvb_pipeline_create drives one lane in the caller's thread.
// rvb_pipeline_create_lanes drives several, each from a host thread of its own (the only thread that touches the lane and its
// contexts) that the caller posts to through a Mailbox; unit u goes to lane u % lanes, results come back in submission order.
#include "pipeline_lane.h"

#include <cmath>
#include <condition_variable>
#include <cstring>
#include <memory>
#include <mutex>
#include <thread>

namespace {
struct Mailbox {                              // what a lane's thread shares with the caller's: guarded by rvb_pipeline::mu, all of it
    bool initialised = false, quit = false;
    int init_rc = RVB_OK;                     // lane_init's, once `initialised`
    std::condition_variable wake;
    std::deque<Job> inbox;                    // submitted by the caller, not yet handed to the lane
    std::deque<uint64_t> ids;                 // pipeline job numbers of the lane's jobs [returned, submitted) and of the inbox
    int failed = RVB_OK;                      // a stage failed: every pending and later job of the lane returns this code
    std::string failure;
};

struct Post {                                 // a lane and who drives it
    Lane lane;
    Mailbox box;
    uint64_t index = 0;
    std::thread worker;                       // rvb_pipeline_create_lanes only
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
    std::vector<std::unique_ptr<Post>> lanes;
    bool threaded = false;                    // the caller posts to lane threads (rvb_pipeline_create_lanes) or runs the one lane itself
    uint64_t pairs = 1;
    sched::Capacity capacity{0, 0, 0};
    const char * full = "";                   // the text of RVB_ERR_CAPACITY
    std::string error;
    uint64_t submitted = 0, returned = 0;     // the caller's count, in both modes: pending = submitted - returned
    // rvb_pipeline_create_lanes: the caller's side
    std::mutex mu;
    std::condition_variable done;
    std::deque<Outcome> outcomes;             // jobs [returned, submitted)
    uint64_t wanted = 0;                      // rvb_pipeline_next waits for the jobs below it
};

namespace {
// (p->mu held) a job's result or failure for the caller
void finish(rvb_pipeline * p, uint64_t id, int rc, const std::string & error, const rvb_pipeline_result * r)
{
    Outcome & o = p->outcomes[(size_t) (id - p->returned)];
    o.ready = true; o.rc = rc; o.error = error;
    if (r) { o.result = *r; o.result.job = id; }
}

void lane_thread(rvb_pipeline * p, Post * post)
{
    Lane * l = &post->lane;
    Mailbox & b = post->box;
    std::unique_lock<std::mutex> lk(p->mu);
    auto fail = [&](int rc) { b.failed = rc; b.failure = "lane " + std::to_string(post->index) + ": " + l->error; };
    for (;;) {
        if (b.quit) return;
        if (b.failed != RVB_OK) {
            // every pending and later job of a failed lane returns its failure; the other lanes go on
            for (uint64_t id : b.ids) finish(p, id, b.failed, b.failure, nullptr);
            b.ids.clear();
            b.inbox.clear();
            p->done.notify_all();
            b.wake.wait(lk);
            continue;
        }
        if (!b.inbox.empty()) {
            std::deque<Job> in;
            in.swap(b.inbox);
            l->allow = UINT64_MAX;                // (lane_submit itself traces complete groups only)
            lk.unlock();
            int rc = RVB_OK;
            for (const Job & j : in)
                if ((rc = lane_submit(l, j)) != RVB_OK) break;
            lk.lock();
            if (rc != RVB_OK) fail(rc);
            continue;
        }
        if (l->submitted > l->returned) {
            uint64_t waited = 0;                  // how many of the lane's jobs the caller waits for (or for a later job)
            while (waited < b.ids.size() && b.ids[(size_t) waited] < p->wanted) ++waited;
            l->allow = sched::allow(l->shape, l->submitted, l->returned, waited);
            if (l->returned < l->allow) {
                lk.unlock();
                rvb_pipeline_result r;
                const int rc = lane_next(l, &r);
                lk.lock();
                if (rc != RVB_OK) { fail(rc); continue; }
                finish(p, b.ids.front(), RVB_OK, std::string(), &r);
                b.ids.pop_front();
                p->done.notify_all();
                continue;
            }
        }
        b.wake.wait(lk);
    }
}

// a lane's thread: sets the lane up, serves it, drains it — every call on the lane's contexts is made here
void lane_main(rvb_pipeline * p, Post * post, uint64_t group)
{
    const int rc = lane_init(&post->lane, group, p->pairs, p->capacity.ring);
    {
        std::unique_lock<std::mutex> lk(p->mu);
        post->box.init_rc = rc;
        post->box.initialised = true;
        p->done.notify_all();
        if (rc != RVB_OK) post->box.wake.wait(lk, [post] { return post->box.quit; });
    }
    if (rc == RVB_OK) lane_thread(p, post);
    lane_drain(&post->lane);
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
int inline_rc(rvb_pipeline * p, int rc) { return rc != RVB_OK ? pfail(p, rc, p->lanes[0]->lane.error) : rc; }

// the contexts of a pipeline: 1 .. 64, none null, none twice
bool usable_contexts(rvb_ctx ** ctxs, uint64_t count)
{
    if (!ctxs || count == 0 || count > 64) return false;
    for (uint64_t i = 0; i < count; ++i)
        for (uint64_t k = 0; k <= i; ++k)
            if (!ctxs[i] || (k < i && ctxs[k] == ctxs[i])) return false;
    return true;
}

Post * add_lane(rvb_pipeline * p, rvb_ctx ** ctxs, uint64_t count)
{
    p->lanes.emplace_back(new Post());
    Post * post = p->lanes.back().get();
    post->lane.cfg = &p->cfg;
    post->index = p->lanes.size() - 1;
    post->lane.slots.resize((size_t) count);
    for (uint64_t i = 0; i < count; ++i) post->lane.slots[(size_t) i].ctx = ctxs[i];
    return post;
}
}  // namespace

extern "C" {
int rvb_pipeline_create(rvb_pipeline ** out, rvb_ctx ** ctxs, uint64_t count, uint64_t group)
{
    if (!out || !usable_contexts(ctxs, count)) return RVB_ERR_INVALID;
    *out = nullptr;
    rvb_pipeline * p = new rvb_pipeline();
    p->capacity = sched::capacity_inline(count);
    p->full = "rvb_pipeline_submit: take results first (4 x contexts jobs are pending)";
    const int rc = lane_init(&add_lane(p, ctxs, count)->lane, group, 1, p->capacity.ring);
    if (rc != RVB_OK) { rvb_pipeline_destroy(p); return rc; }
    *out = p;
    return RVB_OK;
}

int rvb_pipeline_create_lanes(rvb_pipeline ** out, rvb_ctx ** ctxs, uint64_t count, const uint64_t * lane_sizes, uint64_t nlanes,
                              const rvb_pipeline_options * options)
{
    if (!out) return RVB_ERR_INVALID;
    *out = nullptr;
    if (!usable_contexts(ctxs, count) || !lane_sizes || nlanes == 0 || nlanes > count) return RVB_ERR_INVALID;
    uint64_t total = 0;
    for (uint64_t i = 0; i < nlanes; total += lane_sizes[i++])
        if (lane_sizes[i] == 0) return RVB_ERR_INVALID;
    if (total != count) return RVB_ERR_INVALID;
    const uint64_t group = options ? options->group : 0;
    const uint64_t pairs = options ? options->pairs_per_launch : 1;
    if (pairs == 0 || pairs > RVB_PIPELINE_MAX_PAIRS || (pairs > 1 && group > 1)) return RVB_ERR_INVALID;
    rvb_pipeline * p = new rvb_pipeline();
    p->threaded = true;
    p->pairs = pairs;
    p->capacity = sched::capacity_lanes(count, pairs, nlanes);
    p->full = "rvb_pipeline_submit: take results first (2 x contexts x pairs per launch jobs are pending)";
    for (uint64_t i = 0, first = 0; i < nlanes; first += lane_sizes[i++]) add_lane(p, ctxs + first, lane_sizes[i]);
    for (std::unique_ptr<Post> & l : p->lanes) l->worker = std::thread(lane_main, p, l.get(), group);
    int rc = RVB_OK;
    {
        std::unique_lock<std::mutex> lk(p->mu);
        for (std::unique_ptr<Post> & l : p->lanes) {
            Mailbox * b = &l->box;
            p->done.wait(lk, [b] { return b->initialised; });
            if (b->init_rc != RVB_OK && rc == RVB_OK) rc = b->init_rc;
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
            for (std::unique_ptr<Post> & l : p->lanes) { l->box.quit = true; l->box.wake.notify_all(); }
        }
        for (std::unique_ptr<Post> & l : p->lanes)
            if (l->worker.joinable()) l->worker.join();
    } else for (std::unique_ptr<Post> & l : p->lanes) lane_drain(&l->lane);
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
    for (std::unique_ptr<Post> & l : p->lanes)
        for (Slot & s : l->lane.slots) s.has_table = false;   // (no jobs are pending: the lanes are idle)
    std::memcpy(p->cfg.facing, facing, sizeof(p->cfg.facing));
    std::memcpy(p->cfg.up, up, sizeof(p->cfg.up));
    return RVB_OK;
}

static bool usable_direction(const float d[3])      // what rvb_set_source_pattern accepts: finite, and a length binary32 can normalise
{
    const float len = std::sqrt(d[0] * d[0] + d[1] * d[1] + d[2] * d[2]);
    return std::isfinite(d[0]) && std::isfinite(d[1]) && std::isfinite(d[2]) && len > 0.0f && std::isfinite(len);
}

int rvb_pipeline_set_source_pattern(rvb_pipeline * p, const float shape[8], const float direction[3])
{
    if (!p) return RVB_ERR_INVALID;
    std::lock_guard<std::mutex> lk(p->mu);        // (the lane threads read the configuration while jobs are pending: none are)
    if (rvb_pipeline_pending(p) != 0) return pfail(p, RVB_ERR_STATE, "rvb_pipeline_set_source_pattern: jobs are pending");
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

int rvb_pipeline_submit_oriented(rvb_pipeline * p, const float mic[3], const float source[3], const float facing[3], const float up[3]) { return rvb_pipeline_submit_directed(p, mic, source, facing, up, nullptr); }

int rvb_pipeline_submit_directed(rvb_pipeline * p, const float mic[3], const float source[3], const float facing[3], const float up[3],
                                 const float source_direction[3])
{
    if (!p) return RVB_ERR_INVALID;
    if (!p->cfg.configured) return pfail(p, RVB_ERR_STATE, "rvb_pipeline_submit: rvb_pipeline_configure_* first");
    if (!mic || !source) return pfail(p, RVB_ERR_INVALID, "rvb_pipeline_submit: null argument");
    if (source_direction && !p->cfg.source_on) return pfail(p, RVB_ERR_STATE, "rvb_pipeline_submit_directed: rvb_pipeline_set_source_pattern first");
    if (source_direction && !usable_direction(source_direction))
        return pfail(p, RVB_ERR_INVALID, "rvb_pipeline_submit_directed: the source direction is not finite or has zero length");
    if (rvb_pipeline_pending(p) >= p->capacity.limit) return pfail(p, RVB_ERR_CAPACITY, p->full);
    Job j;
    std::memcpy(j.mic, mic, sizeof(j.mic));
    std::memcpy(j.source, source, sizeof(j.source));
    std::memcpy(j.facing, facing ? facing : p->cfg.facing, sizeof(j.facing));
    std::memcpy(j.up, up ? up : p->cfg.up, sizeof(j.up));
    std::memcpy(j.source_direction, source_direction ? source_direction : p->cfg.source_direction, sizeof(j.source_direction));
    const uint64_t id = p->submitted++;
    if (!p->threaded) return inline_rc(p, lane_submit(&p->lanes[0]->lane, j));
    // unit u (pairs per launch consecutive jobs) goes to lane u % lanes; the lane's thread takes it from there
    std::lock_guard<std::mutex> lk(p->mu);
    Mailbox & b = p->lanes[(size_t) ((id / p->pairs) % p->lanes.size())]->box;
    p->outcomes.emplace_back();
    b.inbox.push_back(j);
    b.ids.push_back(id);
    b.wake.notify_all();
    return RVB_OK;
}

int rvb_pipeline_submit(rvb_pipeline * p, const float mic[3], const float source[3]) { return rvb_pipeline_submit_directed(p, mic, source, nullptr, nullptr, nullptr); }

uint64_t rvb_pipeline_pending(const rvb_pipeline * p) { return p ? p->submitted - p->returned : 0; }

int rvb_pipeline_next(rvb_pipeline * p, rvb_pipeline_result * out)
{
    if (!p || !out) return RVB_ERR_INVALID;
    if (rvb_pipeline_pending(p) == 0) return pfail(p, RVB_ERR_STATE, "rvb_pipeline_next: nothing is pending");
    if (!p->threaded) {
        const int rc = inline_rc(p, lane_next(&p->lanes[0]->lane, out));
        if (rc == RVB_OK) ++p->returned;          // (a failed stage leaves the job pending: the next call takes it up again)
        return rc;
    }
    std::unique_lock<std::mutex> lk(p->mu);
    if (p->wanted <= p->returned) {
        p->wanted = p->returned + 1;
        for (std::unique_ptr<Post> & l : p->lanes) l->box.wake.notify_all();
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
