// pipeline_order — the call order of the native impulse-response pipeline (rvb_pipeline_*, csrc/pipeline*.hip) without a GPU.
// This program defines the 14 hip* functions and the rvb_* functions of the public C-ABI that the pipeline calls, links neither
// librvb_hip.so nor the HIP runtime, and drives the pipeline through ten named scenarios.  Every call is logged to the context it
// names, with the integer arguments that define the schedule and never an array or a float (as tests/test_distributed_call_order.py
// does for distributed.IrPipeline); a job's mic[0] carries its job number.  Printed per scenario: one sequence per context, then
// the results in the order they came back.  tests/test_pipeline_order_host.py builds it with the sanitizers, runs it and holds
// stdout against tests/golden/pipeline_call_order.txt.  A broken invariant goes to stderr and the exit code.  No argument.
#include "rvb_capi.h"

#include <hip/hip_runtime.h>

#include <cmath>
#include <condition_variable>
#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <deque>
#include <map>
#include <mutex>
#include <string>
#include <vector>

// ---- the stand-ins ---------------------------------------------------------------------------------------------------------------------

struct rvb_ctx {                                  // touched by the thread that drives its lane only (main reads it after the destroy)
    int slot = 0, device = 0;
    std::vector<std::string> log;
    std::string error;
    uint64_t traces = 0, nreflections = 0, pair = 0, nchannels = 0, exports = 0;
    uint64_t fail_export = 0;                     // the failure switch: the k-th rvb_ir_accumulate_export fails (0: none)
    std::vector<long> launch;                     // the job of every pair of the last launch
    long configured = -1;                         // the job of the last rvb_ir_configure_*
    bool has_table = false;
};

namespace {

const uint64_t RAYS = 6;                          // per pair
const float RATE = 1000.0f;
const char * FAILURE = "rvb_ir_accumulate_export: the harness's failure switch";

struct JobRec { int traced = 0, ctx = -1, staged = 0; };
struct View { size_t bytes; long job; };
struct Event { int slot = -1; };

struct Harness {                                  // what several threads share
    std::mutex mu;
    std::condition_variable gate_cv;
    bool gate_open = true;                        // closed: every logged call waits (a lanes scenario submits a batch, then opens)
    std::map<void *, size_t> blocks;              // hipMalloc, hipHostMalloc
    std::map<const void *, View> views;           // pinned histograms that are pending or inside their validity window
    std::map<long, JobRec> jobs;
    int violations = 0;
} H;

thread_local std::vector<std::string> fill_log;   // the fill stream's calls, until rvb_wait_for_event names the context they serve

void violation(const std::string & what)          // (H.mu held or not: stderr only)
{
    std::fprintf(stderr, "VIOLATION: %s\n", what.c_str());
    ++H.violations;
}

std::string fmt(const char * f, ...)
{
    char buf[256];
    va_list ap;
    va_start(ap, f);
    std::vsnprintf(buf, sizeof(buf), f, ap);
    va_end(ap);
    return buf;
}

void logc(rvb_ctx * c, const std::string & entry)
{
    {
        std::unique_lock<std::mutex> lk(H.mu);
        H.gate_cv.wait(lk, [] { return H.gate_open; });
    }
    c->log.push_back(entry);
}

void gate(bool open)
{
    std::lock_guard<std::mutex> lk(H.mu);
    H.gate_open = open;
    H.gate_cv.notify_all();
}

void traced(rvb_ctx * c, const float * mics, uint64_t npairs, uint64_t nreflections)
{
    ++c->traces;
    c->nreflections = nreflections;
    c->pair = 0;
    c->launch.clear();
    std::lock_guard<std::mutex> lk(H.mu);
    for (uint64_t k = 0; k < npairs; ++k) {
        const long job = (long) mics[3 * k];
        c->launch.push_back(job);
        JobRec & r = H.jobs[job];
        ++r.traced;
        r.ctx = c->slot;
    }
}

std::string jobs_of(const float * mics, uint64_t n)
{
    std::string s;
    for (uint64_t k = 0; k < n; ++k) s += (k ? "," : "") + std::to_string((long) mics[3 * k]);
    return s;
}

uint64_t candidates_of(const rvb_ctx * c, uint64_t pair) { return 1 + ((uint64_t) c->slot + c->traces + pair) % 4; }

int configured(rvb_ctx * c, const float mic[3], uint64_t nchannels, const std::string & entry)
{
    const long job = (long) mic[0];
    logc(c, entry);
    std::lock_guard<std::mutex> lk(H.mu);
    const JobRec & r = H.jobs[job];
    if (r.traced < 1 || r.ctx != c->slot) violation(fmt("job %ld staged on context %d before it was traced there", job, c->slot));
    if (c->pair >= c->launch.size() || c->launch[(size_t) c->pair] != job) violation(fmt("job %ld staged while another pair is selected", job));
    c->configured = job;
    c->nchannels = nchannels;
    return RVB_OK;
}

}  // namespace

extern "C" {

// ---- HIP: memory is malloc and free, streams and events are small heap objects ----------------------------------------------------------
hipError_t hipSetDevice(int) { return hipSuccess; }
const char * hipGetErrorString(hipError_t) { return "no error"; }
static hipError_t block(void ** p, size_t bytes)
{
    *p = std::malloc(bytes);
    std::lock_guard<std::mutex> lk(H.mu);
    H.blocks[*p] = bytes;
    return hipSuccess;
}
static hipError_t unblock(void * p)
{
    {
        std::lock_guard<std::mutex> lk(H.mu);
        if (H.views.count(p)) violation(fmt("the histogram of job %ld was freed while pending or inside its validity window", H.views[p].job));
        H.blocks.erase(p);
    }
    std::free(p);
    return hipSuccess;
}
hipError_t hipMalloc(void ** p, size_t bytes) { return block(p, bytes); }
hipError_t hipHostMalloc(void ** p, size_t bytes, unsigned int) { return block(p, bytes); }
hipError_t hipFree(void * p) { return unblock(p); }
hipError_t hipHostFree(void * p) { return unblock(p); }
hipError_t hipStreamCreateWithFlags(hipStream_t * s, unsigned int) { *s = reinterpret_cast<hipStream_t>(new int(0)); return hipSuccess; }
hipError_t hipStreamDestroy(hipStream_t s) { delete reinterpret_cast<int *>(s); return hipSuccess; }
hipError_t hipStreamSynchronize(hipStream_t) { return hipSuccess; }
hipError_t hipEventCreateWithFlags(hipEvent_t * e, unsigned int) { *e = reinterpret_cast<hipEvent_t>(new Event()); return hipSuccess; }
hipError_t hipEventDestroy(hipEvent_t e) { delete reinterpret_cast<Event *>(e); return hipSuccess; }
hipError_t hipMemsetAsync(void * p, int value, size_t bytes, hipStream_t)
{
    std::memset(p, value, bytes);
    fill_log.push_back("hipMemsetAsync");
    return hipSuccess;
}
hipError_t hipEventRecord(hipEvent_t, hipStream_t) { fill_log.push_back("hipEventRecord"); return hipSuccess; }

}  // extern "C"

namespace { std::vector<rvb_ctx *> * slots = nullptr; }     // the scenario's contexts by slot (hipEventSynchronize logs to the event's)

extern "C" {

hipError_t hipEventSynchronize(hipEvent_t e)
{
    const int slot = reinterpret_cast<Event *>(e)->slot;
    if (slot < 0) violation("hipEventSynchronize on an event that no context has recorded");
    else logc((*slots)[(size_t) slot], "hipEventSynchronize");
    return hipSuccess;
}

// ---- the C-ABI below the pipeline --------------------------------------------------------------------------------------------------------
const char * rvb_last_error(const rvb_ctx * c) { return c ? c->error.c_str() : ""; }
int rvb_device_index(rvb_ctx * c, int * device) { logc(c, "rvb_device_index"); *device = c->device; return RVB_OK; }
int rvb_synchronize(rvb_ctx * c) { logc(c, "rvb_synchronize"); return RVB_OK; }
int rvb_synchronize_exports(rvb_ctx * c) { logc(c, "rvb_synchronize_exports"); return RVB_OK; }
int rvb_set_concurrent_traces(rvb_ctx * c, uint32_t traces) { logc(c, fmt("rvb_set_concurrent_traces traces=%u", traces)); return RVB_OK; }
int rvb_wait_for_event(rvb_ctx * c, void * e)
{
    static_cast<Event *>(e)->slot = c->slot;
    for (const std::string & entry : fill_log) logc(c, entry);
    fill_log.clear();
    logc(c, "rvb_wait_for_event");
    return RVB_OK;
}
int rvb_record_event(rvb_ctx * c, void * e) { static_cast<Event *>(e)->slot = c->slot; logc(c, "rvb_record_event"); return RVB_OK; }
int rvb_set_source_pattern(rvb_ctx * c, const rvb_source_pattern * patterns, uint64_t n)
{
    logc(c, fmt("rvb_set_source_pattern patterns=%llu null=%d", (unsigned long long) n, patterns ? 0 : 1));
    return RVB_OK;
}
int rvb_trace(rvb_ctx * c, const float mic[3], const float *, uint64_t nreflections, const float *, uint64_t)
{
    logc(c, fmt("rvb_trace job=%ld nreflections=%llu", (long) mic[0], (unsigned long long) nreflections));
    traced(c, mic, 1, nreflections);
    return RVB_OK;
}
int rvb_trace_pairs(rvb_ctx * c, const float * mics, const float *, uint64_t npairs, uint64_t nreflections, const float *, uint64_t)
{
    logc(c, fmt("rvb_trace_pairs jobs=%s nreflections=%llu", jobs_of(mics, npairs).c_str(), (unsigned long long) nreflections));
    traced(c, mics, npairs, nreflections);
    return RVB_OK;
}
int rvb_trace_group(rvb_ctx ** ctxs, uint64_t count, const float * mics, const float *, uint64_t nreflections, const float *, const uint64_t *)
{
    std::string names;
    for (uint64_t k = 0; k < count; ++k) names += (k ? "," : "") + std::to_string(ctxs[k]->slot);
    for (uint64_t k = 0; k < count; ++k) {        // logged to every context it names
        logc(ctxs[k], fmt("rvb_trace_group contexts=%s jobs=%s nreflections=%llu", names.c_str(), jobs_of(mics, count).c_str(), (unsigned long long) nreflections));
        traced(ctxs[k], mics + 3 * k, 1, nreflections);
    }
    return RVB_OK;
}
int rvb_ir_select_pair(rvb_ctx * c, uint64_t pair)
{
    logc(c, fmt("rvb_ir_select_pair pair=%llu", (unsigned long long) pair));
    if (pair >= c->launch.size()) { c->error = "rvb_ir_select_pair: no such pair"; return RVB_ERR_INVALID; }
    c->pair = pair;
    return RVB_OK;
}
int rvb_diffuse_device(rvb_ctx * c, const void ** d, uint64_t * count)
{
    logc(c, "rvb_diffuse_device");
    *d = nullptr;
    *count = c->launch.size() * RAYS * c->nreflections;
    return RVB_OK;
}
int rvb_get_direct(rvb_ctx * c, rvb_impulse * out) { logc(c, "rvb_get_direct"); std::memset(out, 0, sizeof(*out)); return RVB_OK; }
int rvb_get_image_candidates(rvb_ctx * c, rvb_image_candidate * out, uint64_t capacity, uint64_t * count)
{
    uint64_t total = 0;
    for (uint64_t p = 0; p < c->launch.size(); ++p) total += candidates_of(c, p);
    logc(c, fmt("rvb_get_image_candidates capacity=%llu -> %llu", (unsigned long long) capacity, (unsigned long long) total));
    *count = total;
    if (!out) return RVB_OK;
    if (capacity < total) { c->error = "rvb_get_image_candidates: capacity"; return RVB_ERR_CAPACITY; }
    for (uint64_t p = 0; p < c->launch.size(); ++p)
        for (uint64_t k = 0; k < candidates_of(c, p); ++k, ++out) {
            std::memset(out, 0, sizeof(*out));
            out->ray = p * RAYS + k;              // global ray numbers: pair = ray / rays per pair
            out->slot = (uint32_t) (1 + k);
            out->index = (uint32_t) (1 + p);
        }
    return RVB_OK;
}
int rvb_merge_images(const rvb_image_candidate * candidates, uint64_t n, const rvb_impulse *, int, rvb_impulse * out, uint64_t capacity, uint64_t * count)
{
    for (uint64_t k = 0; k < n; ++k)
        if (candidates[k].ray >= RAYS) violation("a candidate's ray number is not relative to its pair");
    *count = (n + 1) / 2;                         // keeps every second candidate
    if (!out) return RVB_OK;
    if (capacity < *count) return RVB_ERR_CAPACITY;
    for (uint64_t k = 0; k < n; k += 2) *out++ = candidates[k].impulse;
    return RVB_OK;
}
int rvb_ir_configure_speakers(rvb_ctx * c, const float mic[3], const rvb_speaker *, uint64_t nspeakers, int which, const rvb_impulse *, uint64_t nimages)
{
    return configured(c, mic, nspeakers, fmt("rvb_ir_configure_speakers job=%ld speakers=%llu which=%d images=%llu", (long) mic[0],
                                             (unsigned long long) nspeakers, which, (unsigned long long) nimages));
}
int rvb_ir_configure_hrtf(rvb_ctx * c, const float mic[3], const float * table, const float *, const float *, int which, const rvb_impulse *, uint64_t nimages)
{
    const int rc = configured(c, mic, 2, fmt("rvb_ir_configure_hrtf job=%ld table=%d which=%d images=%llu", (long) mic[0], table ? 1 : 0, which,
                                             (unsigned long long) nimages));
    if (!table && !c->has_table) { c->error = "rvb_ir_configure_hrtf: no table on the device"; return RVB_ERR_STATE; }
    c->has_table = true;
    return rc;
}
int rvb_ir_time_range_begin(rvb_ctx * c) { logc(c, "rvb_ir_time_range_begin"); return RVB_OK; }
int rvb_ir_time_range(rvb_ctx * c, float * lo, float * hi)
{
    logc(c, "rvb_ir_time_range");
    *lo = 0.010f + 0.001f * (float) c->slot;
    *hi = 0.050f + 0.004f * (float) ((c->traces * 3 + c->pair) % 7);
    return RVB_OK;
}
uint64_t rvb_ir_bins(float max_time, float predelay, float sample_rate) { return (uint64_t) std::ceil((max_time - predelay) * sample_rate) + 1; }
int rvb_ir_accumulate_export(rvb_ctx * c, float, float, uint64_t nbins, int mode, void * d_histogram, void * pinned_dst, uint32_t)
{
    const long job = c->configured;
    logc(c, fmt("rvb_ir_accumulate_export job=%ld nbins=%llu mode=%d", job, (unsigned long long) nbins, mode));
    if (++c->exports == c->fail_export) { c->error = FAILURE; return RVB_ERR_HIP; }
    const size_t count = (size_t) (c->nchannels * 8 * nbins);
    float * dev = static_cast<float *>(d_histogram), * host = static_cast<float *>(pinned_dst);
    std::lock_guard<std::mutex> lk(H.mu);
    if (H.blocks[d_histogram] < count * sizeof(float) || H.blocks[pinned_dst] < count * sizeof(float)) { violation(fmt("job %ld: a histogram buffer is too small", job)); return RVB_OK; }
    for (size_t k = 0; k < count; ++k)
        if (dev[k] != 0.0f) { violation(fmt("job %ld is binned into a histogram that was not zeroed", job)); break; }
    const std::map<const void *, View>::iterator v = H.views.find(pinned_dst);
    if (v != H.views.end() && v->second.job != job)
        violation(fmt("job %ld is exported over the histogram of job %ld, which is pending or inside its validity window", job, v->second.job));
    H.views[pinned_dst] = View{count * sizeof(float), job};
    for (size_t k = 0; k < count; ++k) dev[k] = host[k] = (float) (job + 1);
    ++H.jobs[job].staged;
    return RVB_OK;
}

}  // extern "C"

// ---- the driver --------------------------------------------------------------------------------------------------------------------------
namespace {

const float AIR[8] = {0, 0, 0, 0, 0, 0, 0, 0};
const float FACING[3] = {0, 0, 1}, UP[3] = {0, 1, 0};
std::vector<float> table_a, table_b;

struct Taken { const float * histogram; size_t count; long job; };

struct Scenario {
    std::vector<rvb_ctx *> ctxs;
    std::vector<uint64_t> lane_sizes;             // inline: one lane of all contexts
    uint64_t pairs = 1, valid_for = 0;
    rvb_pipeline * pipe = nullptr;
    long submitted = 0, taken = 0;
    std::deque<Taken> window;
    std::vector<std::string> results;
    std::vector<bool> failed;                     // per job

    Scenario(int number, const char * name, const std::vector<uint64_t> & sizes, uint64_t pairs_per_launch, bool lanes, uint64_t group)
        : lane_sizes(sizes), pairs(pairs_per_launch)
    {
        std::printf("scenario %d %s\n", number, name);
        {
            std::lock_guard<std::mutex> lk(H.mu);
            H.jobs.clear();
            H.views.clear();
        }
        uint64_t count = 0;
        for (uint64_t s : sizes) count += s;
        for (uint64_t i = 0; i < count; ++i) {
            ctxs.push_back(new rvb_ctx());
            ctxs.back()->slot = (int) i;
        }
        slots = &ctxs;
        valid_for = count * pairs;
        int rc;
        if (lanes) {
            rvb_pipeline_options opt;
            opt.group = group;
            opt.pairs_per_launch = pairs;
            rc = rvb_pipeline_create_lanes(&pipe, ctxs.data(), count, lane_sizes.data(), lane_sizes.size(), &opt);
        } else rc = rvb_pipeline_create(&pipe, ctxs.data(), count, group);
        if (rc != RVB_OK) { violation("create failed"); std::exit(1); }
    }

    void speakers(uint64_t n, int which)
    {
        std::vector<rvb_speaker> sp((size_t) n);
        std::memset(sp.data(), 0, sp.size() * sizeof(rvb_speaker));
        if (rvb_pipeline_configure_speakers(pipe, sp.data(), n, which, 0, 1, RATE, RVB_IR_EXACT, 5, AIR) != RVB_OK) violation("configure_speakers failed");
    }
    void hrtf(const std::vector<float> & table, int which)
    {
        if (rvb_pipeline_configure_hrtf(pipe, table.data(), FACING, UP, which, 0, 1, RATE, RVB_IR_FAST, 7, AIR) != RVB_OK) violation("configure_hrtf failed");
    }

    // where the header says job i runs: unit i / P, lane unit % lanes, the lane's k-th unit on its context k % size
    int context_of(long job) const
    {
        const uint64_t unit = (uint64_t) job / pairs, lane = unit % lane_sizes.size(), k = unit / lane_sizes.size();
        uint64_t first = 0;
        for (uint64_t l = 0; l < lane; ++l) first += lane_sizes[l];
        return (int) (first + k % lane_sizes[lane]);
    }

    void submit(bool oriented = false, bool directed = false)
    {
        const float mic[3] = {(float) submitted, 1.0f, 2.0f}, src[3] = {3.0f, 4.0f, 5.0f}, facing[3] = {1.0f, 0.0f, (float) submitted}, dir[3] = {0.0f, 1.0f, 1.0f};
        const int rc = rvb_pipeline_submit_directed(pipe, mic, src, oriented ? facing : nullptr, oriented ? UP : nullptr, directed ? dir : nullptr);
        if (rc != RVB_OK) violation(fmt("submit of job %ld failed: %s", submitted, rvb_pipeline_last_error(pipe)));
        ++submitted;
        failed.push_back(false);
    }

    void release_oldest()
    {
        // every element read at the end of the window: the job's own value, and memory that is still there
        const Taken t = window.front();
        window.pop_front();
        for (size_t k = 0; k < t.count; ++k)
            if (t.histogram[k] != (float) (t.job + 1)) { violation(fmt("the histogram of job %ld changed inside its validity window", t.job)); break; }
        std::lock_guard<std::mutex> lk(H.mu);
        const std::map<const void *, View>::iterator v = H.views.find(t.histogram);
        if (v != H.views.end() && v->second.job == t.job) H.views.erase(v);
    }

    int take()
    {
        rvb_pipeline_result r;
        std::memset(&r, 0, sizeof(r));
        const uint64_t pending = rvb_pipeline_pending(pipe);
        if (window.size() == valid_for) release_oldest();     // the result taken now is the last of the oldest view's window
        const int rc = rvb_pipeline_next(pipe, &r);
        if (rc != RVB_OK) {
            results.push_back(fmt("next rc=%d pending=%llu->%llu error=%s", rc, (unsigned long long) pending, (unsigned long long) rvb_pipeline_pending(pipe),
                                  rvb_pipeline_last_error(pipe)));
            if (rvb_pipeline_pending(pipe) < pending) { failed[(size_t) taken] = true; ++taken; }     // (a failed job of a lane counts as taken)
            return rc;
        }
        if ((long) r.job != taken) violation(fmt("result of job %llu where job %ld was due", (unsigned long long) r.job, taken));
        results.push_back(fmt("result job=%llu nbins=%llu nimages=%llu nchannels=%llu", (unsigned long long) r.job, (unsigned long long) r.nbins,
                              (unsigned long long) r.nimages, (unsigned long long) r.nchannels));
        window.push_back(Taken{r.histogram, (size_t) (r.nchannels * 8 * r.nbins), (long) r.job});
        ++taken;
        return rc;
    }
    void drain(int attempts = 64)
    {
        while (rvb_pipeline_pending(pipe) != 0 && attempts-- > 0) (void) take();
        if (rvb_pipeline_pending(pipe) != 0) violation("jobs stay pending");
    }
    // a batch that a lane cannot begin before all of it is there: what its threads do then does not depend on their timing
    void batch(int n, bool oriented = false)
    {
        gate(false);
        for (int i = 0; i < n; ++i) submit(oriented);
        gate(true);
        drain();
    }

    ~Scenario()
    {
        while (!window.empty()) release_oldest();             // (valid until the pipeline is destroyed)
        {
            std::lock_guard<std::mutex> lk(H.mu);
            H.views.clear();
        }
        rvb_pipeline_destroy(pipe);
        if (!fill_log.empty()) violation("fill-stream calls that no context waited for");
        fill_log.clear();
        // a new line after the calls that end a phase, so that a line is a trace or a stage
        for (rvb_ctx * c : ctxs) {
            std::string line;
            for (const std::string & e : c->log) {
                line += (line.empty() ? "" : "; ") + e;
                if (!e.compare(0, 9, "rvb_trace") || e == "rvb_ir_time_range_begin" || !e.compare(0, 24, "rvb_ir_accumulate_export") ||
                    e == "rvb_synchronize_exports" || !e.compare(0, 25, "rvb_set_concurrent_traces")) {
                    std::printf("context %d: %s\n", c->slot, line.c_str());
                    line.clear();
                }
            }
            if (!line.empty()) std::printf("context %d: %s\n", c->slot, line.c_str());
        }
        for (const std::string & r : results) std::printf("%s\n", r.c_str());
        for (long job = 0; job < submitted; ++job) {
            if (failed[(size_t) job]) continue;
            const JobRec & r = H.jobs[job];
            if (r.traced != 1 || r.ctx != context_of(job)) violation(fmt("job %ld: traced %d time(s), last on context %d, due on context %d", job, r.traced, r.ctx, context_of(job)));
            if (r.staged < 1) violation(fmt("job %ld was never staged", job));
        }
        for (rvb_ctx * c : ctxs) delete c;
        slots = nullptr;
    }
};

}  // namespace

int main()
{
    table_a.assign((size_t) 2 * 360 * 180 * 8, 0.5f);
    table_b.assign((size_t) 2 * 360 * 180 * 8, 0.25f);
    {
        Scenario s(1, "inline_4_contexts_default_group_speakers_submitted_ahead", {4}, 1, false, 0);
        s.speakers(2, RVB_IR_ALL);
        while (s.taken < 10) {
            while (s.submitted < 10 && rvb_pipeline_pending(s.pipe) < 4) s.submit();
            s.take();
        }
    }
    {
        Scenario s(2, "inline_1_context_hrtf_facing_per_job", {1}, 1, false, 0);
        s.hrtf(table_a, RVB_IR_ALL);
        for (int i = 0; i < 3; ++i) s.submit(true);
        s.drain();
    }
    {
        Scenario s(3, "inline_3_contexts_group_3_diffuse_only_all_submitted_then_drained", {3}, 1, false, 3);
        s.speakers(3, RVB_IR_DIFFUSE);
        for (int i = 0; i < 7; ++i) s.submit();
        s.drain();
    }
    {
        Scenario s(4, "inline_4_contexts_group_2_speakers_then_hrtf_then_a_new_table", {4}, 1, false, 2);
        s.speakers(2, RVB_IR_ALL);
        for (int i = 0; i < 3; ++i) s.submit();
        s.drain();
        s.hrtf(table_a, RVB_IR_ALL);
        for (int i = 0; i < 6; ++i) s.submit(true);
        s.drain();
        s.hrtf(table_b, RVB_IR_IMAGES);
        for (int i = 0; i < 5; ++i) s.submit();
        s.drain();
    }
    {
        Scenario s(5, "inline_2_contexts_source_pattern_on_directed_off", {2}, 1, false, 0);
        s.speakers(2, RVB_IR_ALL);
        const float shape[8] = {0, 0.5f, 1, 0, 0.5f, 1, 0, 0.5f};
        s.submit();
        s.drain();                                            // before the first call: the contexts' patterns are left alone
        if (rvb_pipeline_set_source_pattern(s.pipe, shape, FACING) != RVB_OK) violation("set_source_pattern failed");
        s.submit(false, true);
        s.submit();
        s.submit(false, true);
        s.drain();
        if (rvb_pipeline_set_source_pattern(s.pipe, nullptr, nullptr) != RVB_OK) violation("set_source_pattern off failed");
        s.submit();
        s.submit();
        s.drain();
    }
    {
        Scenario s(6, "inline_2_contexts_failing_stage", {2}, 1, false, 2);
        s.ctxs[1]->fail_export = 2;
        s.speakers(2, RVB_IR_ALL);
        for (int i = 0; i < 6; ++i) s.submit();
        s.drain();
    }
    {
        Scenario s(7, "lanes_2x2_contexts_4_pairs_hrtf", {2, 2}, 4, true, 0);
        s.hrtf(table_a, RVB_IR_ALL);
        s.batch(16, true);
    }
    {
        Scenario s(8, "lanes_2x1_context_1_pair_speakers", {1, 1}, 1, true, 0);
        s.speakers(2, RVB_IR_ALL);
        s.batch(4);
        s.batch(2);
    }
    {
        Scenario s(9, "lanes_1x2_contexts_3_pairs_source_pattern_partial_unit", {2}, 3, true, 0);
        s.speakers(2, RVB_IR_IMAGES);
        const float shape[8] = {1, 1, 1, 1, 0, 0, 0, 0};
        if (rvb_pipeline_set_source_pattern(s.pipe, shape, FACING) != RVB_OK) violation("set_source_pattern failed");
        s.batch(5);                                           // the last unit has two of its three pairs: traced when next waits for it
    }
    {
        Scenario s(10, "lanes_2x1_context_failing_lane_beside_a_working_one", {1, 1}, 1, true, 0);
        s.ctxs[1]->fail_export = 1;
        s.speakers(2, RVB_IR_ALL);
        s.batch(4);
        s.batch(2);                                           // a failed lane stays failed
    }
    if (H.violations) { std::fprintf(stderr, "%d violation(s)\n", H.violations); return 1; }
    return 0;
}
