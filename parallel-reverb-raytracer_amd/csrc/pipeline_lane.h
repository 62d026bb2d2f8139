// pipeline_lane.h — a LANE of the impulse-response pipeline: several contexts of one GPU that take turns (csrc/pipeline_lane.hip does
// the device work, csrc/pipeline_schedule.h holds the arithmetic, csrc/pipeline.hip the entry points and the lane threads).
// A Lane is touched by ONE thread — the caller's (rvb_pipeline_create) or the lane's own (rvb_pipeline_create_lanes); what that
// thread shares with the caller lives in pipeline.hip's Mailbox, not here.
#pragma once

#include "../../include/rvb_capi.h"
#include "hip_owned.h"
#include "pipeline_schedule.h"

#include <deque>
#include <string>
#include <vector>

#pragma GCC visibility push(hidden)

template <class Owner>                        // a Lane or the pipeline: each has its own last error
int pfail(Owner * o, int code, const std::string & what) { if (o) o->error = what; return code; }

struct Job {
    uint64_t id = 0;                          // the lane's submission number
    uint64_t pair = 0, launch_pairs = 1;      // this job's pair in its launch, and that launch's pair count
    float mic[3] = {0, 0, 0}, source[3] = {0, 0, 0}, facing[3] = {0, 0, 0}, up[3] = {0, 0, 0};
    float source_direction[3] = {0, 0, 0};    // the way this job's source faces (Config::source_on)
    bool staged = false;                      // its binning and export are enqueued
    uint64_t nbins = 0, nimages = 0;
    float predelay = 0.0f, max_time = 0.0f;
    float * host = nullptr;
};

struct Slot {                                 // per context
    rvb_ctx * ctx = nullptr;
    bool has_table = false;                   // the pipeline's HRTF table is on this context's device (uploaded with its first HRTF job)
    DevBuf hist[RVB_PIPELINE_MAX_PAIRS];      // device [nchannels][8][nbins], one per pair of a unit
    Event zeroed, uploaded;                   // `uploaded`, several pairs only: behind a pair's rvb_ir_configure_* (its image upload reads the context's host copy)
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
    uint64_t nchannels() const { return hrtf ? 2 : speakers.size(); }
};

struct Lane {
    const Config * cfg = nullptr;
    std::vector<Slot> slots;                  // the lane's contexts: set before lane_init
    sched::Shape shape;
    // A launch of SEVERAL pairs differs from a launch of one in these ways, each decided by this flag where it applies:
    //   candidates   one pair: fetched per job, whatever `which` is; several: once per launch, and only with images on
    //   `uploaded`   the event exists with several pairs only (the pairs of a launch share the context's host copy of the images)
    //   the trace    rvb_trace_pairs on the unit's context; one pair: rvb_trace / rvb_trace_group (either way: one rvb_synchronize per context)
    bool several = false;
    int device = 0;
    Stream fill_stream;                       // zero fills of the histograms (the contexts' streams wait for them by an event)
    std::string error;
    std::deque<Job> jobs;                     // [returned, submitted); jobs.front() is the oldest not yet returned
    uint64_t submitted = 0, returned = 0, begun_upto = 0;
    uint64_t allow = UINT64_MAX;              // jobs [0, allow) may be traced (sched::allow; a lane in the caller's thread: all)
    std::vector<PinnedBuf> ring;              // pinned result buffers, job id % ring.size()
    std::vector<rvb_image_candidate> candidates, pair_candidates;
    std::vector<rvb_impulse> images;
    ~Lane() { (void) hipSetDevice(device); }  // (lane_drain has run: nothing uses what the members release)
};

// a lane's streams and events, its contexts' hint; the contexts are the caller's (scene and rays set, all on one device)
int lane_init(Lane * l, uint64_t group, uint64_t pairs, uint64_t ring);
int lane_submit(Lane * l, const Job & in);                // one more job; the traces of complete groups go out as soon as contexts are free
int lane_next(Lane * l, rvb_pipeline_result * out);       // the oldest job's result, its histogram in the ring; blocks until it is there
// the end of a lane's work: its contexts and its fill stream idle, the contexts' hint withdrawn (~Lane then releases buffers and events)
void lane_drain(Lane * l);

#pragma GCC visibility pop
