// pipeline_schedule.h — the arithmetic of a lane's schedule (csrc/pipeline_lane.hip, csrc/pipeline.hip): integers only, no HIP, no rvb_*.
// Vocabulary: a JOB is one impulse response, numbered in the lane's submission order.  A UNIT is `pairs` consecutive jobs, traced by one
// launch on one context (one job where pairs == 1).  A GROUP is `group` consecutive units whose traces go out together and whose binning
// is enqueued together (one unit where a unit has several pairs: rvb_pipeline_create_lanes refuses groups of those).
#pragma once

#include <algorithm>
#include <cstdint>

namespace sched {
struct Shape {
    uint64_t contexts = 1, group = 1, pairs = 1;
    uint64_t group_jobs() const { return group * pairs; }
};

// groups of half the contexts (two groups in flight), as measured best at workload C2 (4 contexts in groups of 2); at most what one
// launch takes; units of several pairs go out one per launch
inline uint64_t group_size(uint64_t asked, uint64_t contexts, uint64_t pairs, uint64_t most) { return pairs > 1 ? 1 : std::min(std::min(asked ? asked : std::max<uint64_t>(1, contexts / 2), contexts), most); }

inline uint64_t unit_of(const Shape & s, uint64_t job) { return job / s.pairs; }
inline uint64_t context_of(const Shape & s, uint64_t unit) { return unit % s.contexts; }      // round-robin over the lane's contexts
inline uint64_t group_first(const Shape & s, uint64_t job) { return job / s.group_jobs() * s.group_jobs(); }
inline uint64_t group_end(const Shape & s, uint64_t job) { return group_first(s, job) + s.group_jobs(); }
// the jobs of complete groups among `submitted`: an incomplete last group (unit) is traced when rvb_pipeline_next gets to it
inline uint64_t complete(const Shape & s, uint64_t submitted) { return group_first(s, submitted); }

// HAND-OVER: a unit may go out once the unit that held its context before has handed it over — returned, or at least staged (its
// binning is enqueued; the new trace follows it in stream order and touches none of its buffers).  The job to look at is that unit's
// last; the first round of units has no predecessor.
inline bool has_predecessor(const Shape & s, uint64_t unit) { return unit >= s.contexts; }
inline uint64_t predecessor_last_job(const Shape & s, uint64_t unit) { return (unit - s.contexts) * s.pairs + s.pairs - 1; }
// THE REST OF A PARTIAL UNIT: a unit whose first part went out in a launch of its own continues at `begun_upto`; the rest waits until
// that part (job begun_upto - 1) is staged — the new launch replaces the context's trace results.
inline bool continues_partial_unit(const Shape & s, uint64_t begun_upto) { return begun_upto % s.pairs != 0; }

// SUBMIT-AHEAD: how far the traces may run ahead of the results taken, as far as contexts are free — every context holds one unit.
// On submit: complete groups only (the contexts of jobs that have not been returned are taken).
inline uint64_t ahead_on_submit(const Shape & s, uint64_t returned, uint64_t submitted) { return std::min(group_first(s, returned) + s.contexts * s.pairs, complete(s, submitted)); }
// Before the front group is staged: the groups after it.
inline uint64_t ahead_before_staging(const Shape & s, uint64_t front) { return group_first(s, front) + s.contexts * s.pairs; }
// After its binning is done: its contexts take the traces of the group after next (complete groups only).
inline uint64_t ahead_after_staging(const Shape & s, uint64_t front, uint64_t submitted) { return std::min(group_end(s, front) + s.contexts * s.pairs, complete(s, submitted)); }

// ALLOW (lane threads): jobs [0, allow) may be traced.  The oldest job goes on when its group is complete, or when the caller waits
// for it or for a later job (`waited` of the lane's jobs): an incomplete last unit is traced then, not as soon as its first job arrives.
inline uint64_t allow(const Shape & s, uint64_t submitted, uint64_t returned, uint64_t waited)
{
    const uint64_t gj = s.group_jobs();
    return std::min(submitted, std::max(complete(s, submitted), (returned + waited + gj - 1) / gj * gj));
}

// CAPACITY: how many jobs may be pending, how many further results a result's histogram outlives, and the pinned buffers per lane.
struct Capacity { uint64_t limit, window, ring; };
// one lane in the caller's thread: job j uses ring slot j % ring, and job j + ring is staged only after `contexts` results beyond j
inline Capacity capacity_inline(uint64_t contexts) { return Capacity{4 * contexts, contexts, 2 * contexts}; }
// lanes: a lane's ring slot is used again ring x lanes jobs later (units go round-robin over the lanes), so
// ring x lanes >= limit + window; a whole number of units
inline Capacity capacity_lanes(uint64_t contexts, uint64_t pairs, uint64_t lanes)
{
    const uint64_t limit = 2 * contexts * pairs, window = contexts * pairs;
    return Capacity{limit, window, ((limit + window + lanes - 1) / lanes + pairs - 1) / pairs * pairs};
}
}  // namespace sched
