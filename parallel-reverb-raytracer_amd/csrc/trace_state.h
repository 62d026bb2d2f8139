// trace_state.h — the host half of a context's trace stage (the rvb_trace*, rvb_reshade, rvb_relisten and rvb_ir_select_pair rules of
// include/rvb_capi.h, the live count of include/rvb_capi_live.h): whether the records are a trace's, its sizes, the selected pair, and
// what of its results the host may rely on.  Plain C++: no HIP call, no kernel, so a host program can include it alone
// (tests/cpp/trace_state.cpp does).  The fields are private: the named transitions below are the only code that writes them.  The
// device half, TraceStage of ctx.h, is built on it; the entry points are in trace.hip, kept.hip and context.hip.
#pragma once

#include <cstdint>

#pragma GCC visibility push(hidden)

class TraceState {
public:
    bool traced() const { return traced_; }
    // the last trace: npairs (source, microphone) pairs x rays / npairs rays each, in one launch of rays() rays
    uint64_t npairs() const { return npairs_; }
    uint64_t rays() const { return rays_; }
    uint64_t nreflections() const { return nreflections_; }
    // ... and its ray_offset: a candidate's ray is ray_offset + pair * (rays of a pair) + the ray's number
    uint64_t ray_offset() const { return ray_offset_; }
    // the pair the IR stage and the result readers work on (rvb_ir_select_pair)
    uint64_t pair() const { return pair_; }
    // the small block and what comes with it are in their host mirrors (fetch_small)
    bool fetched() const { return fetched_; }
    // The live counts that come with the small block bound the diffuse impulses that carry volume: only a trace whose shadow stage
    // wrote the final records vouches for them; where they do not hold, the exact mode lists every record.
    bool live_count_holds() const { return live_count_holds_; }

    // The scene or the directions have changed (rvb_set_scene, rvb_share_scene, rvb_set_directions*): they no longer describe the records.
    void inputs_changed() { traced_ = false; }
    // A trace begins: until it has finished there are no results (a failure must not leave the last trace's half reset), and its
    // kernels count anew.
    void begin() { traced_ = false; live_count_holds_ = false; }
    // A trace has finished: nothing of it is fetched, its first pair is selected.  count_holds: the shadow stage's count bounds the
    // live impulses — no directivity pass behind it has rescaled the records.
    void finished(uint64_t npairs, uint64_t rays, uint64_t nreflections, uint64_t ray_offset, bool count_holds)
    {
        traced_ = true;
        npairs_ = npairs; rays_ = rays; nreflections_ = nreflections; ray_offset_ = ray_offset;
        live_count_holds_ = count_holds;
        fetched_ = false;
        pair_ = 0;
    }
    // The records are being rewritten behind a finished trace (rvb_reshade, rvb_relisten): what was fetched is not theirs, nothing
    // has counted them, and the first pair is selected as after a trace.
    void records_rewritten() { fetched_ = false; live_count_holds_ = false; pair_ = 0; }
    // rvb_ir_select_pair (the caller has held `pair` against npairs())
    void select_pair(uint64_t pair) { pair_ = pair; }
    void small_fetched() { fetched_ = true; }

private:
    bool traced_ = false, fetched_ = false, live_count_holds_ = false;
    uint64_t npairs_ = 1, rays_ = 0, nreflections_ = 0, ray_offset_ = 0, pair_ = 0;
};

#pragma GCC visibility pop
