// window.hip — the echo finder of include/rvb_capi_window.h (rvb_window_select, rvb_window_paths): arguments, scratch, launches and
// timings.  The kernels are csrc/window_kernels.hip, the select's arithmetic csrc/window_select.h.  rvb_window_select works on the
// caller's device array and uses of the context its device, stream, timings and ctx->window_scratch only; rvb_window_paths reads, beside
// those, the selected pair's records and the kept listener records.  Neither changes any state of the context.
#include "ctx.h"
#include "window_select.h"

namespace {

// what both calls refuse before any device is touched; 0 on success
int check_window(rvb_ctx * ctx, const char * call, float t_begin, float t_end, const float * weights, uint64_t max_entries, const char * entries_name)
{
    const std::string who(call);
    if (max_entries == 0) return fail(ctx, RVB_ERR_INVALID, who + ": " + entries_name + " is 0");
    if (max_entries > RVB_WINDOW_MAX_PATHS) return fail(ctx, RVB_ERR_INVALID, who + ": " + entries_name + " is above " RVB_STR(RVB_WINDOW_MAX_PATHS));
    if (!std::isfinite(t_begin) || !std::isfinite(t_end)) return fail(ctx, RVB_ERR_INVALID, who + ": t_begin or t_end is not finite");
    if (weights)
        for (int b = 0; b < 8; ++b)
            if (!std::isfinite(weights[b])) return fail(ctx, RVB_ERR_INVALID, who + ": weight " + std::to_string(b) + " is not finite");
    if (t_end < t_begin) return fail(ctx, RVB_ERR_INVALID, who + ": t_end < t_begin");
    return RVB_OK;
}

WindowWeights weights_of(const float * weights)
{
    WindowWeights w;
    for (int b = 0; b < 8; ++b) w.w[b] = weights ? weights[b] : 1.0f;
    return w;
}

// The selection of n >= 1 records enqueued, up to the sorted entries at `entries` (null: in the scratch, for the paths kernel).
int enqueue_select(rvb_ctx * ctx, const rvb_impulse * in, uint64_t n, float t_begin, float t_end, const float * weights, uint64_t max_entries,
                   rvb_window_entry * entries, void ** scratch_out)
{
    RVB_HIP(fail, ctx, ctx->window_scratch.ensure(rvb_window_scratch_bytes(n)));      // (the calls are synchronous: no earlier one still uses the block)
    void * scratch = ctx->window_scratch.p;
    *scratch_out = scratch;
    ctx->reset_timings();
    RVB_HIP(fail, ctx, rvb_launch_window_begin(scratch, ctx->stream));
    ctx->begin_timing("window_score_kernel");
    rvb_launch_window_score(in, n, t_begin, t_end, weights_of(weights), scratch, ctx->stream);
    ctx->end_timing();
    ctx->begin_timing("window_select_keys");
    for (uint32_t pass = 0; pass < window_select::kPasses; ++pass) rvb_launch_window_pass(pass, n, max_entries, scratch, ctx->stream);
    ctx->end_timing();
    ctx->begin_timing("window_select_records");
    for (uint32_t pass = window_select::kPasses; pass < 2 * window_select::kPasses; ++pass) rvb_launch_window_pass(pass, n, max_entries, scratch, ctx->stream);
    ctx->end_timing();
    ctx->begin_timing("window_gather_kernel");
    rvb_launch_window_gather(n, scratch, ctx->stream);
    ctx->end_timing();
    ctx->begin_timing("window_sort_kernel");
    rvb_launch_window_sort(in, scratch, entries ? entries : rvb_window_scratch_entries(scratch), ctx->stream);
    ctx->end_timing();
    return RVB_OK;
}

// waits for the stream, then the two counts of the select
int fetch_counts(rvb_ctx * ctx, const void * scratch, uint64_t * count, uint64_t * in_window)
{
    RVB_HIP(fail, ctx, hipGetLastError());
    RVB_HIP(fail, ctx, hipStreamSynchronize(ctx->stream));
    window_select::State state;
    const int rc = rvb_copy_to_host(ctx, &state, rvb_window_scratch_state(scratch), sizeof(state));
    if (rc != RVB_OK) return rc;
    if (count) *count = state.want;
    if (in_window) *in_window = state.in_window;
    return RVB_OK;
}

bool overlap(const void * a, uint64_t a_bytes, const void * b, uint64_t b_bytes)
{
    const uintptr_t x = reinterpret_cast<uintptr_t>(a), y = reinterpret_cast<uintptr_t>(b);
    return x < y + b_bytes && y < x + a_bytes;
}

} // namespace

extern "C" {

int rvb_window_select(rvb_ctx * ctx, const void * d_impulses, uint64_t nimpulses, float t_begin, float t_end, const float weights[8],
                      uint64_t max_entries, void * d_entries, uint64_t * count, uint64_t * in_window)
{
    if (!ctx) return RVB_ERR_INVALID;
    if (!d_impulses && nimpulses > 0) return fail(ctx, RVB_ERR_INVALID, "rvb_window_select: null impulses with nimpulses > 0");
    if (!d_entries) return fail(ctx, RVB_ERR_INVALID, "rvb_window_select: null entries");
    int rc = check_window(ctx, "rvb_window_select", t_begin, t_end, weights, max_entries, "max_entries");
    if (rc != RVB_OK) return rc;
    if (nimpulses >= (1ull << 32)) return fail(ctx, RVB_ERR_CAPACITY, "rvb_window_select: 2^32 records or more (record numbers are 32-bit in the selection key)");
    if (nimpulses == 0) {                                            // legal: lists nothing
        ctx->reset_timings();
        if (count) *count = 0;
        if (in_window) *in_window = 0;
        return RVB_OK;
    }
    RVB_BIND(ctx);
    void * scratch = nullptr;
    rc = enqueue_select(ctx, reinterpret_cast<const rvb_impulse *>(d_impulses), nimpulses, t_begin, t_end, weights, max_entries,
                        reinterpret_cast<rvb_window_entry *>(d_entries), &scratch);
    if (rc != RVB_OK) return rc;
    return fetch_counts(ctx, scratch, count, in_window);
}

int rvb_window_paths(rvb_ctx * ctx, float t_begin, float t_end, const float weights[8], uint64_t max_paths, uint64_t max_hits, void * d_paths,
                     void * d_hits, uint64_t * count, uint64_t * in_window)
{
    if (!ctx) return RVB_ERR_INVALID;
    if (!d_paths) return fail(ctx, RVB_ERR_INVALID, "rvb_window_paths: null paths");
    int rc = check_window(ctx, "rvb_window_paths", t_begin, t_end, weights, max_paths, "max_paths");
    if (rc != RVB_OK) return rc;
    if (d_hits && max_hits == 0) return fail(ctx, RVB_ERR_INVALID, "rvb_window_paths: max_hits is 0 with hits given");
    if (d_hits && max_hits > (~0ull / sizeof(rvb_window_hit)) / max_paths) return fail(ctx, RVB_ERR_INVALID, "rvb_window_paths: max_paths * max_hits hits do not fit the address space");
    if (d_hits && overlap(d_paths, max_paths * sizeof(rvb_window_path), d_hits, max_paths * max_hits * sizeof(rvb_window_hit)))
        return fail(ctx, RVB_ERR_INVALID, "rvb_window_paths: the hits overlap the paths");
    if (!ctx->trace.traced()) return fail(ctx, RVB_ERR_STATE, "rvb_window_paths: nothing traced (or the scene or the directions have changed since)");
    if (d_hits && !ctx->kept.listener_valid())
        return fail(ctx, RVB_ERR_STATE, "rvb_window_paths: hits asked for and the last trace was made without rvb_keep_paths(ctx, RVB_KEEP_MATERIALS | RVB_KEEP_LISTENER): "
                                        "a hit's triangle is in its listener record");
    const uint64_t nreflections = ctx->trace.nreflections();
    const uint64_t n = ctx->nrays * nreflections;                     // records of the pair
    if (n >= (1ull << 32) || nreflections >= (1ull << 32))
        return fail(ctx, RVB_ERR_CAPACITY, "rvb_window_paths: nrays * nreflections reaches 2^32 (record numbers are 32-bit in the selection key)");
    if (n == 0) {
        ctx->reset_timings();
        if (count) *count = 0;
        if (in_window) *in_window = 0;
        return RVB_OK;
    }
    RVB_BIND(ctx);
    const rvb_impulse * in = ir_diffuse(ctx);
    // the listener records follow the kept launch: the pair's first is behind those of the pairs before it
    const uint2 * listen = d_hits ? ctx->kept.dev.listen.as<const uint2>() + ctx->trace.pair() * n : nullptr;
    void * scratch = nullptr;
    rc = enqueue_select(ctx, in, n, t_begin, t_end, weights, max_paths, nullptr, &scratch);
    if (rc != RVB_OK) return rc;
    ctx->begin_timing("window_paths_kernel");
    rvb_launch_window_paths(in, listen, (uint32_t) nreflections, max_paths, max_hits, scratch, reinterpret_cast<rvb_window_path *>(d_paths),
                            reinterpret_cast<rvb_window_hit *>(d_hits), ctx->stream);
    ctx->end_timing();
    return fetch_counts(ctx, scratch, count, in_window);
}

} // extern "C"
