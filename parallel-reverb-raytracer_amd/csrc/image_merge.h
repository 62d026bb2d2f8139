// image_merge.h — the size-then-fill idiom of the image-source calls, once, for the host layers above the C-ABI (csrc/multi.hip,
// csrc/pipeline_lane.hip).  Rests on include/rvb_capi.h alone.  Both return the C-ABI's code; the caller words its own error.
#pragma once

#include "../../include/rvb_capi.h"

#include <vector>

// appends the image-source candidates of the context's last trace to `all` (several shards: one call per context, in shard order)
inline int append_image_candidates(rvb_ctx * ctx, std::vector<rvb_image_candidate> & all)
{
    uint64_t n = 0;
    int rc = rvb_get_image_candidates(ctx, nullptr, 0, &n);
    if (rc != RVB_OK) return rc;
    const size_t at = all.size();
    all.resize(at + n);
    return n ? rvb_get_image_candidates(ctx, all.data() + at, n, &n) : rc;
}

// images = rvb_merge_images of the candidates; `direct` may be null (the caller's choice: a trace without rays has no direct path)
inline int merge_images(const rvb_image_candidate * candidates, uint64_t ncandidates, const rvb_impulse * direct, int remove_direct,
                        std::vector<rvb_impulse> & images)
{
    uint64_t count = 0;
    int rc = rvb_merge_images(candidates, ncandidates, direct, remove_direct, nullptr, 0, &count);
    images.resize(rc == RVB_OK ? count : 0);
    if (rc == RVB_OK && count) rc = rvb_merge_images(candidates, ncandidates, direct, remove_direct, images.data(), count, &count);
    return rc;
}
