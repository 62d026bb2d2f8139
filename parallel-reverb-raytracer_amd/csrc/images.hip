// images.hip — include/rvb_capi_images.h: the merged image list made on the device (rvb_ir_configure_speakers_merged,
// rvb_ir_configure_hrtf_merged) and the image-source part of the material gradient (rvb_reshade_grad_images).  The merge rule is
// trace.hip's (merge_image_winners), the configuration's halves are ir.hip's, the kernels are image_grad_kernels.hip's.
#include "../../include/rvb_capi_images.h"
#include "ctx.h"

namespace {

// The winner list of the selected pair: from the cache, or made from one download of the candidates in device order and uploaded.
int ensure_winners(rvb_ctx * ctx, bool remove_direct)
{
    MergedImages & merged = ctx->merged;
    if (merged.serves(ctx->trace.pair(), remove_direct)) return RVB_OK;
    int rc = fetch_small(ctx);
    if (rc != RVB_OK) return rc;
    RVB_HIP(fail, ctx, hipStreamSynchronize(ctx->stream));        // the candidates are final, and no kernel reads the list that is about to be replaced
    const uint32_t ncand = ctx->trace.host->small.candidate_count;
    std::vector<rvb_image_candidate> all(ncand);
    if (ncand) RVB_HIP(fail, ctx, hipMemcpy(all.data(), ctx->trace.candidates.p, (size_t) ncand * sizeof(rvb_image_candidate), hipMemcpyDeviceToHost));
    // the selected pair's candidates (a candidate's ray: ray_offset + pair * nrays + the ray's number within the pair), device positions kept
    std::vector<rvb_image_candidate> mine;
    std::vector<uint32_t> position;
    for (uint32_t i = 0; i < ncand; ++i) {
        if (ctx->trace.npairs() > 1 && ctx->nrays && (all[i].ray - ctx->trace.ray_offset()) / ctx->nrays != ctx->trace.pair()) continue;
        mine.push_back(all[i]);
        position.push_back(i);
    }
    std::vector<uint32_t> winners;
    // (the direct slot takes part whenever the context has rays: what the host path passes to rvb_merge_images)
    rc = merge_image_winners(mine.data(), mine.size(), ctx->nrays != 0, remove_direct, winners);
    if (rc != RVB_OK) return fail(ctx, rc, "rvb_ir_configure_merged: a candidate's slot is out of range");
    for (uint32_t & w : winners)
        if (w != RVB_IMAGE_WINNER_DIRECT) w = position[w];
    // From here on the list on the device is no longer the one a configuration may have been made from: that configuration goes with
    // it (a failure above has left both as they were).
    merged.void_list();
    if (ctx->ir.from_merged_list()) ctx->ir.drop_configuration();
    RVB_HIP(fail, ctx, merged.winners.ensure(winners.size() * sizeof(uint32_t)));
    if (!winners.empty()) RVB_HIP(fail, ctx, hipMemcpy(merged.winners.p, winners.data(), winners.size() * sizeof(uint32_t), hipMemcpyHostToDevice));
    merged.made(ctx->trace.pair(), remove_direct, winners.size());
    return RVB_OK;
}

// behind the model: the list, the configuration's state, the gather in stream order
int configure_merged(rvb_ctx * ctx, int which, int remove_direct, uint64_t * nimages)
{
    int rc = ir_configure_refusals(ctx, which);
    if (rc != RVB_OK) return rc;
    if ((rc = ensure_winners(ctx, remove_direct != 0)) != RVB_OK) return rc;
    const uint64_t n = ctx->merged.count();
    if ((rc = ir_configure_images(ctx, which, nullptr, n, true)) != RVB_OK) return rc;
    ctx->reset_timings();
    ctx->begin_timing("image_gather_kernel");
    rvb_launch_image_gather(ctx->trace.candidates.as<rvb_image_candidate>(), ctx->trace.direct_slot(), ctx->merged.winners.as<uint32_t>(), n,
                            ctx->ir.images.as<rvb_impulse>(), ctx->stream);
    ctx->end_timing();
    RVB_HIP(fail, ctx, hipGetLastError());
    if (nimages) *nimages = n;
    return RVB_OK;
}

}  // namespace

// What rvb_reshade_grad_images refuses of the binning and of the context's state, before any device is touched, under the name of the
// call `name`: rvb_source_grad_images (source_grad.hip) has the same preconditions.
int reshade_grad_images_refusals(rvb_ctx * ctx, const char * name, float predelay, float sample_rate, uint64_t nbins)
{
    const std::string who = name;
    if (nbins == 0 || nbins >= (1ull << 32)) return fail(ctx, RVB_ERR_INVALID, who + ": no bins (or more than 32-bit bin numbers reach)");
    if (!std::isfinite(predelay) || !std::isfinite(sample_rate)) return fail(ctx, RVB_ERR_INVALID, who + ": predelay or sample rate is not finite");
    if (!ctx->trace.traced()) return fail(ctx, RVB_ERR_STATE, who + ": nothing traced (or the scene or the directions have changed since)");
    if (!ctx->kept.valid()) return fail(ctx, RVB_ERR_STATE, who + ": the last trace was made without rvb_keep_paths(ctx, 1)");
    if (!ctx->ir.configured())
        return fail(ctx, RVB_ERR_STATE, who + ": no IR configuration (rvb_ir_configure_speakers_merged after the trace, re-shade or relisten)");
    if (ctx->ir.model.hrtf) return fail(ctx, RVB_ERR_STATE, who + ": the HRTF model is configured; this version takes the speaker model only");
    if (!ctx->ir.from_merged_list() || !ctx->merged.valid())
        return fail(ctx, RVB_ERR_STATE, who + ": the caller's list has lost its chains: configure with rvb_ir_configure_speakers_merged");
    if (ctx->ir.which() == RVB_IR_DIFFUSE)
        return fail(ctx, RVB_ERR_STATE, who + ": configured with which == RVB_IR_DIFFUSE: no image takes part (rvb_reshade_grad has that gradient)");
    if (ctx->ir.model.nchannels > 8)
        return fail(ctx, RVB_ERR_STATE, who + ": " + std::to_string(ctx->ir.model.nchannels) + " speaker channels configured; this version takes 1 to 8");
    if (ctx->scene.nsurfaces >= (1ull << 27)) return fail(ctx, RVB_ERR_CAPACITY, who + ": too many surfaces");
    return RVB_OK;
}

// what an image gradient kernel takes beside `a` (the kept trace's arguments under what the records reflect now): the merged list, the
// binning, the weights in place, and the source directivity that the records reflect, for the selected pair
ImageGradArgs image_grad_args(const rvb_ctx * ctx, const TraceArgs & a, float predelay, float sample_rate, uint64_t nbins, const void * d_weights)
{
    const KeptTrace & kept = ctx->kept;
    ImageGradArgs g = {};
    g.winners = ctx->merged.winners.as<const uint32_t>();
    g.images = ctx->ir.images.as<const rvb_impulse>();
    g.n = ctx->ir.nimages();
    g.direct_dist = a.nrays * (RVB_NUM_IMAGE_SOURCE - 1) + ctx->trace.pair();
    g.weights = reinterpret_cast<const float *>(d_weights);
    g.nbins = nbins;
    g.predelay = predelay;
    g.sample_rate = sample_rate;
    for (int i = 0; i < 3; ++i) g.mic[i] = ctx->trace.mic()[i];
    const SourceShading & shaded = kept.shaded_source();
    g.has_pattern = kept.shaded_pattern(ctx->trace.pair(), g.pattern);
    if (shaded.table_orientations) {
        const SourceTableDev t = ctx->source.table_on_device(shaded.table_orientations);
        g.table = t.table;
        g.table_basis = t.bases + ctx->trace.pair() * t.basis_stride;
    }
    return g;
}

extern "C" {

int rvb_ir_configure_speakers_merged(rvb_ctx * ctx, const float mic[3], const rvb_speaker * speakers, uint64_t nspeakers,
                                     int which, int remove_direct, uint64_t * nimages)
{
    if (!ctx) return RVB_ERR_INVALID;
    const int rc = ir_speaker_model(ctx, mic, speakers, nspeakers);
    return rc == RVB_OK ? configure_merged(ctx, which, remove_direct, nimages) : rc;
}

int rvb_ir_configure_hrtf_merged(rvb_ctx * ctx, const float mic[3], const float * table, const float facing[3], const float up[3],
                                 int which, int remove_direct, uint64_t * nimages)
{
    if (!ctx) return RVB_ERR_INVALID;
    const int rc = ir_hrtf_model(ctx, mic, table, facing, up);
    return rc == RVB_OK ? configure_merged(ctx, which, remove_direct, nimages) : rc;
}

int rvb_reshade_grad_images(rvb_ctx * ctx, float predelay, float sample_rate, uint64_t nbins, const void * d_weights, rvb_surface * grad_surfaces,
                            float grad_air[8])
{
    if (!ctx) return RVB_ERR_INVALID;
    if (!d_weights || !grad_surfaces) return fail(ctx, RVB_ERR_INVALID, "rvb_reshade_grad_images: null weights or null output");
    const int refused = reshade_grad_images_refusals(ctx, "rvb_reshade_grad_images", predelay, sample_rate, nbins);
    if (refused != RVB_OK) return refused;
    RVB_BIND(ctx);
    KeptTrace & kept = ctx->kept;
    MergedImages & merged = ctx->merged;
    TraceArgs a = kept.shaded_args();
    a.scene.stamps = nullptr;
    const uint64_t n = ctx->ir.nimages(), entries = ctx->scene.nsurfaces * 16 + 8;
    // the term rows, then the result
    const size_t row_bytes = (size_t) n * RVB_IMAGE_GRAD_ROW * sizeof(uint32_t);
    RVB_HIP(fail, ctx, merged.grad_scratch.ensure(row_bytes + entries * sizeof(float)));
    uint32_t * rows = merged.grad_scratch.as<uint32_t>();
    float * d_out = reinterpret_cast<float *>(merged.grad_scratch.as<char>() + row_bytes);
    const ImageGradArgs g = image_grad_args(ctx, a, predelay, sample_rate, nbins, d_weights);
    ctx->reset_timings();
    ctx->begin_timing("reshade_grad_images_kernel");
    rvb_launch_reshade_grad_images(a, ctx->ir.model, g, rows, ctx->stream);
    ctx->end_timing();
    ctx->begin_timing("reshade_grad_images_reduce_kernel");
    rvb_launch_reshade_grad_images_reduce(rows, n, ctx->scene.nsurfaces, d_out, ctx->stream);
    ctx->end_timing();
    RVB_HIP(fail, ctx, hipGetLastError());
    return download_surface_gradient(ctx, d_out, grad_surfaces, grad_air);
}

}  // extern "C"
