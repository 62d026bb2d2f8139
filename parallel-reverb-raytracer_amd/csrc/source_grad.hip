// source_grad.hip — include/rvb_capi_source_grad.h: the source-end gradients of a weighted impulse response from a kept trace,
// rvb_source_grad (the diffuse records, beside rvb_reshade_grad of kept.hip) and rvb_source_grad_images (the merged image list, beside
// rvb_reshade_grad_images of images.hip).  Both take those calls' refusals and kernel arguments from the functions those calls use; the
// kernels are source_grad_kernels.hip's.
#include "../../include/rvb_capi_source_grad.h"
#include "ctx.h"

#include <cstring>

namespace {

// [p, p + bytes) of a device output and the weights have a byte in common
bool overlaps(const void * p, uint64_t bytes, const void * d_weights, uint64_t weight_bytes)
{
    if (!p || !bytes) return false;
    const uintptr_t p0 = (uintptr_t) p, p1 = p0 + bytes, w0 = (uintptr_t) d_weights, w1 = w0 + weight_bytes;
    return p0 < w1 && w0 < p1;
}

// What both calls refuse of their outputs, behind the mirrored call's refusals and before any device is touched: an output that overlaps
// the weights (outputs: address and bytes, in the order of the arguments), a pattern gradient without a pattern, rows without a table.
struct DeviceOutput { const char * name; const void * p; uint64_t bytes; };
int output_refusals(rvb_ctx * ctx, const std::string & who, const void * d_weights, uint64_t nbins, std::initializer_list<DeviceOutput> outputs, const void * d_rows,
                    const rvb_source_pattern_grad * pattern_grad)
{
    const uint64_t weight_bytes = nbins * ctx->ir.model.nchannels * 8 * sizeof(float);
    for (const DeviceOutput & o : outputs)
        if (overlaps(o.p, o.bytes, d_weights, weight_bytes)) return fail(ctx, RVB_ERR_INVALID, who + ": " + o.name + " overlaps the weights");
    const SourceShading & shaded = ctx->kept.shaded_source();
    if (d_rows && !shaded.table_orientations)
        return fail(ctx, RVB_ERR_STATE, who + ": rows asked for, but the records reflect no source table (rvb_set_source_table before the trace or re-shade)");
    if (pattern_grad && shaded.patterns.empty())
        return fail(ctx, RVB_ERR_STATE, who + ": pattern_grad asked for, but the records reflect no polar pattern (rvb_set_source_pattern before the trace or re-shade)");
    return RVB_OK;
}

// the source scratch of n items: [n][8] binary64 sums, [n] departure vectors, the pattern partials, the result
struct SourceScratch {
    double * lambda;
    float4 * departures;
    double * partials;
    float * out;
    static size_t bytes(uint64_t n) { return (size_t) n * (8 * sizeof(double) + sizeof(float4)) + (size_t) rvb_source_grad_tiles(n) * 11 * sizeof(double) + 16 * sizeof(float); }
    static SourceScratch in(DevBuf & block, uint64_t n)
    {
        SourceScratch s;
        char * p = block.as<char>();
        s.lambda = reinterpret_cast<double *>(p);
        s.departures = reinterpret_cast<float4 *>(p + (size_t) n * 8 * sizeof(double));
        s.partials = reinterpret_cast<double *>(p + (size_t) n * (8 * sizeof(double) + sizeof(float4)));
        s.out = reinterpret_cast<float *>(s.partials + (size_t) rvb_source_grad_tiles(n) * 11);
        return s;
    }
};

// the pattern pair behind a gradient kernel, then the wait that makes the call synchronous and the twelve floats of the result
int finish(rvb_ctx * ctx, const float4 * vectors, uint64_t n, const SourceScratch & scratch, rvb_source_pattern_grad * pattern_grad)
{
    if (pattern_grad) {
        SourcePatternDev pattern;
        ctx->kept.shaded_pattern(ctx->trace.pair(), pattern);
        ctx->begin_timing("source_grad_pattern_kernel");
        rvb_launch_source_grad_pattern(vectors, scratch.lambda, n, pattern, scratch.partials, ctx->stream);
        ctx->end_timing();
        ctx->begin_timing("source_grad_pattern_fold_kernel");
        rvb_launch_source_grad_pattern_fold(scratch.partials, n, scratch.out, ctx->stream);
        ctx->end_timing();
    }
    RVB_HIP(fail, ctx, hipGetLastError());
    RVB_HIP(fail, ctx, hipStreamSynchronize(ctx->stream));
    if (pattern_grad) {
        float host[12];
        const int rc = rvb_copy_to_host(ctx, host, scratch.out, sizeof(host));
        if (rc != RVB_OK) return rc;
        static_assert(sizeof(rvb_source_pattern_grad) == sizeof(host), "shape[8], then direction[4]");
        std::memcpy(pattern_grad, host, sizeof(host));
    }
    return RVB_OK;
}

}  // namespace

extern "C" {

int rvb_source_grad(rvb_ctx * ctx, float predelay, float sample_rate, uint64_t nbins, const void * d_weights, void * d_ray_grad, void * d_ray_rows,
                    rvb_source_pattern_grad * pattern_grad)
{
    if (!ctx) return RVB_ERR_INVALID;
    if (!d_weights) return fail(ctx, RVB_ERR_INVALID, "rvb_source_grad: null weights");
    int rc = reshade_grad_refusals(ctx, "rvb_source_grad", predelay, sample_rate, nbins);
    if (rc != RVB_OK) return rc;
    const uint64_t nrays = ctx->nrays;
    rc = output_refusals(ctx, "rvb_source_grad", d_weights, nbins,
                         {{"d_ray_grad", d_ray_grad, nrays * 8 * sizeof(float)}, {"d_ray_rows", d_ray_rows, nrays * sizeof(uint32_t)}}, d_ray_rows, pattern_grad);
    if (rc != RVB_OK) return rc;
    RVB_BIND(ctx);
    KeptTrace & kept = ctx->kept;
    const TraceArgs a = for_record_pass(ctx, kept.shaded_args());
    const uint32_t nchannels = ctx->ir.model.nchannels;
    // the weights in the accumulation image's layout go where that image goes, as for rvb_reshade_grad
    RVB_HIP(fail, ctx, ctx->ir.acc.ensure((size_t) nbins * nchannels * 8 * sizeof(float)));
    SourceScratch scratch = {};
    if (pattern_grad) {
        RVB_HIP(fail, ctx, kept.dev.source_scratch.ensure(SourceScratch::bytes(nrays)));
        scratch = SourceScratch::in(kept.dev.source_scratch, nrays);
    }
    const ReshadeGradArgs g = grad_args(ctx, predelay, sample_rate, nbins);
    SourceGradOut o = {};
    o.grad = reinterpret_cast<float *>(d_ray_grad);
    o.lambda = scratch.lambda;
    if (d_ray_rows) {
        const SourceTableDev t = ctx->source.table_on_device(kept.shaded_source().table_orientations);
        o.rows = reinterpret_cast<uint32_t *>(d_ray_rows);
        o.table_basis = t.bases + ctx->trace.pair() * t.basis_stride;
    }
    ctx->reset_timings();
    ctx->begin_timing("reshade_grad_weights_kernel");
    rvb_launch_reshade_grad_weights(reinterpret_cast<const float *>(d_weights), ctx->ir.acc.as<float>(), nchannels, nbins, ctx->stream);
    ctx->end_timing();
    ctx->begin_timing("source_grad_rays_kernel");
    rvb_launch_source_grad_rays(a, kept.dev.paths.as<const float4>(), ctx->ir.model, g, o, ctx->stream);
    ctx->end_timing();
    // (the pattern kernel's vectors: the rays' own directions, shared by every pair)
    return finish(ctx, a.directions, nrays, scratch, pattern_grad);
}

int rvb_source_grad_images(rvb_ctx * ctx, float predelay, float sample_rate, uint64_t nbins, const void * d_weights, void * d_image_grad, void * d_image_depart,
                           void * d_image_rows, rvb_source_pattern_grad * pattern_grad)
{
    if (!ctx) return RVB_ERR_INVALID;
    if (!d_weights) return fail(ctx, RVB_ERR_INVALID, "rvb_source_grad_images: null weights");
    int rc = reshade_grad_images_refusals(ctx, "rvb_source_grad_images", predelay, sample_rate, nbins);
    if (rc != RVB_OK) return rc;
    const uint64_t n = ctx->ir.nimages();
    rc = output_refusals(ctx, "rvb_source_grad_images", d_weights, nbins,
                         {{"d_image_grad", d_image_grad, n * 8 * sizeof(float)}, {"d_image_depart", d_image_depart, n * 4 * sizeof(float)},
                          {"d_image_rows", d_image_rows, n * sizeof(uint32_t)}}, d_image_rows, pattern_grad);
    if (rc != RVB_OK) return rc;
    RVB_BIND(ctx);
    KeptTrace & kept = ctx->kept;
    TraceArgs a = kept.shaded_args();
    a.scene.stamps = nullptr;
    // (the departure vectors always go to the scratch: the kernel writes one per image)
    RVB_HIP(fail, ctx, kept.dev.source_scratch.ensure(SourceScratch::bytes(n)));
    const SourceScratch scratch = SourceScratch::in(kept.dev.source_scratch, n);
    const ImageGradArgs g = image_grad_args(ctx, a, predelay, sample_rate, nbins, d_weights);
    SourceGradOut o = {};
    o.grad = reinterpret_cast<float *>(d_image_grad);
    o.lambda = pattern_grad ? scratch.lambda : nullptr;
    if (d_image_rows) {
        o.rows = reinterpret_cast<uint32_t *>(d_image_rows);
        o.table_basis = g.table_basis;
    }
    ctx->reset_timings();
    ctx->begin_timing("source_grad_images_kernel");
    rvb_launch_source_grad_images(a, ctx->ir.model, g, o, scratch.departures, reinterpret_cast<float4 *>(d_image_depart), ctx->stream);
    ctx->end_timing();
    return finish(ctx, scratch.departures, n, scratch, pattern_grad);
}

}  // extern "C"
