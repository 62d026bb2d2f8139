// kept.hip — behind a kept trace (rvb_keep_paths, KeptTrace in ctx.h): re-shading (rvb_reshade), its material gradients per surface
// (rvb_reshade_grad) and per triangle (rvb_reshade_grad_map), and a new microphone (rvb_relisten), which replays the trace's tail with
// the steps trace.hip shares.
#include "ctx.h"

#include <cstdlib>
#include <cstring>

// `a` for a pass over the kept records (reshade_kernels.hip, reshade_grad_kernels.hip, relisten_kernels.hip): no stamps, and the share
// of the surface table that those kernels stage in LDS
TraceArgs for_record_pass(const rvb_ctx * ctx, TraceArgs a)
{
    a.scene.stamps = nullptr;
    a.lds_surfaces = rvb_reshade_lds_surfaces(ctx->scene.nsurfaces);
    return a;
}

// what a gradient pass takes beside `a`: the selected pair's rays and microphone, the binning, the weights where the accumulation image
// goes (rvb_launch_reshade_grad_weights puts them there), and the source directivity that the records reflect now
ReshadeGradArgs grad_args(const rvb_ctx * ctx, float predelay, float sample_rate, uint64_t nbins)
{
    const KeptTrace & kept = ctx->kept;
    ReshadeGradArgs g;
    g.weights = ctx->ir.acc.as<float>();
    g.nbins = nbins;
    g.predelay = predelay;
    g.sample_rate = sample_rate;
    g.first_ray = ctx->trace.pair() * ctx->nrays;
    g.nrays = (uint32_t) ctx->nrays;
    for (int i = 0; i < 3; ++i) g.mic[i] = ctx->trace.mic()[i];
    g.has_pattern = kept.shaded_pattern(ctx->trace.pair(), g.pattern);
    // a table shaded the records: the pair's rows of the gains that launch left (source_table_rays_kernel)
    g.ray_gains = kept.shaded_source().table_orientations ? ctx->source.gains_of_pair(ctx->trace.pair(), ctx->nrays) : nullptr;
    g.nsurfaces = ctx->scene.nsurfaces;
    return g;
}

// What rvb_reshade_grad refuses of the binning and of the context's state, before any device is touched, under the name of the call
// `name`: rvb_source_grad (source_grad.hip) has the same preconditions.
int reshade_grad_refusals(rvb_ctx * ctx, const char * name, float predelay, float sample_rate, uint64_t nbins)
{
    const std::string who = name;
    if (nbins == 0 || nbins >= (1ull << 32)) return fail(ctx, RVB_ERR_INVALID, who + ": no bins (or more than 32-bit bin numbers reach)");
    if (!std::isfinite(predelay) || !std::isfinite(sample_rate)) return fail(ctx, RVB_ERR_INVALID, who + ": predelay or sample rate is not finite");
    if (!ctx->trace.traced()) return fail(ctx, RVB_ERR_STATE, who + ": nothing traced (or the scene or the directions have changed since)");
    if (!ctx->kept.valid()) return fail(ctx, RVB_ERR_STATE, who + ": the last trace was made without rvb_keep_paths(ctx, 1)");
    if (!ctx->ir.configured()) return fail(ctx, RVB_ERR_STATE, who + ": no IR configuration (rvb_ir_configure_speakers after the trace or re-shade)");
    if (ctx->ir.model.hrtf) return fail(ctx, RVB_ERR_STATE, who + ": the HRTF model is configured; this version takes the speaker model only");
    if (ctx->ir.which() != RVB_IR_DIFFUSE) return fail(ctx, RVB_ERR_STATE, who + ": configured with image sources; this version takes which == RVB_IR_DIFFUSE only");
    if (ctx->ir.model.nchannels > 8)
        return fail(ctx, RVB_ERR_STATE, who + ": " + std::to_string(ctx->ir.model.nchannels) + " speaker channels configured; this version takes 1 to 8");
    if (ctx->trace.nreflections() > RVB_RESHADE_GRAD_MAX_REFLECTIONS)
        return fail(ctx, RVB_ERR_CAPACITY, who + ": more than " RVB_STR(RVB_RESHADE_GRAD_MAX_REFLECTIONS) " reflections");
    if (ctx->scene.nsurfaces >= (1ull << 27)) return fail(ctx, RVB_ERR_CAPACITY, who + ": too many surfaces");
    return RVB_OK;
}

int download_surface_gradient(rvb_ctx * ctx, const float * d_out, rvb_surface * grad_surfaces, float grad_air[8])
{
    const uint64_t nsurfaces = ctx->scene.nsurfaces, entries = nsurfaces * 16 + 8;
    RVB_HIP(fail, ctx, hipStreamSynchronize(ctx->stream));
    std::vector<float> host(entries);
    const int rc = rvb_copy_to_host(ctx, host.data(), d_out, entries * sizeof(float));
    if (rc != RVB_OK) return rc;
    std::memcpy(grad_surfaces, host.data(), (size_t) nsurfaces * sizeof(rvb_surface));
    if (grad_air) std::memcpy(grad_air, host.data() + nsurfaces * 16, 8 * sizeof(float));
    return RVB_OK;
}

extern "C" {

int rvb_keep_paths(rvb_ctx * ctx, int keep)
{
    if (!ctx) return RVB_ERR_INVALID;
    KeptTrace & kept = ctx->kept;
    if (kept.ask(keep) && kept.dev.any()) {       // (asked to keep: the buffers come with the next trace, sized for it)
        RVB_BIND(ctx);
        RVB_HIP(fail, ctx, hipStreamSynchronize(ctx->stream));        // a keep pass or a re-shade may still use them
        RVB_HIP(fail, ctx, hipStreamSynchronize(ctx->side_stream));
        kept.release();
    }
    return RVB_OK;
}

int rvb_relisten(rvb_ctx * ctx, const float * mics, uint64_t npairs)
{
    if (!ctx) return RVB_ERR_INVALID;
    if (!mics) return fail(ctx, RVB_ERR_INVALID, "rvb_relisten: null microphones");
    for (uint64_t i = 0; i < 3 * npairs; ++i)
        if (!std::isfinite(mics[i])) return fail(ctx, RVB_ERR_INVALID, "rvb_relisten: microphone " + std::to_string(i / 3) + " holds a coordinate that is not finite");
    if (!ctx->trace.traced()) return fail(ctx, RVB_ERR_STATE, "rvb_relisten: nothing traced (or the scene or the directions have changed since)");
    if (!ctx->kept.listener_valid())
        return fail(ctx, RVB_ERR_STATE, "rvb_relisten: the last trace was made without rvb_keep_paths(ctx, RVB_KEEP_MATERIALS | RVB_KEEP_LISTENER)");
    if (npairs != ctx->trace.npairs())
        return fail(ctx, RVB_ERR_INVALID, "rvb_relisten: " + std::to_string(npairs) + " microphone(s) for a kept trace of " + std::to_string(ctx->trace.npairs()) + " pair(s)");
    RVB_BIND(ctx);
    KeptTrace & kept = ctx->kept;
    // the table, the air and the source directivity are those the records reflect now (the scene's own after the kept trace, those of the
    // last rvb_reshade after one: the patterns or the source table on the device are these, one set since is not uploaded yet; the
    // source table's per-ray gains do not depend on the microphone and stand)
    TraceArgs a = kept.shaded_args();
    for (int i = 0; i < 3; ++i) a.mic[i] = mics[i];
    // measurements only (tools/relisten_bench.py): the shadow kernel walks the records in natural order instead of the trace's grouping
    static const bool natural_order = getenv("RVB_RELISTEN_ORDER") && getenv("RVB_RELISTEN_ORDER")[0] == '0';
    if (natural_order) a.sort_order = nullptr;
    SmallBlock * small = ctx->trace.small_dev();
    ctx->reset_timings();
    ctx->void_fetched_results();                  // (a trace alone vouches for a live count: after a replay exact mode lists every impulse)
    ctx->merged.void_list();                      // (the image kernels find other candidates: which of them win is decided anew)
    // what the tail appends to or folds into, back where a trace starts; `executed` stays
    RVB_HIP(fail, ctx, hipMemsetAsync(&small->candidate_count, 0, sizeof(uint32_t), ctx->stream));
    RVB_HIP(fail, ctx, hipMemsetAsync(&small->live_count, 0, sizeof(SmallBlock) - offsetof(SmallBlock, live_count), ctx->stream));      // ... and the direct slot
    if (npairs > 1) RVB_HIP(fail, ctx, ctx->trace.pairs.restage_mics(mics, npairs, ctx->stream));       // (reset_time_ranges, next, records the block's event)
    int rc = reset_time_ranges(ctx, a);
    if (rc != RVB_OK) return rc;
    ctx->begin_timing("relisten_records_kernel");
    rvb_launch_relisten_records(for_record_pass(ctx, a), kept.dev.paths.as<const float4>(), kept.dev.listen.as<const uint2>(), ctx->stream);
    ctx->end_timing();
    RVB_HIP(fail, ctx, hipGetLastError());
    if ((rc = launch_images_beside(ctx, a)) != RVB_OK) return rc;
    if ((rc = launch_shadow_behind_images(ctx, a, kept.shaded_source(), true)) != RVB_OK) return rc;
    // the kept trace is now that of the new microphone(s): later rvb_reshade, rvb_reshade_grad and rvb_relisten start from here
    kept.relistened(mics);
    ctx->trace.pairs.mics_host.assign(mics, mics + 3 * npairs);
    return RVB_OK;
}

int rvb_reshade(rvb_ctx * ctx, const rvb_surface * surfaces, uint64_t nsurfaces, const float air_coefficient[8])
{
    if (!ctx) return RVB_ERR_INVALID;
    if (!air_coefficient) return fail(ctx, RVB_ERR_INVALID, "rvb_reshade: null air coefficient");
    if (!ctx->trace.traced()) return fail(ctx, RVB_ERR_STATE, "rvb_reshade: nothing traced (or the scene or the directions have changed since)");
    if (!ctx->kept.valid()) return fail(ctx, RVB_ERR_STATE, "rvb_reshade: the last trace was made without rvb_keep_paths(ctx, 1)");
    if (surfaces && nsurfaces != ctx->scene.nsurfaces)
        return fail(ctx, RVB_ERR_INVALID, "rvb_reshade: " + std::to_string(nsurfaces) + " surfaces for a scene of " + std::to_string(ctx->scene.nsurfaces));
    if (check_source_counts(ctx, "rvb_reshade", ctx->trace.npairs()) != RVB_OK) return RVB_ERR_INVALID;
    RVB_BIND(ctx);
    KeptTrace & kept = ctx->kept;
    TraceArgs a = for_record_pass(ctx, kept.trace_args());   // the trace's own arguments; surfaces and air are the call's
    if (surfaces) {
        RVB_HIP(fail, ctx, kept.surfaces_stage.upload(kept.dev.surfaces, surfaces, (size_t) nsurfaces * sizeof(rvb_surface), ctx->stream));
        a.scene.surfaces = kept.dev.surfaces.as<const rvb_surface>();
    } else {
        a.scene.surfaces = ctx->scene.dev.surfaces;
    }
    for (int i = 0; i < 8; ++i) a.air[i] = air_coefficient[i];
    RVB_HIP(fail, ctx, ctx->source.upload(ctx->stream));
    ctx->reset_timings();
    int rc = reset_time_ranges(ctx, a);
    if (rc != RVB_OK) return rc;
    ctx->void_fetched_results();                  // (the re-shade kernels rewrite every volume and count nothing: no live count)
    ctx->begin_timing("reshade_kernel");
    rvb_launch_reshade(a, kept.dev.paths.as<const float4>(), ctx->stream);
    ctx->end_timing();
    ctx->begin_timing("reshade_images_kernel");
    rvb_launch_reshade_images(a, ctx->stream);
    ctx->end_timing();
    RVB_HIP(fail, ctx, hipGetLastError());
    const SourceShading source = ctx->source.shading();
    if ((rc = apply_source_patterns(ctx, a, source)) != RVB_OK) return rc;
    kept.note_shading(a, source);
    return RVB_OK;
}

int rvb_reshade_grad(rvb_ctx * ctx, float predelay, float sample_rate, uint64_t nbins, const void * d_weights, rvb_surface * grad_surfaces,
                     float grad_air[8])
{
    if (!ctx) return RVB_ERR_INVALID;
    if (!d_weights || !grad_surfaces) return fail(ctx, RVB_ERR_INVALID, "rvb_reshade_grad: null weights or null output");
    const int refused = reshade_grad_refusals(ctx, "rvb_reshade_grad", predelay, sample_rate, nbins);
    if (refused != RVB_OK) return refused;
    RVB_BIND(ctx);
    KeptTrace & kept = ctx->kept;
    const TraceArgs a = for_record_pass(ctx, kept.shaded_args());
    const uint32_t nchannels = ctx->ir.model.nchannels;
    const uint64_t entries = ctx->scene.nsurfaces * 16 + 8;
    const uint32_t blocks = rvb_reshade_grad_blocks(ctx->nrays, ctx->scene.nsurfaces);
    // the weights in the accumulation image's layout go where that image goes; the result (floats), then the partial tables (doubles)
    const size_t out_bytes = (entries * sizeof(float) + 15) & ~(size_t) 15;
    RVB_HIP(fail, ctx, ctx->ir.acc.ensure((size_t) nbins * nchannels * 8 * sizeof(float)));
    RVB_HIP(fail, ctx, kept.dev.grad_scratch.ensure(out_bytes + (size_t) blocks * entries * sizeof(double)));
    float * d_out = kept.dev.grad_scratch.as<float>();
    double * partials = reinterpret_cast<double *>(kept.dev.grad_scratch.as<char>() + out_bytes);
    const ReshadeGradArgs g = grad_args(ctx, predelay, sample_rate, nbins);
    ctx->reset_timings();
    ctx->begin_timing("reshade_grad_weights_kernel");
    rvb_launch_reshade_grad_weights(reinterpret_cast<const float *>(d_weights), ctx->ir.acc.as<float>(), nchannels, nbins, ctx->stream);
    ctx->end_timing();
    ctx->begin_timing("reshade_grad_kernel");
    rvb_launch_reshade_grad(a, kept.dev.paths.as<const float4>(), ctx->ir.model, g, partials, blocks, ctx->stream);
    ctx->end_timing();
    ctx->begin_timing("reshade_grad_reduce_kernel");
    rvb_launch_reshade_grad_reduce(partials, blocks, ctx->scene.nsurfaces, d_out, ctx->stream);
    ctx->end_timing();
    RVB_HIP(fail, ctx, hipGetLastError());
    return download_surface_gradient(ctx, d_out, grad_surfaces, grad_air);
}

int rvb_reshade_grad_map(rvb_ctx * ctx, float predelay, float sample_rate, uint64_t nbins, const void * d_weights, void * d_map, uint64_t ntriangles)
{
    if (!ctx) return RVB_ERR_INVALID;
    if (!d_weights || !d_map) return fail(ctx, RVB_ERR_INVALID, "rvb_reshade_grad_map: null weights or null map");
    if (nbins == 0 || nbins >= (1ull << 32)) return fail(ctx, RVB_ERR_INVALID, "rvb_reshade_grad_map: no bins (or more than 32-bit bin numbers reach)");
    if (!std::isfinite(predelay) || !std::isfinite(sample_rate)) return fail(ctx, RVB_ERR_INVALID, "rvb_reshade_grad_map: predelay or sample rate is not finite");
    // (without a scene there is no count to hold against: nothing is traced then, the next refusal)
    if (ctx->scene.have() && ntriangles != ctx->scene.ntriangles)
        return fail(ctx, RVB_ERR_INVALID, "rvb_reshade_grad_map: a map of " + std::to_string(ntriangles) + " triangles for a scene of " + std::to_string(ctx->scene.ntriangles));
    if (!ctx->trace.traced()) return fail(ctx, RVB_ERR_STATE, "rvb_reshade_grad_map: nothing traced (or the scene or the directions have changed since)");
    if (!ctx->kept.listener_valid())
        return fail(ctx, RVB_ERR_STATE, "rvb_reshade_grad_map: the last trace was made without rvb_keep_paths(ctx, RVB_KEEP_MATERIALS | RVB_KEEP_LISTENER): "
                                        "a record's triangle is in its listener record");
    if (!ctx->ir.configured()) return fail(ctx, RVB_ERR_STATE, "rvb_reshade_grad_map: no IR configuration (rvb_ir_configure_speakers after the trace or re-shade)");
    if (ctx->ir.model.hrtf) return fail(ctx, RVB_ERR_STATE, "rvb_reshade_grad_map: the HRTF model is configured; this version takes the speaker model only");
    if (ctx->ir.which() != RVB_IR_DIFFUSE)
        return fail(ctx, RVB_ERR_STATE, "rvb_reshade_grad_map: configured with image sources; this version takes which == RVB_IR_DIFFUSE only");
    const uint32_t nchannels = ctx->ir.model.nchannels;
    if (nchannels > 8) return fail(ctx, RVB_ERR_STATE, "rvb_reshade_grad_map: " + std::to_string(nchannels) + " speaker channels configured; this version takes 1 to 8");
    {
        const uintptr_t m0 = (uintptr_t) d_map, m1 = m0 + ntriangles * sizeof(rvb_surface);
        const uintptr_t w0 = (uintptr_t) d_weights, w1 = w0 + (uintptr_t) nbins * nchannels * 8 * sizeof(float);
        if (m0 < w1 && w0 < m1) return fail(ctx, RVB_ERR_INVALID, "rvb_reshade_grad_map: the map overlaps the weights");
    }
    if (ctx->trace.nreflections() > RVB_RESHADE_GRAD_MAX_REFLECTIONS)
        return fail(ctx, RVB_ERR_CAPACITY, "rvb_reshade_grad_map: more than " RVB_STR(RVB_RESHADE_GRAD_MAX_REFLECTIONS) " reflections");
    const uint64_t n = ctx->nrays * ctx->trace.nreflections();              // records of the pair
    if (n >= (1ull << 32))
        return fail(ctx, RVB_ERR_CAPACITY, "rvb_reshade_grad_map: nrays * nreflections reaches 2^32 (record numbers are 32-bit sort values)");
    if (ntriangles >= (1ull << 27)) return fail(ctx, RVB_ERR_CAPACITY, "rvb_reshade_grad_map: too many triangles (2^27 or more)");
    RVB_BIND(ctx);
    KeptTrace & kept = ctx->kept;
    if (n == 0) {                                                   // no record: every entry is still written
        RVB_HIP(fail, ctx, hipMemsetAsync(d_map, 0, ntriangles * sizeof(rvb_surface), ctx->stream));
        return RVB_OK;
    }
    const TraceArgs a = for_record_pass(ctx, kept.shaded_args());
    // the term rows, then the fold's partials; the (key, value) list in the sort buffers, which voids a prepared exact list and the keys
    // that a size query of rvb_flatten left
    const size_t term_bytes = (size_t) n * 16 * sizeof(float);
    RVB_HIP(fail, ctx, ctx->ir.acc.ensure((size_t) nbins * nchannels * 8 * sizeof(float)));
    RVB_HIP(fail, ctx, kept.dev.map_scratch.ensure(term_bytes + (size_t) rvb_grad_map_tiles(n) * 2 * 16 * sizeof(double)));
    int rc = ensure_sort_buffers(ctx, n);
    if (rc != RVB_OK) return rc;
    float * terms = kept.dev.map_scratch.as<float>();
    double * partials = reinterpret_cast<double *>(kept.dev.map_scratch.as<char>() + term_bytes);
    const ReshadeGradArgs g = grad_args(ctx, predelay, sample_rate, nbins);
    ctx->reset_timings();
    ctx->begin_timing("reshade_grad_weights_kernel");
    rvb_launch_reshade_grad_weights(reinterpret_cast<const float *>(d_weights), ctx->ir.acc.as<float>(), nchannels, nbins, ctx->stream);
    ctx->end_timing();
    ctx->begin_timing("reshade_grad_map_terms_kernel");
    rvb_launch_reshade_grad_map_terms(a, kept.dev.paths.as<const float4>(), kept.dev.listen.as<const uint2>(), ctx->ir.model, g, (uint32_t) ntriangles, terms,
                                      ctx->sort.keys_a.as<uint32_t>(), ctx->sort.vals_a.as<uint32_t>(), ctx->stream);
    ctx->end_timing();
    ctx->begin_timing("reshade_grad_map_sort");
    rc = sort_and_bin(ctx, n, ntriangles + 1, key_bits_for(ntriangles), true);     // (values are the entry numbers: either sort)
    ctx->end_timing();
    if (rc != RVB_OK) return rc;
    const uint32_t * starts = ctx->sort.bin_starts.as<uint32_t>();
    ctx->begin_timing("reshade_grad_map_fold_kernel");
    rvb_launch_reshade_grad_map_fold(ctx->sort.keys_b.as<uint32_t>(), ctx->sort.vals_b.as<uint32_t>(), n, (uint32_t) ntriangles, terms, partials,
                                     reinterpret_cast<float *>(d_map), ctx->stream);
    ctx->end_timing();
    ctx->begin_timing("reshade_grad_map_combine_kernel");
    rvb_launch_reshade_grad_map_combine(starts, starts + ntriangles + 1, (uint32_t) ntriangles, partials, reinterpret_cast<float *>(d_map), ctx->stream);
    ctx->end_timing();
    RVB_HIP(fail, ctx, hipGetLastError());
    return RVB_OK;
}

}  // extern "C"
