// source.hip — source directivity of include/rvb_capi.h over SourceDirectivity (ctx.h; its host half: source_state.h): the two setters,
// the upload in front of a trace or a re-shade, and the launches behind the kernel that wrote the final records.
#include "ctx.h"

#include <cstring>

// The patterns, where they have changed since the last upload: up in stream order, through a staging block of their own ...
hipError_t SourceDirectivity::upload(hipStream_t stream)
{
    hipError_t e;
    if (patterns_need_upload()) {
        if ((e = patterns_stage.upload(patterns_dev, patterns.data(), patterns.size() * sizeof(SourcePatternDev), stream)) != hipSuccess) return e;
        patterns_dirty = false;
    }
    // ... and the table with the bases of its orientations behind it, in one block
    if (table_needs_upload()) {
        const size_t table_floats = (size_t) RVB_HRTF_ROWS * 8, bytes = (table_floats + bases.size()) * sizeof(float);
        if ((e = table_stage.acquire(bytes, stream, &table_dev)) != hipSuccess) return e;
        float * host = table_stage.host<float>();
        std::memcpy(host, table.data(), table.size() * sizeof(float));
        std::memset(host + table.size(), 0, (table_floats - table.size()) * sizeof(float));               // the zero row
        std::memcpy(host + table_floats, bases.data(), bases.size() * sizeof(float));
        if ((e = hipMemcpyAsync(table_dev.p, host, bytes, hipMemcpyHostToDevice, stream)) != hipSuccess) return e;
        if ((e = table_stage.record(stream)) != hipSuccess) return e;
        table_dirty = false;
    }
    return hipSuccess;
}

int check_source_counts(rvb_ctx * ctx, const char * who, uint64_t npairs)
{
    std::string error;
    const int rc = ctx->source.check_counts(who, npairs, error);
    return rc == RVB_OK ? rc : fail(ctx, rc, error);
}

// Directional sources behind the kernel that wrote the final records (the shadow kernel of a trace, the re-shade kernels of rvb_reshade):
// the records scaled once — this stream has waited for the image kernels, so the candidates are final too — and the diffuse time range
// taken again, over the scaled records: it replaces that kernel's.
// `source` names which directivity, the patterns of rvb_set_source_pattern or the table of rvb_set_source_table: what is on the device —
// the context's after SourceDirectivity::upload; rvb_relisten passes what the records reflect.  The table's diffuse gains are taken once per (pair, ray)
// in front of the streaming pass; gains_stand: those of the launch that shaded the records last are still there (rvb_relisten: they do
// not depend on the microphone).
int apply_source_patterns(rvb_ctx * ctx, const TraceArgs & a, const SourceShading & source, bool gains_stand)
{
    if (source.off()) return RVB_OK;
    if (source.table_orientations && !gains_stand) RVB_HIP(fail, ctx, ctx->source.gains.ensure((size_t) a.nrays * 8 * sizeof(float)));
    const int rc = reset_time_ranges(ctx, a);
    if (rc != RVB_OK) return rc;
    if (source.table_orientations) {
        const SourceTableDev d = ctx->source.table_on_device(source.table_orientations);
        if (!gains_stand) {
            ctx->begin_timing("source_table_rays_kernel");
            rvb_launch_source_table_rays(a, d, ctx->stream);
            ctx->end_timing();
        }
        ctx->begin_timing("source_table_kernel");
        rvb_launch_source_table(a, d, ctx->stream);
        ctx->end_timing();
    } else {
        ctx->begin_timing("source_pattern_kernel");
        rvb_launch_source_pattern(a, ctx->source.patterns_on_device(), (uint32_t) source.patterns.size(), ctx->stream);
        ctx->end_timing();
    }
    RVB_HIP(fail, ctx, hipGetLastError());
    return RVB_OK;
}

extern "C" {

int rvb_set_source_pattern(rvb_ctx * ctx, const rvb_source_pattern * patterns, uint64_t npatterns)
{
    if (!ctx) return RVB_ERR_INVALID;
    std::string error;
    const int rc = ctx->source.set_patterns(patterns, npatterns, error);
    return rc == RVB_OK ? rc : fail(ctx, rc, error);
}

int rvb_set_source_table(rvb_ctx * ctx, const float * table, const rvb_source_orientation * orientations, uint64_t norientations)
{
    if (!ctx) return RVB_ERR_INVALID;
    std::string error;
    const int rc = ctx->source.set_table(table, orientations, norientations, error);
    return rc == RVB_OK ? rc : fail(ctx, rc, error);
}

}  // extern "C"
