// flatten.hip — the materialised steps of the reference on caller-held arrays: attenuate per channel, fix the predelay, flatten.  They
// share nothing with the fused stage of ir.hip but the HRTF table image and the sort buffers.
#include "ctx.h"

#include <cstring>

namespace {

AttenuationModel one_speaker_model(const float mic[3], const rvb_speaker & speaker)
{
    AttenuationModel m;
    m.hrtf = 0;
    m.nchannels = 1;
    for (int i = 0; i < 3; ++i) m.mic[i] = mic[i];
    m.speakers[0] = speaker;
    return m;
}

// the attenuate calls of the HRTF model take ONE ear's table: parked in the ear's slot of the device image
int set_one_ear_table(rvb_ctx * ctx, const float * table, uint64_t channel)
{
    RVB_HIP(fail, ctx, hipStreamSynchronize(ctx->stream));           // the table image is about to be replaced
    const int rc = upload_hrtf_table(ctx, table, (int) channel, 1);
    if (rc != RVB_OK) return rc;
    ctx->ir.one_ear_table();                  // (a prepared list of the HRTF model folds with the table image that has just been replaced)
    return RVB_OK;
}

int attenuate_device(rvb_ctx * ctx, const AttenuationModel & m, uint32_t channel, const void * d_in, uint64_t n, void * d_out)
{
    ctx->reset_timings();
    ctx->begin_timing("attenuate_kernel");
    rvb_launch_attenuate(m, channel, reinterpret_cast<const rvb_impulse *>(d_in), n, reinterpret_cast<rvb_attenuated_impulse *>(d_out), ctx->stream);
    ctx->end_timing();
    RVB_HIP(fail, ctx, hipGetLastError());
    return RVB_OK;
}

// the host forms: stage in, the device form, stage out
int attenuate_host(rvb_ctx * ctx, const AttenuationModel & m, uint32_t channel, const rvb_impulse * in, uint64_t n,
                   rvb_attenuated_impulse * out)
{
    if (n == 0) return RVB_OK;
    if (!in || !out) return fail(ctx, RVB_ERR_INVALID, "attenuate: null buffer");
    IrStage & ir = ctx->ir;
    RVB_HIP(fail, ctx, ir.scratch_in.ensure(n * sizeof(rvb_impulse)));
    RVB_HIP(fail, ctx, ir.scratch_out.ensure(n * sizeof(rvb_attenuated_impulse)));
    int rc = rvb_copy_to_device(ctx, ir.scratch_in.p, in, n * sizeof(rvb_impulse));
    if (rc == RVB_OK) rc = attenuate_device(ctx, m, channel, ir.scratch_in.p, n, ir.scratch_out.p);
    if (rc != RVB_OK) return rc;
    return rvb_copy_to_host(ctx, out, ir.scratch_out.p, n * sizeof(rvb_attenuated_impulse));
}

// keys + max time of a device-resident AttenuatedImpulse array -> *bins, in the sort buffers the caller has claimed
int flatten_keys(rvb_ctx * ctx, const rvb_attenuated_impulse * d_in, uint64_t n, float sample_rate, uint64_t * bins)
{
    uint32_t * max_bits = &ctx->trace.small_dev()->max_time_bits;
    RVB_HIP(fail, ctx, hipMemsetAsync(max_bits, 0, 4, ctx->stream));
    rvb_launch_flat_keys(d_in, n, sample_rate, ctx->sort.keys_a.as<uint32_t>(), ctx->sort.vals_a.as<uint32_t>(), max_bits, ctx->stream);
    uint32_t bits = 0;
    RVB_HIP(fail, ctx, hipMemcpyAsync(&bits, max_bits, 4, hipMemcpyDeviceToHost, ctx->stream));
    RVB_HIP(fail, ctx, hipStreamSynchronize(ctx->stream));
    float max_time;
    std::memcpy(&max_time, &bits, 4);
    *bins = bins_for(max_time, 0.0f, sample_rate);
    return RVB_OK;
}

// the shared tail of rvb_flatten / rvb_flatten_device: the size answer, or (out != NULL) sort, ordered sum, download
int flatten_finish(rvb_ctx * ctx, const rvb_attenuated_impulse * d_in, uint64_t n, uint64_t bins, float * out, uint64_t capacity_bins,
                   uint64_t * nbins, const char * too_small)
{
    *nbins = bins;
    if (!out)
        return RVB_OK;
    if (capacity_bins < bins)
        return fail(ctx, RVB_ERR_CAPACITY, too_small);
    DevBuf & hist = ctx->ir.hist;
    RVB_HIP(fail, ctx, hist.ensure(bins * 8 * sizeof(float)));
    const int rc = sort_and_bin(ctx, n, bins, key_bits_for(bins), true);
    if (rc != RVB_OK) return rc;
    rvb_launch_flat_ordered_sum(d_in, ctx->sort.keys_b.as<uint32_t>(), ctx->sort.vals_b.as<uint32_t>(), ctx->sort.bin_starts.as<uint32_t>(), n, bins,
                                hist.as<float>(), ctx->stream);
    RVB_HIP(fail, ctx, hipGetLastError());
    RVB_HIP(fail, ctx, hipMemcpyAsync(out, hist.p, bins * 8 * sizeof(float), hipMemcpyDeviceToHost, ctx->stream));
    RVB_HIP(fail, ctx, hipStreamSynchronize(ctx->stream));
    return RVB_OK;
}

}  // namespace

extern "C" {

int rvb_attenuate_speaker(rvb_ctx * ctx, const float mic[3], const rvb_impulse * in, uint64_t n,
                          const rvb_speaker * speaker, rvb_attenuated_impulse * out)
{
    if (!ctx) return RVB_ERR_INVALID;
    if (!mic || !speaker) return fail(ctx, RVB_ERR_INVALID, "rvb_attenuate_speaker: null argument");
    RVB_BIND(ctx);
    return attenuate_host(ctx, one_speaker_model(mic, *speaker), 0, in, n, out);
}

int rvb_attenuate_speaker_device(rvb_ctx * ctx, const float mic[3], const void * d_in, uint64_t n,
                                 const rvb_speaker * speaker, void * d_out)
{
    if (!ctx) return RVB_ERR_INVALID;
    if (!mic || !speaker) return fail(ctx, RVB_ERR_INVALID, "rvb_attenuate_speaker_device: null argument");
    if (n && (!d_in || !d_out)) return fail(ctx, RVB_ERR_INVALID, "rvb_attenuate_speaker_device: null buffer");
    if (n && d_in == d_out) return fail(ctx, RVB_ERR_INVALID, "rvb_attenuate_speaker_device: in-place is not supported");
    RVB_BIND(ctx);
    return attenuate_device(ctx, one_speaker_model(mic, *speaker), 0, d_in, n, d_out);
}

int rvb_attenuate_hrtf(rvb_ctx * ctx, const float mic[3], const rvb_impulse * in, uint64_t n,
                       const float * table, const float facing[3], const float up[3], uint64_t channel,
                       rvb_attenuated_impulse * out)
{
    if (!ctx) return RVB_ERR_INVALID;
    if (!mic || !table || !facing || !up || channel > 1) return fail(ctx, RVB_ERR_INVALID, "rvb_attenuate_hrtf: bad argument");
    RVB_BIND(ctx);
    const int rc = set_one_ear_table(ctx, table, channel);
    if (rc != RVB_OK) return rc;
    return attenuate_host(ctx, hrtf_model(ctx, mic, facing, up), (uint32_t) channel, in, n, out);
}

int rvb_attenuate_hrtf_device(rvb_ctx * ctx, const float mic[3], const void * d_in, uint64_t n,
                              const float * table, const float facing[3], const float up[3], uint64_t channel, void * d_out)
{
    if (!ctx) return RVB_ERR_INVALID;
    if (!mic || !table || !facing || !up || channel > 1) return fail(ctx, RVB_ERR_INVALID, "rvb_attenuate_hrtf_device: bad argument");
    if (n && (!d_in || !d_out)) return fail(ctx, RVB_ERR_INVALID, "rvb_attenuate_hrtf_device: null buffer");
    if (n && d_in == d_out) return fail(ctx, RVB_ERR_INVALID, "rvb_attenuate_hrtf_device: in-place is not supported");
    RVB_BIND(ctx);
    const int rc = set_one_ear_table(ctx, table, channel);
    if (rc != RVB_OK) return rc;
    return attenuate_device(ctx, hrtf_model(ctx, mic, facing, up), (uint32_t) channel, d_in, n, d_out);
}

int rvb_flatten(rvb_ctx * ctx, const rvb_attenuated_impulse * in, uint64_t n, float sample_rate,
                float * out, uint64_t capacity_bins, uint64_t * nbins)
{
    if (!ctx || !nbins) return RVB_ERR_INVALID;
    if (n && !in) return fail(ctx, RVB_ERR_INVALID, "rvb_flatten: null input");
    if (n >= (1ull << 32)) return fail(ctx, RVB_ERR_CAPACITY, "rvb_flatten: too many impulses");
    RVB_BIND(ctx);
    IrStage & ir = ctx->ir;
    uint64_t bins = ir.query().bins;
    if (!out || !ir.resident(in, n, sample_rate)) {
        // (the sort buffers first: the query whose array flat_in holds is void before the upload overwrites it)
        int rc = ensure_sort_buffers(ctx, n);
        if (rc != RVB_OK) return rc;
        RVB_HIP(fail, ctx, ir.flat_in.ensure(n * sizeof(rvb_attenuated_impulse)));
        if (n && (rc = rvb_copy_to_device(ctx, ir.flat_in.p, in, n * sizeof(rvb_attenuated_impulse))) != RVB_OK) return rc;
        if ((rc = flatten_keys(ctx, ir.flat_in.as<rvb_attenuated_impulse>(), n, sample_rate, &bins)) != RVB_OK) return rc;
    }
    // a size query is remembered for the fill; the fill's sort consumes the keys
    if (out) ir.flatten_filled();
    else ir.flatten_queried(in, n, sample_rate, bins);
    return flatten_finish(ctx, ir.flat_in.as<rvb_attenuated_impulse>(), n, bins, out, capacity_bins, nbins, "rvb_flatten: capacity_bins too small");
}

int rvb_flatten_device(rvb_ctx * ctx, const void * d_attenuated, uint64_t n, float sample_rate,
                       float * out, uint64_t capacity_bins, uint64_t * nbins)
{
    if (!ctx || !nbins) return RVB_ERR_INVALID;
    if (n && !d_attenuated) return fail(ctx, RVB_ERR_INVALID, "rvb_flatten_device: null input");
    if (n >= (1ull << 32)) return fail(ctx, RVB_ERR_CAPACITY, "rvb_flatten_device: too many impulses");
    RVB_BIND(ctx);
    uint64_t bins = 0;
    int rc = ensure_sort_buffers(ctx, n);
    if (rc == RVB_OK) rc = flatten_keys(ctx, reinterpret_cast<const rvb_attenuated_impulse *>(d_attenuated), n, sample_rate, &bins);
    if (rc != RVB_OK) return rc;
    return flatten_finish(ctx, reinterpret_cast<const rvb_attenuated_impulse *>(d_attenuated), n, bins, out, capacity_bins, nbins,
                          "rvb_flatten_device: capacity_bins too small");
}

int rvb_fix_predelay_device(rvb_ctx * ctx, void * d_attenuated, uint64_t n, float seconds)
{
    if (!ctx) return RVB_ERR_INVALID;
    if (n && !d_attenuated) return fail(ctx, RVB_ERR_INVALID, "rvb_fix_predelay_device: null array");
    RVB_BIND(ctx);
    rvb_launch_fix_predelay(reinterpret_cast<rvb_attenuated_impulse *>(d_attenuated), n, seconds, ctx->stream);
    RVB_HIP(fail, ctx, hipGetLastError());
    return RVB_OK;
}

}  // extern "C"
