// ir.hip — from impulses to histograms: the materialised steps of the reference (attenuate per channel, fix the predelay, flatten) and
// the fused impulse-response stage (configure, time range, binning in fast or exact mode, download / export).
#include "bin_blocks.h"
#include "ctx.h"

#include <algorithm>
#include <cstdlib>
#include <cstring>

namespace {

// ---- materialised attenuation / flatten ---------------------------------------------------------

// device layout [ear][RVB_HRTF_ROWS][8]; the last row is the zero padding behind quirk Q5.  `table` holds `ears` ears: they go to the
// slots from `first_ear` on, a slot without a table is zeros.
int upload_hrtf_table(rvb_ctx * ctx, const float * table, int first_ear, int ears)
{
    const size_t rows = RVB_HRTF_ROWS - 1;                 // rows per ear of the caller's table
    std::vector<float> padded((size_t) 2 * RVB_HRTF_ROWS * 8, 0.0f);
    for (int e = 0; e < ears; ++e)
        std::memcpy(padded.data() + (size_t) (first_ear + e) * RVB_HRTF_ROWS * 8, table + (size_t) e * rows * 8, rows * 8 * sizeof(float));
    RVB_HIP(fail, ctx, ctx->hrtf_table.ensure(padded.size() * sizeof(float)));
    RVB_HIP(fail, ctx, hipMemcpy(ctx->hrtf_table.p, padded.data(), padded.size() * sizeof(float), hipMemcpyHostToDevice));
    return RVB_OK;
}

AttenuationModel one_speaker_model(const float mic[3], const rvb_speaker & speaker)
{
    AttenuationModel m;
    m.hrtf = 0;
    m.nchannels = 1;
    for (int i = 0; i < 3; ++i) m.mic[i] = mic[i];
    m.speakers[0] = speaker;
    return m;
}

// (over the table on the device as it is NOW: after the upload that may have replaced its buffer)
AttenuationModel hrtf_model(const rvb_ctx * ctx, const float mic[3], const float facing[3], const float up[3])
{
    AttenuationModel m;
    m.hrtf = 1;
    m.nchannels = 2;
    m.hrtf_table = ctx->hrtf_table.as<const float>();
    for (int i = 0; i < 3; ++i) { m.mic[i] = mic[i]; m.facing[i] = facing[i]; m.up[i] = up[i]; }
    return m;
}

// the attenuate calls of the HRTF model take ONE ear's table: parked in the ear's slot of the device image
int set_one_ear_table(rvb_ctx * ctx, const float * table, uint64_t channel)
{
    RVB_HIP(fail, ctx, hipStreamSynchronize(ctx->stream));           // the table image is about to be replaced
    const int rc = upload_hrtf_table(ctx, table, (int) channel, 1);
    if (rc != RVB_OK) return rc;
    ctx->hrtf_table_ears = 1;                 // (one ear's table in its slot: not what rvb_ir_configure_hrtf(table == NULL) may reuse)
    ctx->ir_configured = false;
    ctx->exact.valid = false;                 // (a prepared list of the HRTF model folds with the table image that has just been replaced)
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
    RVB_HIP(fail, ctx, ctx->scratch_in.ensure(n * sizeof(rvb_impulse)));
    RVB_HIP(fail, ctx, ctx->scratch_out.ensure(n * sizeof(rvb_attenuated_impulse)));
    int rc = rvb_copy_to_device(ctx, ctx->scratch_in.p, in, n * sizeof(rvb_impulse));
    if (rc == RVB_OK) rc = attenuate_device(ctx, m, channel, ctx->scratch_in.p, n, ctx->scratch_out.p);
    if (rc != RVB_OK) return rc;
    return rvb_copy_to_host(ctx, out, ctx->scratch_out.p, n * sizeof(rvb_attenuated_impulse));
}

// keys + max time of a device-resident AttenuatedImpulse array -> *bins
int flatten_keys(rvb_ctx * ctx, const rvb_attenuated_impulse * d_in, uint64_t n, float sample_rate, uint64_t * bins)
{
    int rc = ensure_sort_buffers(ctx, n);
    if (rc != RVB_OK) return rc;
    uint32_t * max_bits = &ctx->small_dev()->max_time_bits;
    RVB_HIP(fail, ctx, hipMemsetAsync(max_bits, 0, 4, ctx->stream));
    rvb_launch_flat_keys(d_in, n, sample_rate, ctx->keys_a.as<uint32_t>(), ctx->vals_a.as<uint32_t>(), max_bits, ctx->stream);
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
    RVB_HIP(fail, ctx, ctx->hist.ensure(bins * 8 * sizeof(float)));
    const int rc = sort_and_bin(ctx, n, bins, key_bits_for(bins), true);
    if (rc != RVB_OK) return rc;
    rvb_launch_flat_ordered_sum(d_in, ctx->keys_b.as<uint32_t>(), ctx->vals_b.as<uint32_t>(), ctx->bin_starts.as<uint32_t>(), n, bins,
                                ctx->hist.as<float>(), ctx->stream);
    RVB_HIP(fail, ctx, hipGetLastError());
    RVB_HIP(fail, ctx, hipMemcpyAsync(out, ctx->hist.p, bins * 8 * sizeof(float), hipMemcpyDeviceToHost, ctx->stream));
    RVB_HIP(fail, ctx, hipStreamSynchronize(ctx->stream));
    return RVB_OK;
}

// ---- fused impulse-response stage ----------------------------------------------------------------

}  // namespace

int ir_configure_refusals(rvb_ctx * ctx, int which)
{
    if (!ctx->traced) return fail(ctx, RVB_ERR_STATE, "rvb_ir_configure: nothing traced");
    if (which < 1 || which > 3) return fail(ctx, RVB_ERR_INVALID, "rvb_ir_configure: which must be 1..3");
    return RVB_OK;
}

// (behind ir_configure_refusals, which every caller has passed)
int ir_configure_images(rvb_ctx * ctx, int which, const rvb_impulse * images, uint64_t nimages, bool gathered)
{
    if (!gathered && nimages && !images) return fail(ctx, RVB_ERR_INVALID, "rvb_ir_configure: null images");
    if (nimages * sizeof(rvb_impulse) > ctx->images.cap)
        RVB_HIP(fail, ctx, hipStreamSynchronize(ctx->stream));          // the buffer is about to be replaced
    RVB_HIP(fail, ctx, ctx->images.ensure(nimages * sizeof(rvb_impulse)));
    ctx->nimages = nimages;
    if (gathered) {
        ctx->images_host.clear();
    } else {
        ctx->images_host.assign(images, images + nimages);
        // in stream order (kernels of an earlier configuration that read the old images run before it); the source is the
        // context's own copy, which lives until the next configure
        if (nimages) RVB_HIP(fail, ctx, hipMemcpyAsync(ctx->images.p, ctx->images_host.data(), nimages * sizeof(rvb_impulse), hipMemcpyHostToDevice, ctx->stream));
    }
    ctx->images_host_stale = gathered;
    ctx->merged.configured = gathered;
    ctx->which = which;
    ctx->ir_configured = true;
    ctx->exact.valid = false;
    ctx->range_pending = false;
    return RVB_OK;
}

// A list gathered on the device (rvb_ir_configure_*_merged): its host copy, fetched once per configuration by the first reader.
int ir_images_on_host(rvb_ctx * ctx)
{
    if (!ctx->images_host_stale) return RVB_OK;
    ctx->images_host.resize(ctx->nimages);
    if (ctx->nimages)
        RVB_HIP(fail, ctx, hipMemcpyAsync(ctx->images_host.data(), ctx->images.p, ctx->nimages * sizeof(rvb_impulse), hipMemcpyDeviceToHost, ctx->stream));
    RVB_HIP(fail, ctx, hipStreamSynchronize(ctx->stream));
    ctx->images_host_stale = false;
    return RVB_OK;
}

int ir_speaker_model(rvb_ctx * ctx, const float mic[3], const rvb_speaker * speakers, uint64_t nspeakers)
{
    if (!mic || !speakers || nspeakers == 0 || nspeakers > RVB_MAX_SPEAKERS)
        return fail(ctx, RVB_ERR_INVALID, "rvb_ir_configure_speakers: 1.." RVB_STR(RVB_MAX_SPEAKERS) " speakers required");
    RVB_BIND(ctx);
    AttenuationModel m;
    m.hrtf = 0;
    m.nchannels = (uint32_t) nspeakers;
    for (int i = 0; i < 3; ++i) m.mic[i] = mic[i];
    for (uint64_t s = 0; s < nspeakers && s < 8; ++s) m.speakers[s] = speakers[s];
    if (nspeakers > 8) {
        // the wide kernels read their speakers from device memory: uploaded in stream order like the images (kernels of an earlier
        // configuration that read the old table run before the copy; the source is the context's own copy, alive until the next configure)
        if (nspeakers * sizeof(float4) > ctx->speakers.cap)
            RVB_HIP(fail, ctx, hipStreamSynchronize(ctx->stream));          // the buffer is about to be replaced
        RVB_HIP(fail, ctx, ctx->speakers.ensure(RVB_MAX_SPEAKERS * sizeof(float4)));
        ctx->speakers_host.resize(nspeakers);
        rvb_make_speaker_table(speakers, nspeakers, ctx->speakers_host.data());
        RVB_HIP(fail, ctx, hipMemcpyAsync(ctx->speakers.p, ctx->speakers_host.data(), nspeakers * sizeof(float4), hipMemcpyHostToDevice, ctx->stream));
        m.speaker_table = ctx->speakers.as<const float4>();
    }
    ctx->model = m;
    return RVB_OK;
}

int ir_hrtf_model(rvb_ctx * ctx, const float mic[3], const float * table, const float facing[3], const float up[3])
{
    if (!mic || !facing || !up) return fail(ctx, RVB_ERR_INVALID, "rvb_ir_configure_hrtf: null argument");
    RVB_BIND(ctx);
    if (table) {
        // (the table on the device may still be read by kernels enqueued under the previous configuration)
        RVB_HIP(fail, ctx, hipStreamSynchronize(ctx->stream));
        int rc = upload_hrtf_table(ctx, table, 0, 2);
        if (rc != RVB_OK) return rc;
        ctx->hrtf_table_ears = 2;
    } else if (ctx->hrtf_table_ears != 2) {
        // table == NULL: the two-ear table of the previous rvb_ir_configure_hrtf on this context stays (a caller that configures many
        // listeners with one table — the pipeline — uploads its 4 MB once, not per impulse response)
        return fail(ctx, RVB_ERR_STATE, "rvb_ir_configure_hrtf: table == NULL needs an earlier call with a table on this context");
    }
    ctx->model = hrtf_model(ctx, mic, facing, up);
    return RVB_OK;
}

namespace {

// HRTF model: the attenuated time of an impulse differs per ear (kernel.cpp:616-622), so the range needs a pass over the impulses; the
// pass and the copy of its two words to pinned host memory are ENQUEUED here and waited for in rvb_ir_time_range — a caller with several
// contexts enqueues all of them (rvb_ir_time_range_begin) before it waits for the first.
int time_range_enqueue(rvb_ctx * ctx)
{
    uint32_t * range = ctx->small_dev()->range;
    RVB_HIP(fail, ctx, hipMemsetAsync(range, 0xFF, 4, ctx->stream));
    RVB_HIP(fail, ctx, hipMemsetAsync(range + 1, 0, 4, ctx->stream));
    ctx->reset_timings();
    ctx->begin_timing("time_range_kernel");
    if (ctx->which & RVB_IR_DIFFUSE)
        rvb_launch_time_range(ctx->model, ir_diffuse(ctx), ctx->nrays * ctx->nreflections, range, ctx->stream);
    if (ctx->which & RVB_IR_IMAGES)
        rvb_launch_time_range(ctx->model, ctx->images.as<rvb_impulse>(), ctx->nimages, range, ctx->stream);
    ctx->end_timing();
    RVB_HIP(fail, ctx, hipGetLastError());
    RVB_HIP(fail, ctx, hipMemcpyAsync(ctx->range_host, range, 8, hipMemcpyDeviceToHost, ctx->stream));
    ctx->range_pending = true;
    return RVB_OK;
}

// What exact mode works on, against its limits, and the sort buffers for `lists` entries per impulse.
int exact_begin(rvb_ctx * ctx, uint64_t nbins, uint64_t lists, rvb_ctx::ExactState & in)
{
    in.nbins = nbins;
    in.ndiffuse = (ctx->which & RVB_IR_DIFFUSE) ? ctx->nrays * ctx->nreflections : 0;
    in.nimages = (ctx->which & RVB_IR_IMAGES) ? ctx->nimages : 0;
    in.n = in.ndiffuse + in.nimages;
    if (in.n >= (1ull << 31)) return fail(ctx, RVB_ERR_CAPACITY, "rvb_ir_accumulate: too many impulses for exact mode");
    if (nbins >= 0x7FFFFFF0ull) return fail(ctx, RVB_ERR_CAPACITY, "rvb_ir_accumulate: too many bins for exact mode");
    ctx->flat_host = nullptr;                 // keys_a / vals_a are rewritten by the caller: a pending rvb_flatten size query is void
    return ensure_sort_buffers(ctx, lists * in.n);
}

// One channel's list: keys are bins, nbins itself marks "adds nothing" (key_bits_for(nbins) bits cover 0 .. nbins); sorted, with bin boundaries.
int exact_list(rvb_ctx * ctx, const rvb_ctx::ExactState & in, uint32_t channel, float predelay, float sample_rate, uint64_t nbins, bool may_sort_own)
{
    uint32_t * keys = ctx->keys_a.as<uint32_t>(), * values = ctx->vals_a.as<uint32_t>();
    rvb_launch_bin_keys(ctx->model, channel, ir_diffuse(ctx), in.ndiffuse, 0, predelay, sample_rate, (uint32_t) nbins, keys, values, ctx->stream);
    rvb_launch_bin_keys(ctx->model, channel, ctx->images.as<rvb_impulse>(), in.nimages, in.ndiffuse, predelay, sample_rate, (uint32_t) nbins, keys, values, ctx->stream);
    return sort_and_bin(ctx, in.n, nbins, key_bits_for(nbins), may_sort_own);
}

// Exact mode, step 1 (everything that does not depend on what the histogram holds): per-impulse bin keys, the radix sort, where each
// bin's run starts and ends.  Speaker channels keep the input time (kernel.cpp:530-533) and share ONE sorted list; the two HRTF ears
// shift the arrival time differently (kernel.cpp:616-622) and are keyed in one pass into ONE list of 2 n entries (bin_keys_hrtf_kernel).
int exact_prepare(rvb_ctx * ctx, float predelay, float sample_rate, uint64_t nbins)
{
    const AttenuationModel & m = ctx->model;
    rvb_ctx::ExactState in;
    int rc = exact_begin(ctx, nbins, m.hrtf ? 2 : 1, in);
    if (rc != RVB_OK) return rc;
    if (m.hrtf) {
        uint32_t * keys = ctx->keys_a.as<uint32_t>(), * values = ctx->vals_a.as<uint32_t>();
        const uint64_t nkeys = 2 * (nbins + 1);
        rvb_launch_bin_keys_hrtf(m, ir_diffuse(ctx), in.ndiffuse, 0, in.n, predelay, sample_rate, (uint32_t) nbins, keys, values, ctx->stream);
        rvb_launch_bin_keys_hrtf(m, ctx->images.as<rvb_impulse>(), in.nimages, in.ndiffuse, in.n, predelay, sample_rate, (uint32_t) nbins, keys, values, ctx->stream);
        // (explicit values — the two halves carry the same impulse numbers — and always rocPRIM's sort: RVB_SORT=own takes identity values only.
        // Values derived from the entry's position by a transform iterator instead of an array: 1.52 -> 1.58 ms, and 0.85 -> 0.88 ms for the
        // one-list speaker form; rocPRIM's first pass reads an array faster than it evaluates an iterator.)
        rc = sort_and_bin(ctx, 2 * in.n, nkeys, key_bits_for(nkeys - 1), false);
    } else {
        rc = exact_list(ctx, in, 0, predelay, sample_rate, nbins, true);
    }
    if (rc != RVB_OK) return rc;
    RVB_HIP(fail, ctx, hipGetLastError());
    in.valid = true;                          // (ensure_sort_buffers above cleared the context's)
    in.hrtf_combined = m.hrtf != 0;
    ctx->exact = in;
    return RVB_OK;
}

// Exact mode, step 2: bins [b0, b1) — every bin's impulses added in impulse order ON TOP of what the histogram holds (rayverb.cpp:67-74).
int exact_fold(rvb_ctx * ctx, uint64_t b0, uint64_t b1, float * hist)
{
    const AttenuationModel & m = ctx->model;
    const rvb_ctx::ExactState & e = ctx->exact;
    if (!e.valid) return fail(ctx, RVB_ERR_STATE, "rvb_ir_exact_fold: rvb_ir_exact_prepare first (and nothing that reuses the sort buffers in between)");
    if (b1 > e.nbins) b1 = e.nbins;
    if (e.hrtf_combined) {
        const uint64_t nkeys = 2 * (e.nbins + 1);
        rvb_launch_ordered_sum_hrtf(m, ir_diffuse(ctx), e.ndiffuse, ctx->images.as<rvb_impulse>(), ctx->vals_b.as<uint32_t>(),
                                    ctx->bin_starts.as<uint32_t>(), ctx->bin_starts.as<uint32_t>() + nkeys, e.nbins, hist, ctx->stream, b0, b1);
    } else if (m.nchannels > 8) {
        rvb_launch_ordered_sum_wide(m, ir_diffuse(ctx), e.ndiffuse, ctx->images.as<rvb_impulse>(), ctx->vals_b.as<uint32_t>(),
                                    ctx->bin_starts.as<uint32_t>(), ctx->bin_starts.as<uint32_t>() + e.nbins, e.n, e.nbins, hist, ctx->stream, b0, b1);
    } else {
        rvb_launch_ordered_sum(m, 0, m.nchannels, ir_diffuse(ctx), e.ndiffuse, ctx->images.as<rvb_impulse>(), ctx->vals_b.as<uint32_t>(),
                               ctx->bin_starts.as<uint32_t>(), ctx->bin_starts.as<uint32_t>() + e.nbins, e.n, e.nbins, hist, ctx->stream, b0, b1);
    }
    RVB_HIP(fail, ctx, hipGetLastError());
    return RVB_OK;
}

// Bins [b0, b1) of every row of the [rows][nbins] histogram leave for pinned host memory on the export stream, behind what the context's
// stream holds now (rvb_copy_to_pinned_host_async for a bin range: one strided copy).
int export_bin_range(rvb_ctx * ctx, float * pinned_dst, const float * hist, uint64_t rows, uint64_t nbins, uint64_t b0, uint64_t b1)
{
    if (b1 <= b0) return RVB_OK;
    RVB_HIP(fail, ctx, hipEventRecord(ctx->export_ready, ctx->stream));
    RVB_HIP(fail, ctx, hipStreamWaitEvent(ctx->export_stream, ctx->export_ready, 0));
    if (b0 == 0 && b1 == nbins) {
        RVB_HIP(fail, ctx, hipMemcpyAsync(pinned_dst, hist, rows * nbins * sizeof(float), hipMemcpyDeviceToHost, ctx->export_stream));
    } else {
        RVB_HIP(fail, ctx, hipMemcpy2DAsync(pinned_dst + b0, nbins * sizeof(float), hist + b0, nbins * sizeof(float), (b1 - b0) * sizeof(float), rows,
                                            hipMemcpyDeviceToHost, ctx->export_stream));
    }
    return RVB_OK;
}

// rvb_ir_accumulate, and — with pinned_dst — the histogram's way to the host: in exact mode with the speaker model the last kernel of the
// stage (ordered_sum_kernel: a lane pair per bin) runs bin range by bin range and every range's copy is enqueued behind it, so the link
// is busy while the later ranges are still being folded; the other forms copy the finished histogram in one piece.
int ir_accumulate_impl(rvb_ctx * ctx, float predelay, float sample_rate, uint64_t nbins, int mode, void * d_histogram,
                       float * pinned_dst, uint32_t slices)
{
    if (!ctx) return RVB_ERR_INVALID;
    if (!ctx->ir_configured) return fail(ctx, RVB_ERR_STATE, "rvb_ir_accumulate: rvb_ir_configure_* first");
    if (!d_histogram || nbins == 0) return fail(ctx, RVB_ERR_INVALID, "rvb_ir_accumulate: null histogram or no bins");
    RVB_BIND(ctx);
    if (slices == 0) slices = 1;
    bool exported = false;
    const AttenuationModel & m = ctx->model;
    const uint64_t ndiffuse = (ctx->which & RVB_IR_DIFFUSE) ? ctx->nrays * ctx->nreflections : 0;
    const uint64_t nimages = (ctx->which & RVB_IR_IMAGES) ? ctx->nimages : 0;
    float * hist = reinterpret_cast<float *>(d_histogram);
    ctx->reset_timings();
    // More than 8 speakers: RVB_IR_FAST runs the sorted fold too.  An atomic histogram adds 32 bytes per live impulse and channel at
    // the chip-wide float-atomic rate (about 6.5 ms for 32 channels at workload C2 before its transpose); the fold gathers each record
    // once for all channels and writes with plain stores (profiles/speaker_arrays_n1.txt).  Its sums are the exact mode's, which meet
    // the fast mode's bound trivially.
    const bool wide = !m.hrtf && m.nchannels > 8;
    if (mode == RVB_IR_FAST && !wide) {
        const size_t acc_bytes = (size_t) nbins * m.nchannels * 8 * sizeof(float);
        RVB_HIP(fail, ctx, ctx->acc.ensure(acc_bytes));
        RVB_HIP(fail, ctx, hipMemsetAsync(ctx->acc.p, 0, acc_bytes, ctx->stream));
        ctx->begin_timing("histogram_fast_kernel");
        rvb_launch_histogram_fast(m, ir_diffuse(ctx), ndiffuse, predelay, sample_rate, nbins, ctx->acc.as<float>(), ctx->stream);
        rvb_launch_histogram_fast(m, ctx->images.as<rvb_impulse>(), nimages, predelay, sample_rate, nbins, ctx->acc.as<float>(), ctx->stream);
        ctx->end_timing();
        ctx->begin_timing("histogram_transpose_kernel");
        rvb_launch_histogram_transpose(ctx->acc.as<float>(), hist, m.nchannels, nbins, ctx->stream);
        ctx->end_timing();
    } else if (mode == RVB_IR_EXACT || mode == RVB_IR_FAST) {
        const char * split_env = getenv("RVB_HRTF_SPLIT_EARS");     // measurement / test switch (read per call): one list per ear, as in round 2
        const bool split_ears = m.hrtf && split_env && split_env[0] == '1';
        ctx->begin_timing(mode == RVB_IR_FAST ? "sorted_fold_wide" : "exact_mode");
        if (!split_ears) {
            // one sorted list (speaker channels share it; the two HRTF ears are keyed into one list of 2 n entries), then the fold —
            // bin range by bin range when the histogram leaves for the host as it becomes final
            int rc = exact_prepare(ctx, predelay, sample_rate, nbins);
            if (rc != RVB_OK) return rc;
            const uint32_t parts = pinned_dst ? slices : 1u;
            const BinBlocks pieces(nbins, parts);                                  // whole 64-byte segments
            for (uint64_t k = 0; k < pieces.count(); ++k) {
                const uint64_t b0 = pieces.range(k).b0, b1 = pieces.range(k).b1;
                rc = exact_fold(ctx, b0, b1, hist);
                if (rc == RVB_OK && pinned_dst && parts > 1) rc = export_bin_range(ctx, pinned_dst, hist, (uint64_t) m.nchannels * 8, nbins, b0, b1);
                if (rc != RVB_OK) return rc;
            }
            exported = pinned_dst && parts > 1;
        } else {
            // a list per ear: keys, sorted list and bin boundaries, that ear's fold
            rvb_ctx::ExactState in;
            int rc = exact_begin(ctx, nbins, 1, in);
            if (rc != RVB_OK) return rc;
            for (uint32_t ch = 0; ch < m.nchannels; ++ch) {
                if ((rc = exact_list(ctx, in, ch, predelay, sample_rate, nbins, false)) != RVB_OK) return rc;      // (always rocPRIM's sort, as round 2 had it)
                rvb_launch_ordered_sum(m, ch, 1u, ir_diffuse(ctx), ndiffuse, ctx->images.as<rvb_impulse>(),
                                       ctx->vals_b.as<uint32_t>(), ctx->bin_starts.as<uint32_t>(), ctx->bin_starts.as<uint32_t>() + nbins, in.n, nbins, hist, ctx->stream);
            }
        }
        ctx->end_timing();
    } else {
        return fail(ctx, RVB_ERR_INVALID, "rvb_ir_accumulate: unknown mode");
    }
    RVB_HIP(fail, ctx, hipGetLastError());
    if (pinned_dst && !exported) return export_bin_range(ctx, pinned_dst, hist, (uint64_t) m.nchannels * 8, nbins, 0, nbins);
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
    // the fill that follows a size query of the same array finds it (and its keys) on the device
    const bool resident = out && ctx->flat_host == in && ctx->flat_n == n && ctx->flat_rate == sample_rate && in != nullptr;
    uint64_t bins = ctx->flat_bins;
    if (!resident) {
        ctx->flat_host = nullptr;
        RVB_HIP(fail, ctx, ctx->flat_in.ensure(n * sizeof(rvb_attenuated_impulse)));
        if (n) {
            int rc = rvb_copy_to_device(ctx, ctx->flat_in.p, in, n * sizeof(rvb_attenuated_impulse));
            if (rc != RVB_OK) return rc;
        }
        int rc = flatten_keys(ctx, ctx->flat_in.as<rvb_attenuated_impulse>(), n, sample_rate, &bins);
        if (rc != RVB_OK) return rc;
    }
    if (!out) { ctx->flat_n = n; ctx->flat_rate = sample_rate; ctx->flat_bins = bins; }
    ctx->flat_host = out ? nullptr : in;      // a size query is remembered for the fill; the fill's sort consumes the keys
    return flatten_finish(ctx, ctx->flat_in.as<rvb_attenuated_impulse>(), n, bins, out, capacity_bins, nbins, "rvb_flatten: capacity_bins too small");
}

int rvb_flatten_device(rvb_ctx * ctx, const void * d_attenuated, uint64_t n, float sample_rate,
                       float * out, uint64_t capacity_bins, uint64_t * nbins)
{
    if (!ctx || !nbins) return RVB_ERR_INVALID;
    if (n && !d_attenuated) return fail(ctx, RVB_ERR_INVALID, "rvb_flatten_device: null input");
    if (n >= (1ull << 32)) return fail(ctx, RVB_ERR_CAPACITY, "rvb_flatten_device: too many impulses");
    RVB_BIND(ctx);
    ctx->flat_host = nullptr;
    uint64_t bins = 0;
    int rc = flatten_keys(ctx, reinterpret_cast<const rvb_attenuated_impulse *>(d_attenuated), n, sample_rate, &bins);
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

int rvb_ir_configure_speakers(rvb_ctx * ctx, const float mic[3], const rvb_speaker * speakers, uint64_t nspeakers,
                              int which, const rvb_impulse * images, uint64_t nimages)
{
    if (!ctx) return RVB_ERR_INVALID;
    int rc = ir_speaker_model(ctx, mic, speakers, nspeakers);
    if (rc == RVB_OK) rc = ir_configure_refusals(ctx, which);
    return rc == RVB_OK ? ir_configure_images(ctx, which, images, nimages, false) : rc;
}

int rvb_ir_configure_hrtf(rvb_ctx * ctx, const float mic[3], const float * table, const float facing[3], const float up[3],
                          int which, const rvb_impulse * images, uint64_t nimages)
{
    if (!ctx) return RVB_ERR_INVALID;
    int rc = ir_hrtf_model(ctx, mic, table, facing, up);
    if (rc == RVB_OK) rc = ir_configure_refusals(ctx, which);
    return rc == RVB_OK ? ir_configure_images(ctx, which, images, nimages, false) : rc;
}

int rvb_ir_time_range_begin(rvb_ctx * ctx)
{
    if (!ctx) return RVB_ERR_INVALID;
    if (!ctx->ir_configured) return fail(ctx, RVB_ERR_STATE, "rvb_ir_time_range_begin: rvb_ir_configure_* first");
    RVB_BIND(ctx);
    if (!ctx->model.hrtf) return RVB_OK;          // speakers: the range came with the trace (reduced inside the shadow kernel)
    return time_range_enqueue(ctx);
}

int rvb_ir_time_range(rvb_ctx * ctx, float * min_nonzero_time, float * max_time)
{
    if (!ctx) return RVB_ERR_INVALID;
    if (!ctx->ir_configured) return fail(ctx, RVB_ERR_STATE, "rvb_ir_time_range: rvb_ir_configure_* first");
    RVB_BIND(ctx);
    uint32_t got[2] = {0xFFFFFFFFu, 0u};          // float bits: earliest non-zero time (all ones: none), latest time
    if (ctx->model.hrtf) {
        if (!ctx->range_pending) {
            const int rc = time_range_enqueue(ctx);
            if (rc != RVB_OK) return rc;
        }
        ctx->range_pending = false;
        RVB_HIP(fail, ctx, hipStreamSynchronize(ctx->stream));
        std::memcpy(got, ctx->range_host, sizeof(got));
    } else {
        // Speaker channels keep the input time (kernel.cpp:530-533), so the range is that of the raw
        // impulses: the diffuse part was reduced inside shadow_kernel, the few images are scanned below.
        ctx->reset_timings();
        if (ctx->which & RVB_IR_DIFFUSE) {
            int rc = fetch_small(ctx);
            if (rc != RVB_OK) return rc;
            if (ctx->npairs > 1) { got[0] = ctx->pairs.range_of(ctx->ir_pair)[0]; got[1] = ctx->pairs.range_of(ctx->ir_pair)[1]; }
            else std::memcpy(got, ctx->small_host->trace_range, sizeof(got));
        }
    }
    float lo = 0.0f, hi = 0.0f;
    bool have_lo = got[0] != 0xFFFFFFFFu;
    if (have_lo) std::memcpy(&lo, &got[0], 4);
    std::memcpy(&hi, &got[1], 4);
    if (!ctx->model.hrtf && (ctx->which & RVB_IR_IMAGES)) {
        const int rc = ir_images_on_host(ctx);                  // (a list gathered on the device comes down once)
        if (rc != RVB_OK) return rc;
        for (const rvb_impulse & im : ctx->images_host) {
            bool nonzero = false;
            for (int b = 0; b < 8; ++b) nonzero = nonzero || im.volume[b] != 0.0f;
            if (!nonzero) continue;
            if (im.time != 0.0f && (!have_lo || im.time < lo)) { lo = im.time; have_lo = true; }
            if (im.time > hi) hi = im.time;
        }
    }
    if (min_nonzero_time) *min_nonzero_time = have_lo ? lo : 0.0f;
    if (max_time) *max_time = hi;
    return RVB_OK;
}

uint64_t rvb_ir_bins(float max_time, float predelay, float sample_rate)
{
    return bins_for(max_time, predelay, sample_rate);
}

int rvb_ir_accumulate(rvb_ctx * ctx, float predelay, float sample_rate, uint64_t nbins, int mode, void * d_histogram)
{
    const int rc = ir_accumulate_impl(ctx, predelay, sample_rate, nbins, mode, d_histogram, nullptr, 1);
    if (ctx && rc == RVB_OK) ctx->exact.valid = false;        // include/rvb_capi.h: rvb_ir_accumulate voids a prepared list, whatever its mode and its nbins
    return rc;
}

int rvb_ir_accumulate_export(rvb_ctx * ctx, float predelay, float sample_rate, uint64_t nbins, int mode, void * d_histogram,
                             void * pinned_dst, uint32_t slices)
{
    if (ctx && !pinned_dst) return fail(ctx, RVB_ERR_INVALID, "rvb_ir_accumulate_export: null destination");
    // Default: ONE piece.  Measured at workload C2 (profiles/r04_export_slices_n1.txt): 1 / 2 / 4 / 8 bin ranges leave one impulse response
    // on the host after 6.98 / 7.04 / 7.02 / 7.00 ms (5.88 ms to HBM: the 54 MB need 1.1 ms of the link whenever they start, and the fold they
    // could overlap is 0.27 ms split into launches that cost what the overlap gains) and the pipeline at 4.82 / 4.81 / 4.80 / 4.96 ms per IR.
    const int rc = ir_accumulate_impl(ctx, predelay, sample_rate, nbins, mode, d_histogram, static_cast<float *>(pinned_dst), slices ? slices : 1u);
    if (ctx && rc == RVB_OK) ctx->exact.valid = false;
    return rc;
}

int rvb_ir_exact_prepare(rvb_ctx * ctx, float predelay, float sample_rate, uint64_t nbins)
{
    if (!ctx) return RVB_ERR_INVALID;
    if (!ctx->ir_configured) return fail(ctx, RVB_ERR_STATE, "rvb_ir_exact_prepare: rvb_ir_configure_* first");
    if (nbins == 0) return fail(ctx, RVB_ERR_INVALID, "rvb_ir_exact_prepare: no bins");
    RVB_BIND(ctx);
    ctx->reset_timings();
    ctx->begin_timing("exact_prepare");
    const int rc = exact_prepare(ctx, predelay, sample_rate, nbins);
    ctx->end_timing();
    return rc;
}

int rvb_ir_exact_fold(rvb_ctx * ctx, uint64_t nbins, uint64_t bin_begin, uint64_t bin_end, void * d_histogram)
{
    if (!ctx) return RVB_ERR_INVALID;
    if (!d_histogram) return fail(ctx, RVB_ERR_INVALID, "rvb_ir_exact_fold: null histogram");
    if (!ctx->exact.valid || ctx->exact.nbins != nbins) return fail(ctx, RVB_ERR_STATE, "rvb_ir_exact_fold: rvb_ir_exact_prepare with this nbins first");
    if (bin_begin > bin_end) return fail(ctx, RVB_ERR_INVALID, "rvb_ir_exact_fold: bin range");
    RVB_BIND(ctx);
    return exact_fold(ctx, bin_begin, bin_end, static_cast<float *>(d_histogram));
}

int rvb_ir_download(rvb_ctx * ctx, int trim_predelay, float sample_rate, int mode,
                    float * out, uint64_t capacity_bins, uint64_t * nbins)
{
    if (!ctx || !nbins) return RVB_ERR_INVALID;
    float lo = 0.0f, hi = 0.0f;
    int rc = rvb_ir_time_range(ctx, &lo, &hi);
    if (rc != RVB_OK) return rc;
    const float predelay = trim_predelay ? lo : 0.0f;
    const uint64_t bins = bins_for(hi, predelay, sample_rate);
    *nbins = bins;
    if (!out)
        return RVB_OK;
    if (capacity_bins < bins)
        return fail(ctx, RVB_ERR_CAPACITY, "rvb_ir_download: capacity_bins too small");
    const size_t bytes = (size_t) bins * ctx->model.nchannels * 8 * sizeof(float);
    RVB_HIP(fail, ctx, ctx->hist.ensure(bytes));
    RVB_HIP(fail, ctx, hipMemsetAsync(ctx->hist.p, 0, bytes, ctx->stream));
    rc = rvb_ir_accumulate(ctx, predelay, sample_rate, bins, mode, ctx->hist.p);
    if (rc != RVB_OK) return rc;
    RVB_HIP(fail, ctx, hipMemcpyAsync(out, ctx->hist.p, bytes, hipMemcpyDeviceToHost, ctx->stream));
    RVB_HIP(fail, ctx, hipStreamSynchronize(ctx->stream));
    return RVB_OK;
}

}  // extern "C"
