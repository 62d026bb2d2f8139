// ir.hip — from impulses to histograms, the fused impulse-response stage: configure, time range, binning in fast or exact mode,
// download / export.  Its state is IrStage (ctx.h) over IrState (ir_state.h); the materialised steps of the reference are flatten.hip's.
#include "bin_blocks.h"
#include "ctx.h"

#include <algorithm>
#include <cstdlib>
#include <cstring>

// device layout [ear][RVB_HRTF_ROWS][8]; the last row is the zero padding behind quirk Q5.  `table` holds `ears` ears: they go to the
// slots from `first_ear` on, a slot without a table is zeros.
int upload_hrtf_table(rvb_ctx * ctx, const float * table, int first_ear, int ears)
{
    const size_t rows = RVB_HRTF_ROWS - 1;                 // rows per ear of the caller's table
    std::vector<float> padded((size_t) 2 * RVB_HRTF_ROWS * 8, 0.0f);
    for (int e = 0; e < ears; ++e)
        std::memcpy(padded.data() + (size_t) (first_ear + e) * RVB_HRTF_ROWS * 8, table + (size_t) e * rows * 8, rows * 8 * sizeof(float));
    RVB_HIP(fail, ctx, ctx->ir.hrtf_table.ensure(padded.size() * sizeof(float)));
    RVB_HIP(fail, ctx, hipMemcpy(ctx->ir.hrtf_table.p, padded.data(), padded.size() * sizeof(float), hipMemcpyHostToDevice));
    return RVB_OK;
}

// (over the table on the device as it is NOW: after the upload that may have replaced its buffer)
AttenuationModel hrtf_model(const rvb_ctx * ctx, const float mic[3], const float facing[3], const float up[3])
{
    AttenuationModel m;
    m.hrtf = 1;
    m.nchannels = 2;
    m.hrtf_table = ctx->ir.hrtf_table.as<const float>();
    for (int i = 0; i < 3; ++i) { m.mic[i] = mic[i]; m.facing[i] = facing[i]; m.up[i] = up[i]; }
    return m;
}

int ir_configure_refusals(rvb_ctx * ctx, int which)
{
    if (!ctx->trace.traced()) return fail(ctx, RVB_ERR_STATE, "rvb_ir_configure: nothing traced");
    if (which < 1 || which > 3) return fail(ctx, RVB_ERR_INVALID, "rvb_ir_configure: which must be 1..3");
    return RVB_OK;
}

// (behind ir_configure_refusals, which every caller has passed)
int ir_configure_images(rvb_ctx * ctx, int which, const rvb_impulse * images, uint64_t nimages, bool gathered)
{
    if (!gathered && nimages && !images) return fail(ctx, RVB_ERR_INVALID, "rvb_ir_configure: null images");
    IrStage & ir = ctx->ir;
    if (nimages * sizeof(rvb_impulse) > ir.images.cap)
        RVB_HIP(fail, ctx, hipStreamSynchronize(ctx->stream));          // the buffer is about to be replaced
    RVB_HIP(fail, ctx, ir.images.ensure(nimages * sizeof(rvb_impulse)));
    if (gathered) {
        ir.images_host.clear();
    } else {
        ir.images_host.assign(images, images + nimages);
        // in stream order (kernels of an earlier configuration that read the old images run before it); the source is the
        // context's own copy, which lives until the next configure
        if (nimages) RVB_HIP(fail, ctx, hipMemcpyAsync(ir.images.p, ir.images_host.data(), nimages * sizeof(rvb_impulse), hipMemcpyHostToDevice, ctx->stream));
    }
    ir.configure(which, nimages, gathered);
    return RVB_OK;
}

// A list gathered on the device (rvb_ir_configure_*_merged): its host copy, fetched once per configuration by the first reader.
int ir_images_on_host(rvb_ctx * ctx)
{
    IrStage & ir = ctx->ir;
    if (!ir.host_images_stale()) return RVB_OK;
    ir.images_host.resize(ir.nimages());
    if (ir.nimages())
        RVB_HIP(fail, ctx, hipMemcpyAsync(ir.images_host.data(), ir.images.p, ir.nimages() * sizeof(rvb_impulse), hipMemcpyDeviceToHost, ctx->stream));
    RVB_HIP(fail, ctx, hipStreamSynchronize(ctx->stream));
    ir.images_fetched();
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
        if (nspeakers * sizeof(float4) > ctx->ir.speakers.cap)
            RVB_HIP(fail, ctx, hipStreamSynchronize(ctx->stream));          // the buffer is about to be replaced
        RVB_HIP(fail, ctx, ctx->ir.speakers.ensure(RVB_MAX_SPEAKERS * sizeof(float4)));
        ctx->ir.speakers_host.resize(nspeakers);
        rvb_make_speaker_table(speakers, nspeakers, ctx->ir.speakers_host.data());
        RVB_HIP(fail, ctx, hipMemcpyAsync(ctx->ir.speakers.p, ctx->ir.speakers_host.data(), nspeakers * sizeof(float4), hipMemcpyHostToDevice, ctx->stream));
        m.speaker_table = ctx->ir.speakers.as<const float4>();
    }
    ctx->ir.model = m;
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
        ctx->ir.two_ear_table();
    } else if (ctx->ir.table_ears() != 2) {
        // table == NULL: the two-ear table of the previous rvb_ir_configure_hrtf on this context stays (a caller that configures many
        // listeners with one table — the pipeline — uploads its 4 MB once, not per impulse response)
        return fail(ctx, RVB_ERR_STATE, "rvb_ir_configure_hrtf: table == NULL needs an earlier call with a table on this context");
    }
    ctx->ir.model = hrtf_model(ctx, mic, facing, up);
    return RVB_OK;
}

namespace {

// HRTF model: the attenuated time of an impulse differs per ear (kernel.cpp:616-622), so the range needs a pass over the impulses; the
// pass and the copy of its two words to pinned host memory are ENQUEUED here and waited for in rvb_ir_time_range — a caller with several
// contexts enqueues all of them (rvb_ir_time_range_begin) before it waits for the first.
int time_range_enqueue(rvb_ctx * ctx)
{
    uint32_t * range = ctx->trace.small_dev()->range;
    RVB_HIP(fail, ctx, hipMemsetAsync(range, 0xFF, 4, ctx->stream));
    RVB_HIP(fail, ctx, hipMemsetAsync(range + 1, 0, 4, ctx->stream));
    ctx->reset_timings();
    ctx->begin_timing("time_range_kernel");
    if (ctx->ir.which() & RVB_IR_DIFFUSE)
        rvb_launch_time_range(ctx->ir.model, ir_diffuse(ctx), ctx->nrays * ctx->trace.nreflections(), range, ctx->stream);
    if (ctx->ir.which() & RVB_IR_IMAGES)
        rvb_launch_time_range(ctx->ir.model, ctx->ir.images.as<rvb_impulse>(), ctx->ir.nimages(), range, ctx->stream);
    ctx->end_timing();
    RVB_HIP(fail, ctx, hipGetLastError());
    RVB_HIP(fail, ctx, hipMemcpyAsync(ctx->trace.host->hrtf_range, range, 8, hipMemcpyDeviceToHost, ctx->stream));
    ctx->ir.range_enqueued();
    return RVB_OK;
}

// What exact mode works on, against its limits, and the sort buffers for `lists` entries per impulse.
int exact_begin(rvb_ctx * ctx, uint64_t nbins, uint64_t lists, ExactList & in)
{
    const IrCounts count = ir_counts(ctx);
    in.nbins = nbins;
    in.ndiffuse = count.ndiffuse;
    in.nimages = count.nimages;
    in.n = in.ndiffuse + in.nimages;
    if (in.n >= (1ull << 31)) return fail(ctx, RVB_ERR_CAPACITY, "rvb_ir_accumulate: too many impulses for exact mode");
    if (nbins >= 0x7FFFFFF0ull) return fail(ctx, RVB_ERR_CAPACITY, "rvb_ir_accumulate: too many bins for exact mode");
    in.listed = in.n;
    return ensure_sort_buffers(ctx, lists * in.n);
}

// The live list (exact_kernels.hip) in keys_a / vals_a: `in.listed` entries per ear — the trace's count of live diffuse impulses, which
// came down with the small block, and every image; all n where the count no longer holds (same launches, only the list is padded).
// The raw keys pass through keys_b, which the sort overwrites afterwards.
int live_list(rvb_ctx * ctx, ExactList & in, float predelay, float sample_rate, uint64_t nbins)
{
    in.compacted = true;
    in.count_valid = ctx->trace.live_count_holds();
    if (in.count_valid && in.ndiffuse) {
        const int rc = fetch_small(ctx);                // (the caller's rvb_ir_time_range or image merge has waited for it already)
        if (rc != RVB_OK) return rc;
        in.listed = std::min<uint64_t>(ctx->trace.live_count(), in.ndiffuse) + in.nimages;
    }
    RVB_HIP(fail, ctx, ctx->sort.live.ensure(rvb_live_scratch_bytes(in.n)));
    rvb_launch_live_list(ctx->ir.model, ir_diffuse(ctx), in.ndiffuse, ctx->ir.images.as<rvb_impulse>(), in.n, predelay, sample_rate, (uint32_t) nbins,
                         in.listed, ctx->sort.keys_b.as<uint32_t>(), ctx->sort.live.p, ctx->sort.keys_a.as<uint32_t>(), ctx->sort.vals_a.as<uint32_t>(),
                         &ctx->trace.host->live_overflow, ctx->stream);
    return RVB_OK;
}

// One channel's list: keys are bins, nbins itself marks "adds nothing" (key_bits_for(nbins) bits cover 0 .. nbins); sorted, with bin boundaries.
int exact_list(rvb_ctx * ctx, const ExactList & in, uint32_t channel, float predelay, float sample_rate, uint64_t nbins, bool may_sort_own)
{
    uint32_t * keys = ctx->sort.keys_a.as<uint32_t>(), * values = ctx->sort.vals_a.as<uint32_t>();
    rvb_launch_bin_keys(ctx->ir.model, channel, ir_diffuse(ctx), in.ndiffuse, 0, predelay, sample_rate, (uint32_t) nbins, keys, values, ctx->stream);
    rvb_launch_bin_keys(ctx->ir.model, channel, ctx->ir.images.as<rvb_impulse>(), in.nimages, in.ndiffuse, predelay, sample_rate, (uint32_t) nbins, keys, values, ctx->stream);
    return sort_and_bin(ctx, in.n, nbins, key_bits_for(nbins), may_sort_own);
}

// RVB_EXACT_COARSE=0, the measurement switch (tools/README.md): the speaker fold keeps the list ordered by bin and ordered_sum_kernel.
bool coarse_list_enabled()
{
    static const bool on = !(getenv("RVB_EXACT_COARSE") && std::strcmp(getenv("RVB_EXACT_COARSE"), "0") == 0);
    return on;
}

// Exact mode, step 1 (everything that does not depend on what the histogram holds): per-impulse bin keys, the radix sort, where each
// bin's run starts and ends.  Speaker channels keep the input time (kernel.cpp:530-533) and share ONE sorted list; the two HRTF ears
// shift the arrival time differently (kernel.cpp:616-622) and are keyed in one pass into ONE list of 2 n entries (bin_keys_hrtf_kernel).
int exact_prepare(rvb_ctx * ctx, float predelay, float sample_rate, uint64_t nbins)
{
    const AttenuationModel & m = ctx->ir.model;
    ExactList in;
    int rc = exact_begin(ctx, nbins, m.hrtf ? 2 : 1, in);
    if (rc != RVB_OK) return rc;
    if (m.hrtf) {
        // (explicit values — the two halves carry the same impulse numbers — and always rocPRIM's sort: RVB_SORT=own takes identity values only.
        // Values derived from the entry's position by a transform iterator instead of an array: 1.52 -> 1.58 ms, and 0.85 -> 0.88 ms for the
        // one-list speaker form; rocPRIM's first pass reads an array faster than it evaluates an iterator.)
        const uint64_t nkeys = 2 * (nbins + 1);
        if ((rc = live_list(ctx, in, predelay, sample_rate, nbins)) == RVB_OK) rc = sort_and_bin(ctx, 2 * in.listed, nkeys, key_bits_for(nkeys - 1), false);
    } else if (own_sort_enabled()) {
        rc = exact_list(ctx, in, 0, predelay, sample_rate, nbins, true);          // identity values: the list of every impulse
    } else {
        // up to 8 speakers: the fold works by coarse bin (ordered_sum_coarse_kernel) and the sort leaves the low key bits alone
        in.coarse_shift = m.nchannels <= 8 && coarse_list_enabled() ? RVB_COARSE_SHIFT : 0;
        if ((rc = live_list(ctx, in, predelay, sample_rate, nbins)) == RVB_OK)
            rc = sort_and_bin(ctx, in.listed, nbins, key_bits_for(nbins), false, in.coarse_shift);
    }
    if (rc != RVB_OK) return rc;
    RVB_HIP(fail, ctx, hipGetLastError());
    in.hrtf_combined = m.hrtf != 0;
    ctx->ir.exact_prepared(in);
    return RVB_OK;
}

// Exact mode, step 2: bins [b0, b1) — every bin's impulses added in impulse order ON TOP of what the histogram holds (rayverb.cpp:67-74).
int exact_fold(rvb_ctx * ctx, uint64_t b0, uint64_t b1, float * hist)
{
    const AttenuationModel & m = ctx->ir.model;
    const ExactList & e = ctx->ir.exact();
    if (!ctx->ir.prepared()) return fail(ctx, RVB_ERR_STATE, "rvb_ir_exact_fold: rvb_ir_exact_prepare first (and nothing that reuses the sort buffers in between)");
    if (b1 > e.nbins) b1 = e.nbins;
    if (e.hrtf_combined) {
        const uint64_t nkeys = 2 * (e.nbins + 1);
        rvb_launch_ordered_sum_hrtf(m, ir_diffuse(ctx), e.ndiffuse, ctx->ir.images.as<rvb_impulse>(), ctx->sort.vals_b.as<uint32_t>(),
                                    ctx->sort.bin_starts.as<uint32_t>(), ctx->sort.bin_starts.as<uint32_t>() + nkeys, e.nbins, hist, ctx->stream, b0, b1);
    } else if (m.nchannels > 8) {
        rvb_launch_ordered_sum_wide(m, ir_diffuse(ctx), e.ndiffuse, ctx->ir.images.as<rvb_impulse>(), ctx->sort.vals_b.as<uint32_t>(),
                                    ctx->sort.bin_starts.as<uint32_t>(), ctx->sort.bin_starts.as<uint32_t>() + e.nbins, e.listed, e.nbins, hist, ctx->stream, b0, b1);
    } else {
        const uint64_t nruns = coarse_keys(e.nbins, e.coarse_shift);
        rvb_launch_ordered_sum(m, 0, m.nchannels, ir_diffuse(ctx), e.ndiffuse, ctx->ir.images.as<rvb_impulse>(), ctx->sort.vals_b.as<uint32_t>(),
                               ctx->sort.bin_starts.as<uint32_t>(), ctx->sort.bin_starts.as<uint32_t>() + nruns, e.listed, e.nbins, hist, ctx->stream, b0, b1,
                               e.coarse_shift ? ctx->sort.keys_b.as<uint32_t>() : nullptr);
    }
    RVB_HIP(fail, ctx, hipGetLastError());
    return RVB_OK;
}

// RVB_HRTF_SPLIT_EARS=1, the measurement / test switch: a list per ear — keys, sorted list and bin boundaries, that ear's fold —, as
// in round 2; always rocPRIM's sort, as round 2 had it.  No list stays prepared.
int exact_split_ears(rvb_ctx * ctx, float predelay, float sample_rate, uint64_t nbins, float * hist)
{
    const AttenuationModel & m = ctx->ir.model;
    ExactList in;
    int rc = exact_begin(ctx, nbins, 1, in);
    for (uint32_t ch = 0; rc == RVB_OK && ch < m.nchannels; ++ch) {
        if ((rc = exact_list(ctx, in, ch, predelay, sample_rate, nbins, false)) != RVB_OK) break;
        rvb_launch_ordered_sum(m, ch, 1u, ir_diffuse(ctx), in.ndiffuse, ctx->ir.images.as<rvb_impulse>(), ctx->sort.vals_b.as<uint32_t>(),
                               ctx->sort.bin_starts.as<uint32_t>(), ctx->sort.bin_starts.as<uint32_t>() + nbins, in.n, nbins, hist, ctx->stream);
    }
    return rc;
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
// is busy while the later ranges are still being folded; the other forms copy the finished histogram in one piece.  A successful call
// voids a prepared list, whatever its mode and its nbins (include/rvb_capi.h, rvb_ir_exact_prepare).
int ir_accumulate_impl(rvb_ctx * ctx, float predelay, float sample_rate, uint64_t nbins, int mode, void * d_histogram,
                       float * pinned_dst, uint32_t slices)
{
    if (!ctx) return RVB_ERR_INVALID;
    if (!ctx->ir.configured()) return fail(ctx, RVB_ERR_STATE, "rvb_ir_accumulate: rvb_ir_configure_* first");
    if (!d_histogram || nbins == 0) return fail(ctx, RVB_ERR_INVALID, "rvb_ir_accumulate: null histogram or no bins");
    RVB_BIND(ctx);
    if (slices == 0) slices = 1;
    bool exported = false;
    const AttenuationModel & m = ctx->ir.model;
    const IrCounts count = ir_counts(ctx);
    float * hist = reinterpret_cast<float *>(d_histogram);
    ctx->reset_timings();
    // More than 8 speakers: RVB_IR_FAST runs the sorted fold too.  An atomic histogram adds 32 bytes per live impulse and channel at
    // the chip-wide float-atomic rate (about 6.5 ms for 32 channels at workload C2 before its transpose); the fold gathers each record
    // once for all channels and writes with plain stores (profiles/speaker_arrays_n1.txt).  Its sums are the exact mode's, which meet
    // the fast mode's bound trivially.
    const bool wide = !m.hrtf && m.nchannels > 8;
    if (mode == RVB_IR_FAST && !wide) {
        const size_t acc_bytes = (size_t) nbins * m.nchannels * 8 * sizeof(float);
        RVB_HIP(fail, ctx, ctx->ir.acc.ensure(acc_bytes));
        RVB_HIP(fail, ctx, hipMemsetAsync(ctx->ir.acc.p, 0, acc_bytes, ctx->stream));
        ctx->begin_timing("histogram_fast_kernel");
        rvb_launch_histogram_fast(m, ir_diffuse(ctx), count.ndiffuse, predelay, sample_rate, nbins, ctx->ir.acc.as<float>(), ctx->stream);
        rvb_launch_histogram_fast(m, ctx->ir.images.as<rvb_impulse>(), count.nimages, predelay, sample_rate, nbins, ctx->ir.acc.as<float>(), ctx->stream);
        ctx->end_timing();
        ctx->begin_timing("histogram_transpose_kernel");
        rvb_launch_histogram_transpose(ctx->ir.acc.as<float>(), hist, m.nchannels, nbins, ctx->stream);
        ctx->end_timing();
    } else if (mode == RVB_IR_EXACT || mode == RVB_IR_FAST) {
        const char * split_env = getenv("RVB_HRTF_SPLIT_EARS");     // (read per call)
        const bool split_ears = m.hrtf && split_env && split_env[0] == '1';
        ctx->begin_timing(mode == RVB_IR_FAST ? "sorted_fold_wide" : "exact_mode");
        if (split_ears) {
            const int rc = exact_split_ears(ctx, predelay, sample_rate, nbins, hist);
            if (rc != RVB_OK) return rc;
        } else {
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
        }
        ctx->end_timing();
    } else {
        return fail(ctx, RVB_ERR_INVALID, "rvb_ir_accumulate: unknown mode");
    }
    RVB_HIP(fail, ctx, hipGetLastError());
    const int rc = pinned_dst && !exported ? export_bin_range(ctx, pinned_dst, hist, (uint64_t) m.nchannels * 8, nbins, 0, nbins) : RVB_OK;
    if (rc == RVB_OK) ctx->ir.void_exact_list();
    return rc;
}

}  // namespace

extern "C" {

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
    if (!ctx->ir.configured()) return fail(ctx, RVB_ERR_STATE, "rvb_ir_time_range_begin: rvb_ir_configure_* first");
    RVB_BIND(ctx);
    if (!ctx->ir.model.hrtf) return RVB_OK;          // speakers: the range came with the trace (reduced inside the shadow kernel)
    return time_range_enqueue(ctx);
}

int rvb_ir_time_range(rvb_ctx * ctx, float * min_nonzero_time, float * max_time)
{
    if (!ctx) return RVB_ERR_INVALID;
    if (!ctx->ir.configured()) return fail(ctx, RVB_ERR_STATE, "rvb_ir_time_range: rvb_ir_configure_* first");
    RVB_BIND(ctx);
    uint32_t got[2] = {0xFFFFFFFFu, 0u};          // float bits: earliest non-zero time (all ones: none), latest time
    if (ctx->ir.model.hrtf) {
        if (!ctx->ir.range_pending()) {
            const int rc = time_range_enqueue(ctx);
            if (rc != RVB_OK) return rc;
        }
        ctx->ir.range_taken();
        // (the wait takes the trace's small block along where nothing has fetched it yet: the exact mode sizes its list from it)
        if (ctx->trace.fetched()) {
            RVB_HIP(fail, ctx, hipStreamSynchronize(ctx->stream));
        } else {
            const int rc = fetch_small(ctx);
            if (rc != RVB_OK) return rc;
        }
        std::memcpy(got, ctx->trace.host->hrtf_range, sizeof(got));
    } else {
        // Speaker channels keep the input time (kernel.cpp:530-533), so the range is that of the raw
        // impulses: the diffuse part was reduced inside shadow_kernel, the few images are scanned below.
        ctx->reset_timings();
        if (ctx->ir.which() & RVB_IR_DIFFUSE) {
            int rc = fetch_small(ctx);
            if (rc != RVB_OK) return rc;
            std::memcpy(got, ctx->trace.diffuse_range(), sizeof(got));
        }
    }
    float lo = 0.0f, hi = 0.0f;
    bool have_lo = got[0] != 0xFFFFFFFFu;
    if (have_lo) std::memcpy(&lo, &got[0], 4);
    std::memcpy(&hi, &got[1], 4);
    if (!ctx->ir.model.hrtf && (ctx->ir.which() & RVB_IR_IMAGES)) {
        const int rc = ir_images_on_host(ctx);                  // (a list gathered on the device comes down once)
        if (rc != RVB_OK) return rc;
        for (const rvb_impulse & im : ctx->ir.images_host) {
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
    return ir_accumulate_impl(ctx, predelay, sample_rate, nbins, mode, d_histogram, nullptr, 1);
}

int rvb_ir_accumulate_export(rvb_ctx * ctx, float predelay, float sample_rate, uint64_t nbins, int mode, void * d_histogram,
                             void * pinned_dst, uint32_t slices)
{
    if (ctx && !pinned_dst) return fail(ctx, RVB_ERR_INVALID, "rvb_ir_accumulate_export: null destination");
    // Default: ONE piece.  Measured at workload C2 (profiles/r04_export_slices_n1.txt): 1 / 2 / 4 / 8 bin ranges leave one impulse response
    // on the host after 6.98 / 7.04 / 7.02 / 7.00 ms (5.88 ms to HBM: the 54 MB need 1.1 ms of the link whenever they start, and the fold they
    // could overlap is 0.27 ms split into launches that cost what the overlap gains) and the pipeline at 4.82 / 4.81 / 4.80 / 4.96 ms per IR.
    return ir_accumulate_impl(ctx, predelay, sample_rate, nbins, mode, d_histogram, static_cast<float *>(pinned_dst), slices ? slices : 1u);
}

int rvb_ir_exact_prepare(rvb_ctx * ctx, float predelay, float sample_rate, uint64_t nbins)
{
    if (!ctx) return RVB_ERR_INVALID;
    if (!ctx->ir.configured()) return fail(ctx, RVB_ERR_STATE, "rvb_ir_exact_prepare: rvb_ir_configure_* first");
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
    if (!ctx->ir.prepared_for(nbins)) return fail(ctx, RVB_ERR_STATE, "rvb_ir_exact_fold: rvb_ir_exact_prepare with this nbins first");
    if (bin_begin > bin_end) return fail(ctx, RVB_ERR_INVALID, "rvb_ir_exact_fold: bin range");
    RVB_BIND(ctx);
    return exact_fold(ctx, bin_begin, bin_end, static_cast<float *>(d_histogram));
}

int rvb_ir_exact_list_info(rvb_ctx * ctx, uint64_t * listed, uint64_t * live_on_device, int * count_valid)
{
    if (!ctx) return RVB_ERR_INVALID;
    if (!ctx->ir.ever_listed()) return fail(ctx, RVB_ERR_STATE, "rvb_ir_exact_list_info: no exact-mode list has been made on this context");
    const ExactList & e = ctx->ir.exact();
    if (listed) *listed = e.listed;
    if (count_valid) *count_valid = e.count_valid ? 1 : 0;
    if (live_on_device) {
        uint32_t total = (uint32_t) e.listed;           // (the list of every impulse counts nothing)
        if (e.compacted && e.n) {
            RVB_BIND(ctx);
            RVB_HIP(fail, ctx, hipStreamSynchronize(ctx->stream));
            RVB_HIP(fail, ctx, hipMemcpy(&total, ctx->sort.live.p, sizeof(total), hipMemcpyDeviceToHost));       // LiveHeader::total
        }
        *live_on_device = total;
    }
    return RVB_OK;
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
    const size_t bytes = (size_t) bins * ctx->ir.model.nchannels * 8 * sizeof(float);
    RVB_HIP(fail, ctx, ctx->ir.hist.ensure(bytes));
    RVB_HIP(fail, ctx, hipMemsetAsync(ctx->ir.hist.p, 0, bytes, ctx->stream));
    rc = rvb_ir_accumulate(ctx, predelay, sample_rate, bins, mode, ctx->ir.hist.p);
    if (rc != RVB_OK) return rc;
    RVB_HIP(fail, ctx, hipMemcpyAsync(out, ctx->ir.hist.p, bytes, hipMemcpyDeviceToHost, ctx->stream));
    RVB_HIP(fail, ctx, hipStreamSynchronize(ctx->stream));
    return RVB_OK;
}

}  // extern "C"
