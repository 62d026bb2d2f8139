// decay.hip — the decay calls of include/rvb_capi.h (rvb_decay_curve, rvb_decay_times, rvb_decay_loss): arguments, scratch, launches
// and timings.  The kernels are csrc/decay_kernels.hip.  The calls work on the caller's device arrays and use of the context its device,
// stream, timings and ctx->decay_scratch only: no scene, trace or IR state is read or changed.
#include "ctx.h"

#include <cstring>

namespace {

const uint64_t kMaxRows = 4096;

struct DecayScratch {
    double * tiles;         // [3][nrows][ntiles]
    uint32_t * first;       // [2][nrows][ntiles]
    double * loss_rows;     // [nrows]
    uint2 * window;         // [nrows]
    float * seconds;        // [nrows]
};

// rows, bins and the required pointers; 0 on success
int check_shape(rvb_ctx * ctx, const char * call, uint64_t nrows, uint64_t nbins)
{
    if (nrows == 0 || nbins == 0) return fail(ctx, RVB_ERR_INVALID, std::string(call) + ": no rows or no bins");
    if (nrows > kMaxRows) return fail(ctx, RVB_ERR_CAPACITY, std::string(call) + ": more than 4096 rows");
    if (nbins >= 0xFFFFFFFFull) return fail(ctx, RVB_ERR_CAPACITY, std::string(call) + ": more bins than 32-bit bin numbers reach");
    return RVB_OK;
}

bool overlap(const void * a, const void * b, uint64_t bytes)
{
    const uintptr_t x = reinterpret_cast<uintptr_t>(a), y = reinterpret_cast<uintptr_t>(b);
    return x < y + bytes && y < x + bytes;
}

// one block for all three calls (a call of another kind with the same shape finds it large enough)
int scratch_for(rvb_ctx * ctx, uint64_t nrows, uint64_t nbins, DecayScratch * s)
{
    const size_t plane = (size_t) nrows * rvb_decay_tiles(nbins);
    const size_t tiles_bytes = 3 * plane * sizeof(double), first_bytes = (2 * plane * sizeof(uint32_t) + 15) & ~(size_t) 15;
    const size_t rows_bytes = (size_t) nrows * sizeof(double);
    RVB_HIP(fail, ctx, ctx->decay_scratch.ensure(tiles_bytes + first_bytes + 3 * rows_bytes));
    char * p = ctx->decay_scratch.as<char>();
    s->tiles = reinterpret_cast<double *>(p);
    s->first = reinterpret_cast<uint32_t *>(p + tiles_bytes);
    s->loss_rows = reinterpret_cast<double *>(p + tiles_bytes + first_bytes);
    s->window = reinterpret_cast<uint2 *>(p + tiles_bytes + first_bytes + rows_bytes);
    s->seconds = reinterpret_cast<float *>(p + tiles_bytes + first_bytes + 2 * rows_bytes);
    return RVB_OK;
}

} // namespace

extern "C" {

int rvb_decay_curve(rvb_ctx * ctx, const void * d_histogram, uint64_t nrows, uint64_t nbins, void * d_curve)
{
    if (!ctx) return RVB_ERR_INVALID;
    if (!d_histogram || !d_curve) return fail(ctx, RVB_ERR_INVALID, "rvb_decay_curve: null histogram or null curve");
    int rc = check_shape(ctx, "rvb_decay_curve", nrows, nbins);
    if (rc != RVB_OK) return rc;
    if (overlap(d_histogram, d_curve, nrows * nbins * sizeof(float)))
        return fail(ctx, RVB_ERR_INVALID, "rvb_decay_curve: the curve overlaps the histogram");
    RVB_BIND(ctx);
    DecayScratch s;
    if ((rc = scratch_for(ctx, nrows, nbins, &s)) != RVB_OK) return rc;
    const float * h = reinterpret_cast<const float *>(d_histogram);
    ctx->reset_timings();
    ctx->begin_timing("decay_curve_sums_kernel");
    rvb_launch_decay_curve_sums(h, nrows, nbins, s.tiles, ctx->stream);
    ctx->end_timing();
    ctx->begin_timing("decay_curve_carry_kernel");
    rvb_launch_decay_curve_carry(nrows, nbins, s.tiles, ctx->stream);
    ctx->end_timing();
    ctx->begin_timing("decay_curve_scan_kernel");
    rvb_launch_decay_curve_scan(h, nrows, nbins, s.tiles, reinterpret_cast<float *>(d_curve), ctx->stream);
    ctx->end_timing();
    RVB_HIP(fail, ctx, hipGetLastError());
    return RVB_OK;
}

int rvb_decay_times(rvb_ctx * ctx, const void * d_curve, uint64_t nrows, uint64_t nbins, float sample_rate, float db_begin, float db_end,
                    float * seconds)
{
    if (!ctx) return RVB_ERR_INVALID;
    if (!d_curve || !seconds) return fail(ctx, RVB_ERR_INVALID, "rvb_decay_times: null curve or null output");
    int rc = check_shape(ctx, "rvb_decay_times", nrows, nbins);
    if (rc != RVB_OK) return rc;
    if (!std::isfinite(sample_rate) || !(sample_rate > 0.0f)) return fail(ctx, RVB_ERR_INVALID, "rvb_decay_times: the sample rate is not a positive finite number");
    if (!std::isfinite(db_begin) || !std::isfinite(db_end) || !(db_end < db_begin) || !(db_begin <= 0.0f))
        return fail(ctx, RVB_ERR_INVALID, "rvb_decay_times: the levels must be finite with db_end < db_begin <= 0");
    RVB_BIND(ctx);
    DecayScratch s;
    if ((rc = scratch_for(ctx, nrows, nbins, &s)) != RVB_OK) return rc;
    const float * e = reinterpret_cast<const float *>(d_curve);
    const double ratio_begin = std::pow(10.0, (double) db_begin / 10.0), ratio_end = std::pow(10.0, (double) db_end / 10.0);
    ctx->reset_timings();
    ctx->begin_timing("decay_times_find_kernel");
    rvb_launch_decay_times_find(e, nrows, nbins, ratio_begin, ratio_end, s.first, ctx->stream);
    ctx->end_timing();
    ctx->begin_timing("decay_times_window_kernel");
    rvb_launch_decay_times_window(s.first, nrows, nbins, s.window, ctx->stream);
    ctx->end_timing();
    ctx->begin_timing("decay_times_sums_kernel");
    rvb_launch_decay_times_sums(e, nrows, nbins, s.window, s.tiles, ctx->stream);
    ctx->end_timing();
    ctx->begin_timing("decay_times_fit_kernel");
    rvb_launch_decay_times_fit(e, nrows, nbins, s.window, s.tiles, (double) sample_rate, s.seconds, ctx->stream);
    ctx->end_timing();
    RVB_HIP(fail, ctx, hipGetLastError());
    RVB_HIP(fail, ctx, hipStreamSynchronize(ctx->stream));
    std::vector<float> host(nrows);
    if ((rc = rvb_copy_to_host(ctx, host.data(), s.seconds, nrows * sizeof(float))) != RVB_OK) return rc;
    std::memcpy(seconds, host.data(), nrows * sizeof(float));
    return RVB_OK;
}

int rvb_decay_loss(rvb_ctx * ctx, const void * d_histogram, const void * d_curve, const void * d_target, const void * d_mask, uint64_t nrows,
                   uint64_t nbins, unsigned flags, double * loss_rows, void * d_weights)
{
    if (!ctx) return RVB_ERR_INVALID;
    if (!d_histogram || !d_curve || !d_target || !d_mask || !loss_rows) return fail(ctx, RVB_ERR_INVALID, "rvb_decay_loss: null input or null output");
    if (flags & ~(unsigned) RVB_DECAY_NORMALISED) return fail(ctx, RVB_ERR_INVALID, "rvb_decay_loss: unknown flag");
    int rc = check_shape(ctx, "rvb_decay_loss", nrows, nbins);
    if (rc != RVB_OK) return rc;
    const uint64_t bytes = nrows * nbins * sizeof(float);
    if (d_weights)
        for (const void * in : {d_histogram, d_curve, d_target, d_mask})
            if (overlap(in, d_weights, bytes)) return fail(ctx, RVB_ERR_INVALID, "rvb_decay_loss: the weights overlap an input");
    RVB_BIND(ctx);
    DecayScratch s;
    if ((rc = scratch_for(ctx, nrows, nbins, &s)) != RVB_OK) return rc;
    const float * h = reinterpret_cast<const float *>(d_histogram), * e = reinterpret_cast<const float *>(d_curve);
    const float * t = reinterpret_cast<const float *>(d_target), * m = reinterpret_cast<const float *>(d_mask);
    const bool normalised = (flags & RVB_DECAY_NORMALISED) != 0;
    ctx->reset_timings();
    ctx->begin_timing("decay_loss_sums_kernel");
    rvb_launch_decay_loss_sums(e, t, m, nrows, nbins, normalised, s.tiles, ctx->stream);
    ctx->end_timing();
    ctx->begin_timing("decay_loss_carry_kernel");
    rvb_launch_decay_loss_carry(e, nrows, nbins, normalised, s.tiles, s.loss_rows, ctx->stream);
    ctx->end_timing();
    if (d_weights) {
        ctx->begin_timing("decay_loss_scan_kernel");
        rvb_launch_decay_loss_scan(h, e, t, m, nrows, nbins, normalised, s.tiles, reinterpret_cast<float *>(d_weights), ctx->stream);
        ctx->end_timing();
    }
    RVB_HIP(fail, ctx, hipGetLastError());
    RVB_HIP(fail, ctx, hipStreamSynchronize(ctx->stream));
    std::vector<double> host(nrows);
    if ((rc = rvb_copy_to_host(ctx, host.data(), s.loss_rows, nrows * sizeof(double))) != RVB_OK) return rc;
    std::memcpy(loss_rows, host.data(), nrows * sizeof(double));
    return RVB_OK;
}

} // extern "C"
