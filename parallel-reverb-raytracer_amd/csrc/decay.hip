// decay.hip — the decay calls of include/rvb_capi.h (rvb_decay_curve, rvb_decay_times, rvb_decay_loss, rvb_decay_params,
// rvb_decay_params_loss): arguments, scratch, launches and timings.  The kernels are csrc/decay_kernels.hip and
// csrc/decay_params_kernels.hip.  The calls work on the caller's device arrays and use of the context its device,
// stream, timings and ctx->decay_scratch only: no scene, trace or IR state is read or changed.
#include "ctx.h"

#include <cstring>

namespace {

const uint64_t kMaxRows = 4096;

struct DecayScratch {
    double * tiles;         // [4][nrows][ntiles] (curve, times: one plane; loss: three; params: four)
    uint32_t * first;       // [5][nrows][ntiles] (times: two planes; params: five)
    double * loss_rows;     // [nrows]
    uint2 * window;         // [nrows]
    float * seconds;        // [nrows]
    // rvb_decay_params / rvb_decay_params_loss
    double * params_loss;   // [nrows]
    float * params;         // [nrows][7], directly behind params_loss: one download for both
    uint32_t * params_window; // [nrows][5]
    float * targets;        // [nrows][7] targets, then [nrows][7] param_weights: one upload
    DecayParamsRow * rows;  // [nrows]
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

// one block for all calls (a call of another kind with the same shape finds it large enough)
int scratch_for(rvb_ctx * ctx, uint64_t nrows, uint64_t nbins, DecayScratch * s)
{
    const size_t plane = (size_t) nrows * rvb_decay_tiles(nbins);
    const size_t tiles_bytes = 4 * plane * sizeof(double), first_bytes = (5 * plane * sizeof(uint32_t) + 15) & ~(size_t) 15;
    const size_t rows_bytes = (size_t) nrows * sizeof(double);
    const size_t table_bytes = (size_t) nrows * RVB_DECAY_NPARAMS * sizeof(float);
    const size_t tables_bytes = (3 * table_bytes + 15) & ~(size_t) 15;                      // params, targets, param_weights
    const size_t window_bytes = ((size_t) nrows * 5 * sizeof(uint32_t) + 15) & ~(size_t) 15;
    const size_t params_at = tiles_bytes + first_bytes + 3 * rows_bytes;
    RVB_HIP(fail, ctx, ctx->decay_scratch.ensure(params_at + rows_bytes + tables_bytes + window_bytes + (size_t) nrows * sizeof(DecayParamsRow)));
    char * p = ctx->decay_scratch.as<char>();
    s->tiles = reinterpret_cast<double *>(p);
    s->first = reinterpret_cast<uint32_t *>(p + tiles_bytes);
    s->loss_rows = reinterpret_cast<double *>(p + tiles_bytes + first_bytes);
    s->window = reinterpret_cast<uint2 *>(p + tiles_bytes + first_bytes + rows_bytes);
    s->seconds = reinterpret_cast<float *>(p + tiles_bytes + first_bytes + 2 * rows_bytes);
    s->params_loss = reinterpret_cast<double *>(p + params_at);
    s->params = reinterpret_cast<float *>(p + params_at + rows_bytes);
    s->targets = reinterpret_cast<float *>(p + params_at + rows_bytes + table_bytes);
    s->params_window = reinterpret_cast<uint32_t *>(p + params_at + rows_bytes + tables_bytes);
    s->rows = reinterpret_cast<DecayParamsRow *>(p + params_at + rows_bytes + tables_bytes + window_bytes);
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

namespace {

// the bin of `seconds` at the sample rate, (uint64_t) (seconds * fs + 0.5); 0xFFFFFFFF where it lies behind the row's end
uint32_t bin_of(double seconds, double sample_rate, uint64_t nbins)
{
    const double x = seconds * sample_rate + 0.5;
    return x < (double) nbins ? (uint32_t) (uint64_t) x : 0xFFFFFFFFu;
}

// Both params calls: targets == nullptr is rvb_decay_params (no loss, no weights).  The arguments have been checked.
int decay_params(rvb_ctx * ctx, const float * h, const float * e, uint64_t nrows, uint64_t nbins, float sample_rate, const float * targets,
                 const float * param_weights, double * loss_rows, float * params, float * d_weights)
{
    RVB_BIND(ctx);
    DecayScratch s;
    int rc = scratch_for(ctx, nrows, nbins, &s);
    if (rc != RVB_OK) return rc;
    const size_t table = (size_t) nrows * RVB_DECAY_NPARAMS;
    if (targets) {
        std::vector<float> tables(2 * table);
        std::memcpy(tables.data(), targets, table * sizeof(float));
        std::memcpy(tables.data() + table, param_weights, table * sizeof(float));
        if ((rc = rvb_copy_to_device(ctx, s.targets, tables.data(), 2 * table * sizeof(float))) != RVB_OK) return rc;
    }
    DecayParamsRatios ratios;
    const float levels[5] = {0.0f, -10.0f, -5.0f, -25.0f, -35.0f};          // as rvb_decay_times takes them
    for (int i = 0; i < 5; ++i) ratios.r[i] = std::pow(10.0, (double) levels[i] / 10.0);
    const double fs = (double) sample_rate;
    ctx->reset_timings();
    ctx->begin_timing("decay_params_find_kernel");
    rvb_launch_decay_params_find(e, nrows, nbins, ratios, s.first, ctx->stream);
    ctx->end_timing();
    ctx->begin_timing("decay_params_window_kernel");
    rvb_launch_decay_params_window(s.first, nrows, nbins, s.params_window, ctx->stream);
    ctx->end_timing();
    ctx->begin_timing("decay_params_sums_kernel");
    rvb_launch_decay_params_sums(e, nrows, nbins, s.params_window, s.tiles, ctx->stream);
    ctx->end_timing();
    ctx->begin_timing("decay_params_fit_kernel");
    rvb_launch_decay_params_fit(e, nrows, nbins, s.params_window, s.tiles, fs, bin_of(0.05, fs, nbins), bin_of(0.08, fs, nbins),
                                targets ? s.targets : nullptr, targets ? s.targets + table : nullptr, s.params, s.rows, s.params_loss, ctx->stream);
    ctx->end_timing();
    if (d_weights) {
        ctx->begin_timing("decay_params_adjoint_sums_kernel");
        rvb_launch_decay_params_adjoint_sums(e, nrows, nbins, s.rows, s.tiles, ctx->stream);
        ctx->end_timing();
        ctx->begin_timing("decay_params_adjoint_carry_kernel");
        rvb_launch_decay_params_adjoint_carry(nrows, nbins, s.tiles, ctx->stream);
        ctx->end_timing();
        ctx->begin_timing("decay_params_adjoint_scan_kernel");
        rvb_launch_decay_params_adjoint_scan(h, e, nrows, nbins, s.rows, s.tiles, d_weights, ctx->stream);
        ctx->end_timing();
    }
    RVB_HIP(fail, ctx, hipGetLastError());
    RVB_HIP(fail, ctx, hipStreamSynchronize(ctx->stream));
    // the losses and, directly behind them, the parameters
    std::vector<double> host(nrows + (table * sizeof(float) + sizeof(double) - 1) / sizeof(double));
    if ((rc = rvb_copy_to_host(ctx, host.data(), s.params_loss, nrows * sizeof(double) + table * sizeof(float))) != RVB_OK) return rc;
    if (loss_rows) std::memcpy(loss_rows, host.data(), nrows * sizeof(double));
    if (params) std::memcpy(params, host.data() + nrows, table * sizeof(float));
    return RVB_OK;
}

} // namespace

extern "C" {

int rvb_decay_params(rvb_ctx * ctx, const void * d_curve, uint64_t nrows, uint64_t nbins, float sample_rate, float * params)
{
    if (!ctx) return RVB_ERR_INVALID;
    if (!d_curve || !params) return fail(ctx, RVB_ERR_INVALID, "rvb_decay_params: null curve or null output");
    const int rc = check_shape(ctx, "rvb_decay_params", nrows, nbins);
    if (rc != RVB_OK) return rc;
    if (!std::isfinite(sample_rate) || !(sample_rate > 0.0f)) return fail(ctx, RVB_ERR_INVALID, "rvb_decay_params: the sample rate is not a positive finite number");
    return decay_params(ctx, nullptr, reinterpret_cast<const float *>(d_curve), nrows, nbins, sample_rate, nullptr, nullptr, nullptr, params, nullptr);
}

int rvb_decay_params_loss(rvb_ctx * ctx, const void * d_histogram, const void * d_curve, uint64_t nrows, uint64_t nbins, float sample_rate,
                          const float * targets, const float * param_weights, double * loss_rows, float * params, void * d_weights)
{
    if (!ctx) return RVB_ERR_INVALID;
    if (!d_histogram || !d_curve || !targets || !param_weights || !loss_rows) return fail(ctx, RVB_ERR_INVALID, "rvb_decay_params_loss: null input or null output");
    const int rc = check_shape(ctx, "rvb_decay_params_loss", nrows, nbins);
    if (rc != RVB_OK) return rc;
    if (!std::isfinite(sample_rate) || !(sample_rate > 0.0f))
        return fail(ctx, RVB_ERR_INVALID, "rvb_decay_params_loss: the sample rate is not a positive finite number");
    for (uint64_t i = 0; i < nrows * RVB_DECAY_NPARAMS; ++i) {
        if (!std::isfinite(param_weights[i]) || param_weights[i] < 0.0f)
            return fail(ctx, RVB_ERR_INVALID, "rvb_decay_params_loss: a parameter weight is negative or not finite");
        if (param_weights[i] > 0.0f && !std::isfinite(targets[i]))
            return fail(ctx, RVB_ERR_INVALID, "rvb_decay_params_loss: a weighted target is not finite");
    }
    if (d_weights)
        for (const void * in : {d_histogram, d_curve})
            if (overlap(in, d_weights, nrows * nbins * sizeof(float))) return fail(ctx, RVB_ERR_INVALID, "rvb_decay_params_loss: the weights overlap an input");
    return decay_params(ctx, reinterpret_cast<const float *>(d_histogram), reinterpret_cast<const float *>(d_curve), nrows, nbins, sample_rate, targets,
                        param_weights, loss_rows, params, reinterpret_cast<float *>(d_weights));
}

} // extern "C"
