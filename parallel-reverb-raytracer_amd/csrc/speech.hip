// speech.hip — the calls of include/rvb_capi_speech.h (rvb_mtf, rvb_mtf_adjoint, rvb_speech_index): arguments, scratch, launches and
// timings.  The kernels are csrc/speech_kernels.hip, the index's arithmetic csrc/speech_index.h.  The device calls work on the caller's
// device arrays and use of the context its device, stream, timings and ctx->speech_scratch only: no scene, trace or IR state is read
// or changed.
#include "ctx.h"
#include "speech_index.h"
#include "speech_kernels.h"

#include <cstring>

namespace {

const uint64_t kMaxRows = 4096;                 // as the decay calls
const double kTwoPi = 6.283185307179586476925286766559;

struct SpeechScratch {
    double * tiles;         // [1 + 2 nfreqs][nrows][ntiles]
    MtfRow * rows;          // [nrows]
    double * coeffs;        // [nrows][RVB_MTF_MAX_FREQS]
};

// what both device calls refuse before any device is touched; 0 on success, and then `freqs` is filled
int check_mtf(rvb_ctx * ctx, const char * call, const void * d_histogram, uint64_t nrows, uint64_t nbins, float sample_rate, const double * mod_freqs,
              uint64_t nfreqs, MtfFreqs * freqs)
{
    const std::string who(call);
    if (!d_histogram) return fail(ctx, RVB_ERR_INVALID, who + ": null histogram");
    if (!mod_freqs) return fail(ctx, RVB_ERR_INVALID, who + ": null modulation frequencies");
    if (nrows == 0 || nbins == 0) return fail(ctx, RVB_ERR_INVALID, who + ": no rows or no bins");
    if (nfreqs == 0) return fail(ctx, RVB_ERR_INVALID, who + ": no modulation frequencies");
    if (nfreqs > RVB_MTF_MAX_FREQS) return fail(ctx, RVB_ERR_INVALID, who + ": more than " RVB_STR(RVB_MTF_MAX_FREQS) " modulation frequencies");
    if (!std::isfinite(sample_rate) || !(sample_rate > 0.0f)) return fail(ctx, RVB_ERR_INVALID, who + ": the sample rate is not a positive finite number");
    const double fs = (double) sample_rate;
    for (uint64_t i = 0; i < nfreqs; ++i) {
        const double f = mod_freqs[i];
        if (!std::isfinite(f) || !(f > 0.0)) return fail(ctx, RVB_ERR_INVALID, who + ": modulation frequency " + std::to_string(i) + " is not a positive finite number");
        if (f >= 0.5 * fs) return fail(ctx, RVB_ERR_INVALID, who + ": modulation frequency " + std::to_string(i) + " is at or above half the sample rate");
    }
    if (nrows > kMaxRows) return fail(ctx, RVB_ERR_CAPACITY, who + ": more than 4096 rows");
    if (nbins >= 0xFFFFFFFFull) return fail(ctx, RVB_ERR_CAPACITY, who + ": more bins than 32-bit bin numbers reach");
    *freqs = MtfFreqs();
    freqs->n = (uint32_t) nfreqs;
    for (uint64_t i = 0; i < nfreqs; ++i) {
        freqs->q[i] = mod_freqs[i] / fs;
        freqs->step_cos[i] = std::cos(kTwoPi * freqs->q[i]);
        freqs->step_sin[i] = std::sin(kTwoPi * freqs->q[i]);
    }
    return RVB_OK;
}

int scratch_for(rvb_ctx * ctx, uint64_t nrows, uint64_t nbins, uint64_t nfreqs, SpeechScratch * s)
{
    const size_t tiles_bytes = (1 + 2 * (size_t) nfreqs) * nrows * rvb_decay_tiles(nbins) * sizeof(double);
    const size_t rows_bytes = (size_t) nrows * sizeof(MtfRow);
    RVB_HIP(fail, ctx, ctx->speech_scratch.ensure(tiles_bytes + rows_bytes + (size_t) nrows * RVB_MTF_MAX_FREQS * sizeof(double)));
    char * p = ctx->speech_scratch.as<char>();
    s->tiles = reinterpret_cast<double *>(p);
    s->rows = reinterpret_cast<MtfRow *>(p + tiles_bytes);
    s->coeffs = reinterpret_cast<double *>(p + tiles_bytes + rows_bytes);
    return RVB_OK;
}

bool overlap(const void * a, const void * b, uint64_t bytes)
{
    const uintptr_t x = reinterpret_cast<uintptr_t>(a), y = reinterpret_cast<uintptr_t>(b);
    return x < y + bytes && y < x + bytes;
}

// pass 1 of both calls: the tiles' sums, then the rows'
void enqueue_sums(rvb_ctx * ctx, const float * h, uint64_t nrows, uint64_t nbins, const MtfFreqs & freqs, const SpeechScratch & s, bool with_coeffs)
{
    ctx->reset_timings();
    ctx->begin_timing("mtf_sums_kernel");
    rvb_launch_mtf_sums(h, nrows, nbins, freqs, s.tiles, ctx->stream);
    ctx->end_timing();
    ctx->begin_timing("mtf_fold_kernel");
    rvb_launch_mtf_fold(nrows, nbins, freqs.n, s.tiles, with_coeffs ? s.coeffs : nullptr, s.rows, ctx->stream);
    ctx->end_timing();
}

} // namespace

extern "C" {

int rvb_mtf(rvb_ctx * ctx, const void * d_histogram, uint64_t nrows, uint64_t nbins, float sample_rate, const double * mod_freqs, uint64_t nfreqs,
            double * mtf, double * sums)
{
    if (!ctx) return RVB_ERR_INVALID;
    if (!mtf) return fail(ctx, RVB_ERR_INVALID, "rvb_mtf: null output");
    MtfFreqs freqs;
    int rc = check_mtf(ctx, "rvb_mtf", d_histogram, nrows, nbins, sample_rate, mod_freqs, nfreqs, &freqs);
    if (rc != RVB_OK) return rc;
    RVB_BIND(ctx);
    SpeechScratch s;
    if ((rc = scratch_for(ctx, nrows, nbins, nfreqs, &s)) != RVB_OK) return rc;
    enqueue_sums(ctx, reinterpret_cast<const float *>(d_histogram), nrows, nbins, freqs, s, false);
    RVB_HIP(fail, ctx, hipGetLastError());
    RVB_HIP(fail, ctx, hipStreamSynchronize(ctx->stream));
    std::vector<MtfRow> host(nrows);
    if ((rc = rvb_copy_to_host(ctx, host.data(), s.rows, nrows * sizeof(MtfRow))) != RVB_OK) return rc;
    for (uint64_t r = 0; r < nrows; ++r) {
        std::memcpy(mtf + r * nfreqs, host[r].m, nfreqs * sizeof(double));
        if (sums) std::memcpy(sums + r * (1 + 2 * nfreqs), host[r].sums, (1 + 2 * nfreqs) * sizeof(double));
    }
    return RVB_OK;
}

int rvb_mtf_adjoint(rvb_ctx * ctx, const void * d_histogram, uint64_t nrows, uint64_t nbins, float sample_rate, const double * mod_freqs,
                    uint64_t nfreqs, const double * coeffs, void * d_weights)
{
    if (!ctx) return RVB_ERR_INVALID;
    if (!coeffs || !d_weights) return fail(ctx, RVB_ERR_INVALID, "rvb_mtf_adjoint: null coefficients or null weights");
    MtfFreqs freqs;
    int rc = check_mtf(ctx, "rvb_mtf_adjoint", d_histogram, nrows, nbins, sample_rate, mod_freqs, nfreqs, &freqs);
    if (rc != RVB_OK) return rc;
    for (uint64_t i = 0; i < nrows * nfreqs; ++i)
        if (!std::isfinite(coeffs[i])) return fail(ctx, RVB_ERR_INVALID, "rvb_mtf_adjoint: a coefficient is not finite");
    if (overlap(d_histogram, d_weights, nrows * nbins * sizeof(float)))
        return fail(ctx, RVB_ERR_INVALID, "rvb_mtf_adjoint: the weights overlap the histogram");
    RVB_BIND(ctx);
    SpeechScratch s;
    if ((rc = scratch_for(ctx, nrows, nbins, nfreqs, &s)) != RVB_OK) return rc;
    std::vector<double> padded(nrows * RVB_MTF_MAX_FREQS, 0.0);
    for (uint64_t r = 0; r < nrows; ++r) std::memcpy(padded.data() + r * RVB_MTF_MAX_FREQS, coeffs + r * nfreqs, nfreqs * sizeof(double));
    if ((rc = rvb_copy_to_device(ctx, s.coeffs, padded.data(), padded.size() * sizeof(double))) != RVB_OK) return rc;
    const float * h = reinterpret_cast<const float *>(d_histogram);
    enqueue_sums(ctx, h, nrows, nbins, freqs, s, true);
    ctx->begin_timing("mtf_adjoint_kernel");
    rvb_launch_mtf_adjoint(h, nrows, nbins, freqs, s.rows, reinterpret_cast<float *>(d_weights), ctx->stream);
    ctx->end_timing();
    RVB_HIP(fail, ctx, hipGetLastError());
    RVB_HIP(fail, ctx, hipStreamSynchronize(ctx->stream));
    return RVB_OK;
}

int rvb_speech_index(const double * mtf, uint64_t nfreqs, const double * snr_db, const double * alpha, const double * beta, double * sti, double * mti,
                     double * d_sti_d_mtf)
{
    if (!mtf || !alpha || !beta || !sti) return RVB_ERR_INVALID;
    if (nfreqs == 0 || nfreqs > RVB_MTF_MAX_FREQS) return RVB_ERR_INVALID;
    *sti = speech_index::evaluate(mtf, nfreqs, snr_db, alpha, beta, mti, d_sti_d_mtf);
    return RVB_OK;
}

} // extern "C"
