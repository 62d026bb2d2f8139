// wide_kernels.hip — the ordered per-bin summation for speaker layouts of more than 8 channels (up to RVB_MAX_SPEAKERS).
//
// The eight-channel kernels of stream_kernels.hip carry their speakers as kernel arguments (ModelDev) and fold at most four channels
// per launch, so a wider layout would gather every scattered 64-byte record once per four channels.  Here the speaker table sits in
// device memory (AttenuationModel::speaker_table: normalised direction + coefficient, 16 bytes per channel) and ONE launch folds all
// channels of a bin range:
//   * a workgroup owns WIDE_BINS = 32 consecutive bins, two lanes per bin as in ordered_sum_kernel (the even lane folds bands 0-3,
//     the odd lane bands 4-7), so every [channel][band] row is written in 128-byte runs;
//   * the workgroup's waves take NCH consecutive channels each and walk the SAME bins' lists at the same time: the first wave to ask
//     for a record brings it in from HBM, the others find it in the CU's L1 or the XCD's L2;
//   * what does not depend on the channel is evaluated once per record: the two normalisations of (pos - mic), with the operations
//     of speaker_gain on the same operands, and the non-zero test (made when the record was keyed: only live records are listed);
//   * a wave's table entries are wave-uniform and read through the scalar cache; the NCH x 4 sums per lane stay in registers.
// The sums are the left-to-right float sums in impulse order on top of what the histogram holds: bit for bit what
// ordered_sum_kernel<false, N> leaves in the same rows.
#include "kernels.h"
#include "rvb_math.h"

#define WIDE_BINS 32            // bins per workgroup = 64 lanes / 2
#define WIDE_UNROLL 4           // records per round: index loads, then record gathers, leave together (ordered_sum_kernel's SUM_UNROLL)
#define WIDE_MAX_WAVES 4        // waves per workgroup: ceil(RVB_MAX_SPEAKERS / 16), and wide_channels_per_wave never asks for more

namespace {

template <int NCH>
__global__ __launch_bounds__(64 * WIDE_MAX_WAVES) void ordered_sum_wide_kernel(v3 mic, const float4 * __restrict__ speakers, uint32_t nchannels,
                                                                               const rvb_impulse * __restrict__ diffuse, uint64_t ndiffuse,
                                                                               const rvb_impulse * __restrict__ images,
                                                                               const uint32_t * __restrict__ values,
                                                                               const uint32_t * __restrict__ starts, const uint32_t * __restrict__ ends,
                                                                               uint64_t nbins, uint64_t bin_begin, uint64_t bin_end, float * __restrict__ hist)
{
    // channels [c0, c0 + NCH) of this wave; those at or past nchannels (the last wave's tail) are computed on a copy of the last
    // speaker and never loaded or stored
    const uint32_t c0 = (uint32_t) __builtin_amdgcn_readfirstlane((int) (threadIdx.x >> 6)) * NCH;
    const uint32_t lane = threadIdx.x & 63u;
    const uint32_t half = lane & 1u;
    const uint64_t bin = bin_begin + (uint64_t) blockIdx.x * WIDE_BINS + (lane >> 1);
    if (bin >= bin_end)
        return;
    const uint64_t lo = starts[bin];
    if (lo == 0xFFFFFFFFull)
        return;                               // nothing lands in this bin: the histogram keeps what it holds
    const uint64_t hi = ends[bin];
    float4 spk[NCH];
    float sum[NCH][4];
#pragma unroll
    for (int c = 0; c < NCH; ++c) {
        const uint32_t ch = c0 + c < nchannels ? c0 + c : nchannels - 1;
        spk[c] = speakers[ch];
#pragma unroll
        for (int b = 0; b < 4; ++b)
            sum[c][b] = c0 + c < nchannels ? hist[((uint64_t) (c0 + c) * 8 + half * 4 + b) * nbins + bin] : 0.0f;
    }
    for (uint64_t k = lo; k < hi; k += WIDE_UNROLL) {
        float4 v[WIDE_UNROLL], p[WIDE_UNROLL];
#pragma unroll
        for (int u = 0; u < WIDE_UNROLL; ++u) {
            const uint64_t kk = k + u < hi ? k + u : lo;
            const uint64_t idx = values[kk];
            const rvb_impulse * imp = idx < ndiffuse ? diffuse + idx : images + (idx - ndiffuse);
            const float4 * r = reinterpret_cast<const float4 *>(imp);
            v[u] = r[half];
            p[u] = r[2];
        }
#pragma unroll
        for (int u = 0; u < WIDE_UNROLL; ++u) {
            if (k + u >= hi) break;
            const float vol[4] = {v[u].x, v[u].y, v[u].z, v[u].w};
            // reference kernel.cpp:528 getDirection, then :511 normalises the unit vector again — once per record, not per channel
            const v3 direction = normalize3(mk3(p[u].x, p[u].y, p[u].z) - mic);
            const v3 unit = normalize3(direction);
#pragma unroll
            for (int c = 0; c < NCH; ++c) {
                const float g = (1 - spk[c].w) + spk[c].w * dot3(unit, mk3(spk[c].x, spk[c].y, spk[c].z));
#pragma unroll
                for (int b = 0; b < 4; ++b) sum[c][b] += vol[b] * g;
            }
        }
    }
#pragma unroll
    for (int c = 0; c < NCH; ++c) {
        if (c0 + c < nchannels) {
#pragma unroll
            for (int b = 0; b < 4; ++b)
                hist[((uint64_t) (c0 + c) * 8 + half * 4 + b) * nbins + bin] = sum[c][b];
        }
    }
}

// Channels per wave: 12 where that needs no more waves than 16 would (9-12, 17-24, 33-36 channels: fewer idle channel slots in the
// last wave, 2-6 % faster at workload C2), else 16.  A fifth wave costs far more than idle slots do: 56 channels as 5 x 12 took 2.34 ms,
// as 4 x 16 1.70 ms (profiles/speaker_arrays_n1.txt).
uint32_t wide_channels_per_wave(uint32_t nchannels)
{
    return (nchannels + 11) / 12 <= (nchannels + 15) / 16 ? 12u : 16u;
}

}  // namespace

void rvb_make_speaker_table(const rvb_speaker * speakers, uint64_t nspeakers, float4 * table)
{
    for (uint64_t i = 0; i < nspeakers; ++i) {
        // (make_model's operations: the eight-channel kernels get the same bits as kernel arguments)
        const v3 d = normalize3(mk3(speakers[i].direction[0], speakers[i].direction[1], speakers[i].direction[2]));
        table[i] = make_float4(d.x, d.y, d.z, speakers[i].coefficient);
    }
}

void rvb_launch_ordered_sum_wide(const AttenuationModel & m, const rvb_impulse * diffuse, uint64_t ndiffuse, const rvb_impulse * images,
                                 const uint32_t * sorted_values, const uint32_t * starts, const uint32_t * ends, uint64_t n,
                                 uint64_t nbins, float * hist, hipStream_t s, uint64_t bin_begin, uint64_t bin_end)
{
    if (bin_end > nbins) bin_end = nbins;
    if (nbins == 0 || n == 0 || bin_begin >= bin_end || m.nchannels == 0 || !m.speaker_table) return;
    const uint32_t per_wave = wide_channels_per_wave(m.nchannels);
    const uint32_t waves = (m.nchannels + per_wave - 1) / per_wave;        // <= WIDE_MAX_WAVES for nchannels <= RVB_MAX_SPEAKERS
    const dim3 grid((unsigned) ((bin_end - bin_begin + WIDE_BINS - 1) / WIDE_BINS)), block(64 * waves);
    const v3 mic = mk3(m.mic[0], m.mic[1], m.mic[2]);
    if (per_wave == 12)
        hipLaunchKernelGGL(ordered_sum_wide_kernel<12>, grid, block, 0, s, mic, m.speaker_table, m.nchannels, diffuse, ndiffuse, images,
                           sorted_values, starts, ends, nbins, bin_begin, bin_end, hist);
    else
        hipLaunchKernelGGL(ordered_sum_wide_kernel<16>, grid, block, 0, s, mic, m.speaker_table, m.nchannels, diffuse, ndiffuse, images,
                           sorted_values, starts, ends, nbins, bin_begin, bin_end, hist);
}
