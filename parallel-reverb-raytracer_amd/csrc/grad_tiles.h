// grad_tiles.h — what the gradient sweeps over a kept trace share (reshade_grad_kernels.hip: reshade_grad_kernel, the material gradients;
// source_grad_kernels.hip: source_grad_rays_kernel, the source-end gradients): the tile shape on top of kept_tiles.h, the staging of a
// tile's records — what of a record does not depend on the band — and the weight gather of a lane: a record is read, its bin taken and
// u_k = sum_c w[c][b][bin_k] * gain_c(k) formed with the same operations on the same operands in both sweeps.  The constants are shared by
// both; the two functions are source_grad_rays_kernel's.  reshade_grad_kernel keeps the same two loops written out (its terms pass
// adds a sort entry per record inside the first): through these functions the compiler allocates its scalar registers differently, and its
// device code is held unchanged (as relisten_records_kernel keeps chain_over_tile's loop, kept_tiles.h).
#pragma once

#include "kept_tiles.h"
#include "attenuation.h"

namespace {

#define GRAD_TILE 16u                // bounces per tile
typedef KeptRows<GRAD_TILE> GradRows;    // eight rays per wave, a ray's row of staged records padded by one
#define GRAD_BIN_WORD 3u             // a staged record is the side record with dist for newDist and, in this word, the bin (NONE: adds nothing)
#define GRAD_GATHER 8u               // weight gathers of a lane in flight together
#define GRAD_STAGE_WORDS (GradRows::RECORDS * 4u)

// The records of bounces [first, first + GRAD_TILE) of rays [ray0, ray0 + RAYS) of the pair, two lanes per record (FinishedRecord), as
// reshade_kernel reads them: lane 0 of the pair leaves {dist, DIFF, surface, bin} in `side` (bin NONE for a record that is invisible or
// past the histogram), lane 1 the record's arrival direction at the microphone in `toward`.  No record past the last ray or bounce.
// Called by the whole wave; the caller's barrier follows.
__device__ __forceinline__ void stage_grad_records(const TraceArgs & a, const ModelDev & m, const ReshadeGradArgs & g, const float4 * __restrict__ kept,
                                                   const uint32_t ray0, const uint32_t first, const v3 mic, float4 * side, float4 * toward)
{
    const uint32_t lane = threadIdx.x, h = lane & 1u;
    for (uint32_t j = lane >> 1; j < GradRows::RAYS * GRAD_TILE; j += WAVE / 2) {
        const uint32_t rr = j / GRAD_TILE, k = j % GRAD_TILE;
        const bool inside = ray0 + rr < g.nrays && first + k < a.nreflections;
        const uint64_t record = inside ? (g.first_ray + ray0 + rr) * a.nreflections + first + k : 0;
        float4 sd = SideRecord::none();
        if (inside) sd = load_stream(kept + record);
        const FinishedRecord fin = FinishedRecord::read(reinterpret_cast<const float4 *>(a.impulses + record), inside, h);
        const v3 p = fin.position();
        const float time = fin.time();
        const bool visible = fin.visible(sd);
        const float dist = dist_to_mic(sd, p, mic);
        const uint32_t bin = time_bin(time, g.predelay, g.sample_rate);
        const bool adds = visible && bin < g.nbins;
        const v3 dir = arrival_direction(m, p);
        float4 staged = SideRecord::make(dist, SideRecord::diff(sd), SideRecord::surface(sd));
        staged.w = __uint_as_float(adds ? bin : NONE);
        if (h == 0) side[GradRows::at(rr, k)] = staged;
        else toward[GradRows::at(rr, k)] = make_float4(dir.x, dir.y, dir.z, 0.0f);
    }
}

// The weight gather, sum_c w[c][b][bin_k] * gain_c(k) of this lane's (ray, band) for the staged tile's records into us[k][lane]: channel by
// channel with GRAD_GATHER gathers of a channel in flight together (inside a chain every gather would be waited for alone).  A record that
// adds nothing reads bin 0 and its sum is not used.  weights: [bin][channel][band] (reshade_grad_weights_kernel).
__device__ __forceinline__ void gather_tile_weights(const ModelDev & m, const ReshadeGradArgs & g, const uint32_t * side_words, const float4 * toward, float * us)
{
    const uint32_t lane = threadIdx.x, r = lane >> 3, band = lane & 7u;
    const uint32_t nch = m.nchannels, cb = nch * 8u;
#pragma unroll 1
    for (uint32_t k0 = 0; k0 < GRAD_TILE; k0 += GRAD_GATHER) {
        float wsum[GRAD_GATHER];
#pragma unroll
        for (uint32_t k = 0; k < GRAD_GATHER; ++k) wsum[k] = 0.0f;
        for (uint32_t c = 0; c < nch; ++c) {
#pragma unroll
            for (uint32_t k = 0; k < GRAD_GATHER; ++k) {
                const uint32_t bin = side_words[(GradRows::at(r, k0) + k) * 4u + GRAD_BIN_WORD];       // (k added last: a constant offset of the read)
                const float4 t4 = toward[GradRows::at(r, k0) + k];
                const float w = g.weights[(uint64_t) (bin != NONE ? bin : 0u) * cb + c * 8u + band];
                wsum[k] += w * speaker_gain_toward(m, c, mk3(t4.x, t4.y, t4.z));
            }
        }
#pragma unroll
        for (uint32_t k = 0; k < GRAD_GATHER; ++k) us[(k0 + k) * WAVE + lane] = wsum[k];
    }
}

}  // namespace
