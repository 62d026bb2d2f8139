// decay_tiles.h — device code that the decay kernels share (decay_kernels.hip: curve, times, loss; decay_params_kernels.hip: the room
// acoustic parameters and their adjoint): the tile shape, the loads and stores of a chunk, and the sums and scans whose order is fixed
// by (tile, chunk, bin) alone.
//
// A row of nbins floats is cut into tiles of RVB_DECAY_TILE = 4096 bins; rows run along gridDim.y, tiles along x.  A workgroup of 256
// lanes takes one tile as 1024 CHUNKS of 4 consecutive bins: lane t holds chunks i * 256 + t, i = 0..3, so that a wave's loads are 64
// consecutive 16-byte pieces (a row starts wherever r * nbins puts it, so the pieces are 4-byte aligned only; the hardware takes that).
// Per lane the bins of a chunk one after the other, chunks across a wave by a shuffle ladder, the 16 (i, wave) segments of a tile one
// after the other, tiles one after the other — never by which workgroup ran first.  All sums are binary64.
#pragma once

#include "kernels.h"

namespace {

constexpr uint32_t kTile = RVB_DECAY_TILE;
constexpr uint32_t kLanes = 256;                        // lanes of a tile's workgroup
constexpr uint32_t kChunks = 4;                         // chunks of 4 bins per lane
constexpr uint32_t kSegments = kChunks * (kLanes / 64); // (i, wave) runs of 64 chunks in a tile, in bin order
static_assert(kLanes * kChunks * 4 == kTile, "a tile is 256 lanes x 4 chunks x 4 bins");

typedef float float4u __attribute__((ext_vector_type(4), aligned(4)));      // 16 bytes in one access at a float's alignment

// first bin of chunk i of this lane within the row
__device__ inline uint64_t chunk_bin(uint32_t tile, uint32_t i) { return (uint64_t) tile * kTile + (uint64_t) (i * kLanes + threadIdx.x) * 4; }

// bins [bin, bin + 4) of a row; what lies behind the row's end reads as 0
__device__ inline float4 load4(const float * __restrict__ row, uint64_t bin, uint64_t nbins)
{
    if (bin + 4 <= nbins) {
        const float4u v = *reinterpret_cast<const float4u *>(row + bin);
        return make_float4(v.x, v.y, v.z, v.w);
    }
    float4 v = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
    if (bin < nbins) v.x = row[bin];
    if (bin + 1 < nbins) v.y = row[bin + 1];
    if (bin + 2 < nbins) v.z = row[bin + 2];
    return v;
}

__device__ inline void store4(float * __restrict__ row, uint64_t bin, uint64_t nbins, float4 v)
{
    if (bin + 4 <= nbins) {
        float4u o;
        o.x = v.x; o.y = v.y; o.z = v.z; o.w = v.w;
        *reinterpret_cast<float4u *>(row + bin) = o;
        return;
    }
    if (bin < nbins) row[bin] = v.x;
    if (bin + 1 < nbins) row[bin + 1] = v.y;
    if (bin + 2 < nbins) row[bin + 2] = v.z;
}

// Inclusive scan over the 64 lanes of a wave, towards higher lanes (REVERSE: towards lower lanes).
template <bool REVERSE>
__device__ inline double wave_scan(double v)
{
    const uint32_t lane = threadIdx.x & 63u;
#pragma unroll
    for (uint32_t d = 1; d < 64; d <<= 1) {
        const double o = REVERSE ? __shfl_down(v, d, 64) : __shfl_up(v, d, 64);
        const bool has = REVERSE ? lane + d < 64 : lane >= d;
        if (has) v = v + o;
    }
    return v;
}

// Scan of a tile's 1024 chunk values in chunk order (REVERSE: from the last chunk to the first).  In: v[i] = the value of chunk
// i * 256 + t.  Out: v[i] = the sum of all chunks BEFORE it in that order (exclusive); returns the tile's total.  `totals` is LDS,
// kSegments doubles.
template <bool REVERSE>
__device__ inline double tile_scan(double (&v)[kChunks], double * totals)
{
    const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
    double incl[kChunks];
#pragma unroll
    for (uint32_t i = 0; i < kChunks; ++i) {
        incl[i] = wave_scan<REVERSE>(v[i]);
        if (lane == (REVERSE ? 0u : 63u)) totals[i * (kLanes / 64) + wave] = incl[i];
    }
    __syncthreads();
    double running = 0.0, total = 0.0;
    double before[kChunks] = {0.0, 0.0, 0.0, 0.0};
    // the segments in scan order; this lane's segment i * 4 + wave picks up what ran before it
    for (uint32_t n = 0; n < kSegments; ++n) {
        const uint32_t s = REVERSE ? kSegments - 1 - n : n;
#pragma unroll
        for (uint32_t i = 0; i < kChunks; ++i)
            if (s == i * (kLanes / 64) + wave) before[i] = running;
        running = running + totals[s];
    }
    total = running;
#pragma unroll
    for (uint32_t i = 0; i < kChunks; ++i) {
        const double neighbour = REVERSE ? __shfl_down(incl[i], 1, 64) : __shfl_up(incl[i], 1, 64);
        const bool has = REVERSE ? lane < 63 : lane > 0;
        v[i] = has ? before[i] + neighbour : before[i];
    }
    return total;
}

// The tile's total alone, in the same order of segments (lanes inside a wave by the scan's ladder).
__device__ inline double tile_sum(const double (&v)[kChunks], double * totals)
{
    const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
#pragma unroll
    for (uint32_t i = 0; i < kChunks; ++i) {
        const double incl = wave_scan<false>(v[i]);
        if (lane == 63u) totals[i * (kLanes / 64) + wave] = incl;
    }
    __syncthreads();
    double total = 0.0;
    for (uint32_t s = 0; s < kSegments; ++s) total = total + totals[s];
    return total;
}

// One wave per row: values[row][0 .. ntiles) become, in place, the sum of the tiles BEFORE each in walking order (REVERSE: from the
// last tile to the first) on top of `start`; returns the row's total (without `start`) in every lane.
template <bool REVERSE>
__device__ inline double row_carry(double * __restrict__ values, uint32_t ntiles, double start)
{
    const uint32_t lane = threadIdx.x;
    double running = start, total = 0.0;
    for (uint32_t base = 0; base < ntiles; base += 64) {
        const uint32_t n = base + lane;                               // position in walking order
        const bool has = n < ntiles;
        const uint32_t t = has ? (REVERSE ? ntiles - 1 - n : n) : 0;
        const double v = has ? values[t] : 0.0;
        const double incl = wave_scan<false>(v);
        const double up = __shfl_up(incl, 1, 64);
        if (has) values[t] = lane ? running + up : running;
        const double all = __shfl(incl, 63, 64);
        running = running + all;
        total = total + all;
    }
    return total;
}

// A row's tile values added up by one wave: lane l takes tiles l, l + 64, ... one after the other, then the lanes by the ladder.
__device__ inline double row_sum(const double * __restrict__ values, uint32_t ntiles)
{
    double acc = 0.0;
    for (uint32_t t = threadIdx.x; t < ntiles; t += 64) acc = acc + values[t];
    return __shfl(wave_scan<false>(acc), 63, 64);
}

} // namespace
