// kept_tiles.h — device code that the passes over a kept trace share (reshade_kernels.hip: path_keep_kernel and reshade_kernel,
// reshade_grad_kernels.hip: reshade_grad_kernel, relisten_kernels.hip: relisten_records_kernel): the side record and the listener record
// that path_keep_kernel leaves per (ray, bounce), the LDS layout of a wave that works through eight rays tile by tile of bounces
// (KeptRows, KeptTileLds: the kernels' pointers and the launchers' blocks and byte counts), the specular chain along a ray, and the
// two-lane read of a finished record.
#pragma once

#include "traversal.h"

namespace {

// ---- the side record: what the shadow stage destroys of a work record, 16 bytes per (ray, bounce) -------------------------------------
// {newDist, DIFF, surface of the triangle (NONE: the ray had already escaped), 0} as a float4: path_keep_kernel makes it, and a record
// staged in LDS is read through the same functions (reshade_grad_kernel stages {dist, DIFF, surface, bin}: words 1 and 2 as here).
struct SideRecord {
    static constexpr uint32_t SURFACE_WORD = 2u;
    static __device__ __forceinline__ float4 make(float new_dist, float diff, uint32_t surface) { return make_float4(new_dist, diff, __uint_as_float(surface), 0.0f); }
    // no record: the ray had escaped, or the slot lies past the last ray or bounce
    static __device__ __forceinline__ float4 none() { return make(0.0f, 0.0f, NONE); }
    static __device__ __forceinline__ float new_dist(const float4 & s) { return s.x; }
    static __device__ __forceinline__ float diff(const float4 & s) { return s.y; }
    static __device__ __forceinline__ uint32_t surface(const float4 & s) { return __float_as_uint(s.z); }
    // the surface alone of record i, a 4-byte read
    static __device__ __forceinline__ uint32_t surface_of(const float4 * kept, uint64_t i) { return reinterpret_cast<const uint32_t *>(kept + i)[SURFACE_WORD]; }
};

// The listener record (RVB_KEEP_LISTENER): the two words of a work record that nothing else recovers, 8 bytes per (ray, bounce):
// {own-plane threshold (float bits), triangle}; zeros where the ray had escaped.
typedef uint32_t nt_uint2 __attribute__((ext_vector_type(2)));
struct ListenRecord {
    nt_uint2 v;
    static __device__ __forceinline__ ListenRecord make(uint32_t threshold, uint32_t triangle) { return ListenRecord{nt_uint2{threshold, triangle}}; }
    static __device__ __forceinline__ ListenRecord load(const uint2 * listen, uint64_t i)
    {
        const uint2 l = listen[i];
        return make(l.x, l.y);
    }
    __device__ __forceinline__ void store(uint2 * listen, uint64_t i) const { __builtin_nontemporal_store(v, reinterpret_cast<nt_uint2 *>(listen + i)); }
    __device__ __forceinline__ uint32_t threshold() const { return v.x; }
    __device__ __forceinline__ uint32_t triangle() const { return v.y; }
};

// ---- LDS of a wave that takes RAYS rays and stages TILE bounces of each at a time ---------------------------------------------------------
// A region of staged records is [RAYS][ROW] records, a ray's row padded by one record: the eight rays' reads of one bounce fall into
// different banks.
template <uint32_t TILE>
struct KeptRows {
    static constexpr uint32_t RAYS = 8u;             // rays per wave: one lane per (ray, band) in the chain phases
    static constexpr uint32_t ROW = TILE + 1u;       // records per row
    static constexpr uint32_t RECORDS = RAYS * ROW;  // records per region
    static __host__ __device__ __forceinline__ uint64_t groups(uint64_t nrays) { return (nrays + RAYS - 1) / RAYS; }
    // record (ray r of the wave, bounce k of the tile) of a region, and the word of its surface in a region of 16-byte records
    static __device__ __forceinline__ uint32_t at(uint32_t r, uint32_t k) { return r * ROW + k; }
    static __device__ __forceinline__ uint32_t surface_word(uint32_t r, uint32_t k) { return at(r, k) * 4u + SideRecord::SURFACE_WORD; }
};

// The tile passes' whole layout, in words: a region of side records, the chain volumes [RAYS][ROW * 8] (vol_b(k) of the eight bands,
// padded alike), then the surface table (stage_surfaces).  The kernels take their pointers from it and the launchers their blocks and
// byte counts, so the two cannot drift apart.
template <uint32_t TILE>
struct KeptTileLds : KeptRows<TILE> {
    using Rows = KeptRows<TILE>;
    static constexpr uint32_t VOL_ROW = Rows::ROW * 8u;
    static constexpr uint32_t VOL_AT = Rows::RECORDS * 4u;
    static constexpr uint32_t SURFACES_AT = VOL_AT + Rows::RAYS * VOL_ROW;
    static __host__ __device__ __forceinline__ size_t bytes(uint32_t lds_surfaces) { return ((size_t) SURFACES_AT + 16u * lds_surfaces) * sizeof(uint32_t); }
    static __device__ __forceinline__ float4 * side(uint32_t * lds) { return reinterpret_cast<float4 *>(lds); }
    static __device__ __forceinline__ float * chain(uint32_t * lds) { return reinterpret_cast<float *>(lds + VOL_AT); }
    static __device__ __forceinline__ uint32_t * surfaces(uint32_t * lds) { return lds + SURFACES_AT; }
    // the eight chain volumes of record (r, k); lane h of a record's pair takes the four at + 4 h
    static __device__ __forceinline__ uint32_t vol_at(uint32_t r, uint32_t k) { return r * VOL_ROW + 8u * k; }
};

// ---- the chain: kernel.cpp:461 along a ray, one band per lane ----------------------------------------------------------------------------
// band `band` (0..7) of a surface's specular or diffuse row, from the staged table or from memory
__device__ __forceinline__ float band_of(const float4 v, const uint32_t e) { return e == 0 ? v.x : (e == 1 ? v.y : (e == 2 ? v.z : v.w)); }
template <bool SURF_LDS>
__device__ __forceinline__ float specular_band(const TraceArgs & a, const lds_float4_ptr surf_lds, const uint32_t surface, const uint32_t band)
{
    return band_of(surface_row<SURF_LDS>(a, surf_lds, surface, band >> 2), band & 3u);
}
template <bool SURF_LDS>
__device__ __forceinline__ float diffuse_band(const TraceArgs & a, const lds_float4_ptr surf_lds, const uint32_t surface, const uint32_t band)
{
    return band_of(surface_row<SURF_LDS>(a, surf_lds, surface, 2u + (band >> 2)), band & 3u);
}
// one bounce on `surface`: sequential along the ray, float products do not reassociate
template <bool SURF_LDS>
__device__ __forceinline__ float chain_step(const TraceArgs & a, const lds_float4_ptr surf_lds, const float vol, const uint32_t surface, const uint32_t band)
{
    return -vol * specular_band<SURF_LDS>(a, surf_lds, surface, band);
}

// ---- the two tile phases of reshade_kernel and relisten_records_kernel (called by the whole wave; the caller's barrier follows each) ----
// (1) the side records of bounces [first, first + TILE) of rays [ray0, ray0 + RAYS) to LDS, 16 bytes per lane, a ray's run of bounces
// contiguous; no record past the last ray or bounce
template <uint32_t TILE>
__device__ __forceinline__ void stage_side_records(const TraceArgs & a, const float4 * __restrict__ kept, const uint64_t ray0, const uint32_t first, float4 * side)
{
    using L = KeptRows<TILE>;
    for (uint32_t i = threadIdx.x; i < L::RAYS * TILE; i += WAVE) {
        const uint32_t r = i / TILE, k = i % TILE;
        float4 s = SideRecord::none();
        if (ray0 + r < a.nrays && first + k < a.nreflections)
            s = load_stream(kept + (ray0 + r) * a.nreflections + first + k);
        side[L::at(r, k)] = s;
    }
}
// (2) this lane's (ray, band) chain over the staged tile, vol_b(k) into `chain`.  `vol` and `alive` run on from tile to tile: an escape
// (or the end of the ray) ends the chain, there is no record from there on.  reshade_kernel's; relisten_records_kernel keeps the same
// loop written out, being slower through this function (profiles/kept_tiles_n1.txt).
// (unroll 1: unrolled, the 32 steps cost reshade_kernel twice its code, three more VGPRs and SGPRs spilled into VGPR lanes)
template <bool SURF_LDS, uint32_t TILE>
__device__ __forceinline__ void chain_over_tile(const TraceArgs & a, const lds_float4_ptr surf_lds, const uint32_t * side_words, float * chain, float & vol, bool & alive)
{
    using L = KeptTileLds<TILE>;
    const uint32_t r = threadIdx.x >> 3, band = threadIdx.x & 7u;
#pragma unroll 1
    for (uint32_t k = 0; k < TILE && alive; ++k) {
        const uint32_t surface = side_words[L::surface_word(r, k)];
        if (surface == NONE) {
            alive = false;
            break;
        }
        vol = chain_step<SURF_LDS>(a, surf_lds, vol, surface, band);
        chain[L::vol_at(r, k) + band] = vol;
    }
}

// ---- a finished record read by the two lanes of its pair: lane 0 the position chunk, lane 1 the time chunk (the final Impulse the shadow
// stage left), exchanged by DPP where a value is asked for.  `rec`: the record's first chunk; `inside` false reads nothing (zeros).
struct FinishedRecord {
    float4 aux;              // this lane's chunk
    static __device__ __forceinline__ FinishedRecord read(const float4 * rec, const bool inside, const uint32_t h)
    {
        FinishedRecord f = {make_float4(0, 0, 0, 0)};
        if (inside) f.aux = load_stream(rec + h + 2);
        return f;
    }
    __device__ __forceinline__ v3 position() const { return mk3(dpp_f<QP_PAIR_LO>(aux.x), dpp_f<QP_PAIR_LO>(aux.y), dpp_f<QP_PAIR_LO>(aux.z)); }
    // the shadow stage wrote time = seconds_per_meter() * dist for a visible record and 0 otherwise
    __device__ __forceinline__ float time() const { return dpp_f<QP_PAIR_HI>(aux.x); }
    // (both lanes of a pair hold the same side record, so the exchange behind the first test finds its partner lane)
    __device__ __forceinline__ bool visible(const float4 & side) const { return SideRecord::surface(side) != NONE && time() != 0.0f; }
};
// kernel.cpp:471 with :282-286: the path's length to the hit point `p` of the side record's bounce and on to the microphone
__device__ __forceinline__ float dist_to_mic(const float4 & side, const v3 p, const v3 mic) { return SideRecord::new_dist(side) + length3(mic - p); }

}  // namespace
