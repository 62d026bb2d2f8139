// reshade_kernels.hip — re-shading a finished trace (rvb_keep_paths / rvb_reshade of include/rvb_capi.h): new surfaces and a new air
// coefficient without the path stage, the record grouping and the shadow rays.  No reference counterpart for the stage; its arithmetic is
// the three places of reference rayverb/kernel.cpp where surfaces and air enter: :461 (the specular chain), :480-485 (the diffuse
// product) and :260 (add_image), with the functions the trace itself uses (traversal.h, rvb_math.h).
//   path_keep_kernel        between the path and the shadow stage: the three numbers of a work record that the shadow stage destroys
//                           (newDist, DIFF, the surface of the triangle) as a 16-byte side record (SideRecord, kept_tiles.h).  A streaming pass.
//   reshade_kernel          a wave takes eight rays, tile by tile of RESHADE_TILE bounces (the layout: KeptTileLds, kept_tiles.h): the side
//                           records of the tile go to LDS; lane (ray, band) runs the sequential chain vol = -vol * specular over the tile
//                           into LDS; then the wave streams the tile's records two lanes per record, whole 16-byte chunks, each lane
//                           finishing the four bands of the volume chunk it stores (as shadow_pair_kernel does), and folds the time range.
//   reshade_images_kernel   the image-source candidates and the direct slot(s), one lane each: the chain over the ray's first bounces
//                           (TraceArgs::early), then make_image's product with the kept INIT_DIST.
#include "kept_tiles.h"
#include "attenuation.h"

#include <algorithm>

namespace {

// ---- path_keep_kernel: one lane per record ------------------------------------------------------------------------------------------
// reads chunk 3 (newDist, threshold, triangle, tag) and the last word of chunk 2 (DIFF) of the work record, 20 consecutive bytes
// LISTEN (RVB_KEEP_LISTENER): the own-plane threshold, fmaf(skip_b, t, skip_a) with the segment length t, and the triangle as a
// ListenRecord of their own for relisten_records_kernel (relisten_kernels.hip)
template <bool LISTEN>
__global__ __launch_bounds__(256) void path_keep_kernel(const float4 * __restrict__ records, const uint64_t nrecords, const TriShade * __restrict__ shade,
                                                        float4 * __restrict__ kept, uint2 * __restrict__ listen)
{
    const uint64_t g = (uint64_t) blockIdx.x * blockDim.x + threadIdx.x;
    if (g >= nrecords)
        return;
    const float4 tail = load_stream(records + 4 * g + 3);
    float4 o = SideRecord::none();                     // tag 0: the ray had already escaped
    ListenRecord l = ListenRecord::make(0u, 0u);
    if (__float_as_uint(tail.w) != 0u) {
        const float diff = __builtin_nontemporal_load(reinterpret_cast<const float *>(records + 4 * g + 2) + 3);
        const uint32_t surface = shade[__float_as_uint(tail.z)].surface;
        o = SideRecord::make(tail.x, diff, surface);
        l = ListenRecord::make(__float_as_uint(tail.y), __float_as_uint(tail.z));
    }
    store_stream(kept + g, o);
    if (LISTEN) l.store(listen, g);
}

// ---- reshade_kernel -------------------------------------------------------------------------------------------------------------------
#define RESHADE_TILE 32u             // bounces per tile
#define RESHADE_MAX_LDS_SURFACES 64u
typedef KeptTileLds<RESHADE_TILE> ReshadeLds;

template <bool SURF_LDS>
__global__ __launch_bounds__(WAVE) void reshade_kernel(TraceArgs a, const float4 * __restrict__ kept)
{
    typedef ReshadeLds L;
    extern __shared__ __attribute__((aligned(16))) uint32_t lds[];
    float4 * side = L::side(lds);
    float * chain = L::chain(lds);
    const lds_float4_ptr surf_lds = stage_surfaces(a, L::surfaces(lds));
    const uint32_t lane = threadIdx.x, h = lane & 1u;
    const uint64_t ray0 = (uint64_t) blockIdx.x * L::RAYS;
    const float air0 = a.air[4 * h], air1 = a.air[4 * h + 1], air2 = a.air[4 * h + 2], air3 = a.air[4 * h + 3];
    v3 mic = ld3(a.mic);
    float vol = 1.0f;                                        // vol_b(-1) of this lane's (ray, band)
    bool alive = true;
    float tmin = __builtin_inff(), tmax_seen = 0.0f;
    for (uint32_t first = 0; first < a.nreflections; first += RESHADE_TILE) {
        stage_side_records<RESHADE_TILE>(a, kept, ray0, first, side);                     // (1)
        __syncthreads();
        chain_over_tile<SURF_LDS, RESHADE_TILE>(a, surf_lds, lds, chain, vol, alive);     // (2) kernel.cpp:461 along the ray
        __syncthreads();
        // (3) kernel.cpp:471-490 for the tile's records, two lanes per record: lane h stores volume chunk h
        for (uint32_t j = lane >> 1; j < L::RAYS * RESHADE_TILE; j += WAVE / 2) {
            const uint32_t r = j / RESHADE_TILE, k = j % RESHADE_TILE;
            const uint64_t ray = ray0 + r;
            const bool inside = ray < a.nrays && first + k < a.nreflections;
            float4 * rec = reinterpret_cast<float4 *>(a.impulses + (inside ? ray * a.nreflections + first + k : 0));
            const FinishedRecord fin = FinishedRecord::read(rec, inside, h);          // (neither chunk changes)
            const float4 sd = side[L::at(r, k)];
            const v3 p = fin.position();
            const bool visible = fin.visible(sd);
            uint32_t pair = 0;
            if (a.npairs > 1) {
                pair = (uint32_t) ((inside ? ray : 0) / a.rays_per_pair);
                const float4 m4 = a.pair_mics[pair];
                mic = mk3(m4.x, m4.y, m4.z);
            }
            const float reach = dist_to_mic(sd, p, mic);            // (for every record: inside the select it costs reshade_kernel<false> two VGPRs)
            const float dist = visible ? reach : 0.0f;
            const float diff = SideRecord::diff(sd);
            float4 o = make_float4(0, 0, 0, 0);
            if (visible) {
                const float4 dc = surface_row<SURF_LDS>(a, surf_lds, SideRecord::surface(sd), 2 + h);       // diffuse coefficients of this lane's four bands
                const float4 v = *reinterpret_cast<const float4 *>(chain + L::vol_at(r, k) + 4u * h);
                o.x = band_product(v.x, air_attenuation(dist, air0) * 1.0f, dc.x, diff);
                o.y = band_product(v.y, air_attenuation(dist, air1) * 1.0f, dc.y, diff);
                o.z = band_product(v.z, air_attenuation(dist, air2) * 1.0f, dc.z, diff);
                o.w = band_product(v.w, air_attenuation(dist, air3) * 1.0f, dc.w, diff);
            }
            // (slots of escaped rays get their zeros again: a source pattern may have left them as -0)
            if (inside) store_stream(rec + h, o);
            uint32_t nonzero = (o.x != 0.0f || o.y != 0.0f || o.z != 0.0f || o.w != 0.0f) ? 1u : 0u;
            nonzero |= dpp_u<QP_SWAP1>(nonzero);
            note_time(a, nonzero != 0u, h == 0, pair, seconds_per_meter() * dist, tmin, tmax_seen);      // kernel.cpp:489
        }
        __syncthreads();                                     // (the next tile overwrites what this one read)
    }
    time_range_of_wave(a, tmin, tmax_seen);
}

// ---- reshade_images_kernel: the candidates [0, *count) and the direct slot of every pair, one lane each --------------------------------
__global__ __launch_bounds__(256) void reshade_images_kernel(TraceArgs a)
{
    const uint32_t ncand = *a.candidate_count, ndirect = a.npairs > 1 ? a.npairs : 1u;
    const uint64_t total = (uint64_t) ncand + ndirect;
    const uint32_t per_ray = RVB_NUM_IMAGE_SOURCE - 1;
    for (uint64_t i = (uint64_t) blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (uint64_t) gridDim.x * blockDim.x) {
        rvb_impulse * imp;
        float volume[8] = {1, 1, 1, 1, 1, 1, 1, 1};
        float dist;
        if (i < ncand) {
            // make_image's input: the ray's volume BEFORE the surface of bounce slot - 1, the chain over bounces 0 .. slot - 2
            const rvb_image_candidate & cand = a.candidates[i];
            imp = &a.candidates[i].impulse;
            const uint32_t * early = a.early + (cand.ray - a.ray_offset) * per_ray;
            for (uint32_t k = 0; k + 1 < cand.slot; ++k) {
                const rvb_surface & s = a.scene.surfaces[a.scene.shade[early[k]].surface];
#pragma unroll
                for (int b = 0; b < 8; ++b) volume[b] = -volume[b] * s.specular[b];        // kernel.cpp:461
            }
            dist = a.image_dist[i];
        } else {
            imp = a.direct + (i - ncand);
            dist = a.image_dist[a.nrays * per_ray + (i - ncand)];
        }
#pragma unroll
        for (int b = 0; b < 8; ++b)      // kernel.cpp:260; a hidden direct path (negative distance) keeps its zeros
            imp->volume[b] = dist < 0.0f ? 0.0f : volume[b] * (air_attenuation(dist, a.air[b]) * 1.0f);
    }
}

}  // namespace

void rvb_launch_path_keep(const TraceArgs & a, float4 * kept, uint2 * listen, hipStream_t s)
{
    const uint64_t nrecords = a.nrays * (uint64_t) a.nreflections;
    if (nrecords == 0) return;
    hipLaunchKernelGGL(listen ? path_keep_kernel<true> : path_keep_kernel<false>, dim3(stream_blocks(nrecords, 256)), dim3(256), 0, s,
                       reinterpret_cast<const float4 *>(a.impulses), nrecords, a.scene.shade, kept, listen);
}

// the whole table when it is small enough to leave the tiles' LDS most of a CU (64 surfaces: 4 KiB beside 12.4 KiB of tiles)
uint32_t rvb_reshade_lds_surfaces(uint64_t nsurfaces) { return nsurfaces <= RESHADE_MAX_LDS_SURFACES ? (uint32_t) nsurfaces : 0u; }

void rvb_launch_reshade(const TraceArgs & a, const float4 * kept, hipStream_t s)
{
    if (a.nrays * (uint64_t) a.nreflections == 0) return;
    hipLaunchKernelGGL(a.lds_surfaces ? reshade_kernel<true> : reshade_kernel<false>, dim3((unsigned) ReshadeLds::groups(a.nrays)), dim3(WAVE),
                       ReshadeLds::bytes(a.lds_surfaces), s, a, kept);
}

void rvb_launch_reshade_images(const TraceArgs & a, hipStream_t s)
{
    // candidates: at most nrays * 9, in practice a few thousand; the count is on the device, so a fixed small grid strides over them
    const unsigned blocks = (unsigned) std::min<uint64_t>(std::max<uint64_t>((a.nrays * 9 + a.npairs + 255) / 256, 1), 64);
    hipLaunchKernelGGL(reshade_images_kernel, dim3(blocks), dim3(256), 0, s, a);
}
