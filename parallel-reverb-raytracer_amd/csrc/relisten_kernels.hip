// relisten_kernels.hip — a new microphone on a finished trace (rvb_keep_paths with RVB_KEEP_LISTENER / rvb_relisten of include/rvb_capi.h):
// the work records of the path stage again, without the path stage.  No reference counterpart for the stage; in the reference's kernel
// the closest-hit / reflect chain (kernel.cpp:359-375, :459-461, :478, :492-501) never reads the microphone, which enters in the shadow
// ray (:463-490), the image-source validation (:379-457) and the direct path (:335-357) only.
//   relisten_records_kernel   a wave takes RELISTEN_RAYS rays, as reshade_kernel does (reshade_kernels.hip).  Tile by tile of RELISTEN_TILE
//                             bounces: the side records of the tile go to LDS; lane (ray, band) runs the sequential chain
//                             vol = -vol * specular over the tile into LDS; then the wave streams the tile's records two lanes per record,
//                             whole 16-byte chunks: lane 0 the volume chunk of bands 0-3 and (position, DIFF), lane 1 that of bands 4-7 and
//                             (newDist, threshold, triangle, pair + 1) — the layout of trace_kernels.hip, "Work record".  The position is
//                             the one the shadow stage left in the record; DIFF, newDist come from the side record, threshold and triangle
//                             from the listener record that path_keep_kernel wrote beside it.
// The shadow, image and source-pattern kernels then run on these records exactly as behind a path kernel.
#include "traversal.h"

namespace {

#define RELISTEN_RAYS 8u             // rays per wave: one lane per (ray, band) in the chain phase
#define RELISTEN_TILE 32u            // bounces per tile
// LDS of a wave, in words, laid out as reshade_kernel's: [RAYS][TILE + 1] side records (a row padded by one record), [RAYS][(TILE + 1) * 8]
// chain volumes (padded alike), then the surface table (stage_surfaces)
#define RELISTEN_SIDE_ROW ((RELISTEN_TILE + 1u) * 4u)
#define RELISTEN_VOL_ROW ((RELISTEN_TILE + 1u) * 8u)
#define RELISTEN_VOL_AT (RELISTEN_RAYS * RELISTEN_SIDE_ROW)
#define RELISTEN_SURFACES_AT (RELISTEN_VOL_AT + RELISTEN_RAYS * RELISTEN_VOL_ROW)

template <bool SURF_LDS>
__global__ __launch_bounds__(WAVE) void relisten_records_kernel(TraceArgs a, const float4 * __restrict__ kept, const uint2 * __restrict__ listen)
{
    extern __shared__ __attribute__((aligned(16))) uint32_t lds[];
    float4 * side = reinterpret_cast<float4 *>(lds);
    float * chain = reinterpret_cast<float *>(lds + RELISTEN_VOL_AT);
    const lds_float4_ptr surf_lds = stage_surfaces(a, lds + RELISTEN_SURFACES_AT);
    const uint32_t lane = threadIdx.x, h = lane & 1u;
    const uint64_t ray0 = (uint64_t) blockIdx.x * RELISTEN_RAYS;
    const uint32_t chain_ray = lane >> 3, band = lane & 7u;
    float vol = 1.0f;                                        // vol_b(-1) of this lane's (ray, band)
    bool alive = true;
    for (uint32_t first = 0; first < a.nreflections; first += RELISTEN_TILE) {
        // (1) the tile's side records, 16 bytes per lane, a ray's run of bounces contiguous
        for (uint32_t i = lane; i < RELISTEN_RAYS * RELISTEN_TILE; i += WAVE) {
            const uint32_t r = i / RELISTEN_TILE, k = i % RELISTEN_TILE;
            float4 s = make_float4(0.0f, 0.0f, __uint_as_float(NONE), 0.0f);
            if (ray0 + r < a.nrays && first + k < a.nreflections)
                s = load_stream(kept + (ray0 + r) * a.nreflections + first + k);
            side[r * (RELISTEN_TILE + 1u) + k] = s;
        }
        __syncthreads();
        // (2) kernel.cpp:461 along the ray, one band per lane: sequential, float products do not reassociate
        for (uint32_t k = 0; k < RELISTEN_TILE && alive; ++k) {
            const uint32_t surface = lds[chain_ray * RELISTEN_SIDE_ROW + 4u * k + 2u];
            if (surface == NONE) {                           // escaped (or past the last bounce): no record from here on
                alive = false;
                break;
            }
            const float4 sp = surface_row<SURF_LDS>(a, surf_lds, surface, band >> 2);
            const uint32_t e = band & 3u;
            const float s = e == 0 ? sp.x : (e == 1 ? sp.y : (e == 2 ? sp.z : sp.w));
            vol = -vol * s;
            chain[chain_ray * RELISTEN_VOL_ROW + 8u * k + band] = vol;
        }
        __syncthreads();
        // (3) the tile's work records, two lanes per record: lane h stores chunks h and h + 2
        for (uint32_t j = lane >> 1; j < RELISTEN_RAYS * RELISTEN_TILE; j += WAVE / 2) {
            const uint32_t r = j / RELISTEN_TILE, k = j % RELISTEN_TILE;
            const uint64_t ray = ray0 + r;
            if (!(ray < a.nrays && first + k < a.nreflections))
                continue;
            const uint64_t record = ray * a.nreflections + first + k;
            float4 * rec = reinterpret_cast<float4 *>(a.impulses + record);
            const float4 sd = side[r * (RELISTEN_TILE + 1u) + k];
            // a slot behind an escape: all 64 bytes zero, as the path stage leaves it (a source pattern may have left -0 in the volumes)
            float4 v = make_float4(0, 0, 0, 0), aux = v;
            if (__float_as_uint(sd.z) != NONE) {
                v = *reinterpret_cast<const float4 *>(chain + r * RELISTEN_VOL_ROW + 8u * k + 4u * h);
                if (h == 0) {
                    // the hit point: the shadow stage wrote it back for invisible records too, and nothing behind it changes it
                    const float4 p = load_stream(rec + 2);
                    aux = make_float4(p.x, p.y, p.z, sd.y);
                } else {
                    const uint2 l = listen[record];
                    const uint32_t pair = a.npairs > 1 ? (uint32_t) (ray / a.rays_per_pair) : 0u;
                    aux = make_float4(sd.x, __uint_as_float(l.x), __uint_as_float(l.y), __uint_as_float(pair + 1u));
                }
            }
            store_stream(rec + h, v);
            store_stream(rec + h + 2, aux);
        }
        __syncthreads();                                     // (the next tile overwrites what this one read)
    }
}

}  // namespace

void rvb_launch_relisten_records(const TraceArgs & a, const float4 * kept, const uint2 * listen, hipStream_t s)
{
    if (a.nrays * (uint64_t) a.nreflections == 0) return;
    const uint64_t blocks = (a.nrays + RELISTEN_RAYS - 1) / RELISTEN_RAYS;
    const size_t lds = ((size_t) RELISTEN_SURFACES_AT + 16u * a.lds_surfaces) * sizeof(uint32_t);
    hipLaunchKernelGGL(a.lds_surfaces ? relisten_records_kernel<true> : relisten_records_kernel<false>, dim3((unsigned) blocks), dim3(WAVE), lds, s, a, kept,
                       listen);
}
