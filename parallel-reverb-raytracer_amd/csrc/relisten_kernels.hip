// relisten_kernels.hip — a new microphone on a finished trace (rvb_keep_paths with RVB_KEEP_LISTENER / rvb_relisten of include/rvb_capi.h):
// the work records of the path stage again, without the path stage.  No reference counterpart for the stage; in the reference's kernel
// the closest-hit / reflect chain (kernel.cpp:359-375, :459-461, :478, :492-501) never reads the microphone, which enters in the shadow
// ray (:463-490), the image-source validation (:379-457) and the direct path (:335-357) only.
//   relisten_records_kernel   a wave takes eight rays tile by tile of RELISTEN_TILE bounces, with reshade_kernel's LDS layout and its first
//                             two phases (KeptTileLds, stage_side_records, chain_over_tile of kept_tiles.h, the last written out): the side records of the tile
//                             go to LDS; lane (ray, band) runs the sequential chain vol = -vol * specular over the tile into LDS; then
//                             the wave streams the tile's records two lanes per record, whole 16-byte chunks: lane 0 the volume chunk of
//                             bands 0-3 and (position, DIFF), lane 1 that of bands 4-7 and (newDist, threshold, triangle, pair + 1) — the
//                             layout of trace_kernels.hip, "Work record".  The position is the one the shadow stage left in the record;
//                             DIFF, newDist come from the side record, threshold and triangle from the listener record that
//                             path_keep_kernel wrote beside it (SideRecord, ListenRecord of kept_tiles.h).
// The shadow, image and source-pattern kernels then run on these records exactly as behind a path kernel.
#include "kept_tiles.h"

namespace {

#define RELISTEN_TILE 32u            // bounces per tile
typedef KeptTileLds<RELISTEN_TILE> RelistenLds;

template <bool SURF_LDS>
__global__ __launch_bounds__(WAVE) void relisten_records_kernel(TraceArgs a, const float4 * __restrict__ kept, const uint2 * __restrict__ listen)
{
    typedef RelistenLds L;
    extern __shared__ __attribute__((aligned(16))) uint32_t lds[];
    float4 * side = L::side(lds);
    float * chain = L::chain(lds);
    const lds_float4_ptr surf_lds = stage_surfaces(a, L::surfaces(lds));
    const uint32_t lane = threadIdx.x, h = lane & 1u;
    const uint64_t ray0 = (uint64_t) blockIdx.x * L::RAYS;
    const uint32_t chain_ray = lane >> 3, band = lane & 7u;
    float vol = 1.0f;                                        // vol_b(-1) of this lane's (ray, band)
    bool alive = true;
    for (uint32_t first = 0; first < a.nreflections; first += RELISTEN_TILE) {
        stage_side_records<RELISTEN_TILE>(a, kept, ray0, first, side);                    // (1)
        __syncthreads();
        // (2) kernel.cpp:461 along the ray, one band per lane: chain_over_tile of kept_tiles.h written out (through the function the
        // staged surface's address is recomputed in every step, and this kernel is 3 % slower: profiles/kept_tiles_n1.txt)
        for (uint32_t k = 0; k < RELISTEN_TILE && alive; ++k) {
            const uint32_t surface = lds[L::surface_word(chain_ray, k)];
            if (surface == NONE) {
                alive = false;
                break;
            }
            vol = chain_step<SURF_LDS>(a, surf_lds, vol, surface, band);
            chain[L::vol_at(chain_ray, k) + band] = vol;
        }
        __syncthreads();
        // (3) the tile's work records, two lanes per record: lane h stores chunks h and h + 2
        for (uint32_t j = lane >> 1; j < L::RAYS * RELISTEN_TILE; j += WAVE / 2) {
            const uint32_t r = j / RELISTEN_TILE, k = j % RELISTEN_TILE;
            const uint64_t ray = ray0 + r;
            if (!(ray < a.nrays && first + k < a.nreflections))
                continue;
            const uint64_t record = ray * a.nreflections + first + k;
            float4 * rec = reinterpret_cast<float4 *>(a.impulses + record);
            const float4 sd = side[L::at(r, k)];
            // a slot behind an escape: all 64 bytes zero, as the path stage leaves it (a source pattern may have left -0 in the volumes)
            float4 v = make_float4(0, 0, 0, 0), aux = v;
            if (SideRecord::surface(sd) != NONE) {
                v = *reinterpret_cast<const float4 *>(chain + L::vol_at(r, k) + 4u * h);
                if (h == 0) {
                    // the hit point: the shadow stage wrote it back for invisible records too, and nothing behind it changes it
                    const float4 p = load_stream(rec + 2);
                    aux = make_float4(p.x, p.y, p.z, SideRecord::diff(sd));
                } else {
                    const ListenRecord l = ListenRecord::load(listen, record);
                    const uint32_t pair = a.npairs > 1 ? (uint32_t) (ray / a.rays_per_pair) : 0u;
                    aux = make_float4(SideRecord::new_dist(sd), __uint_as_float(l.threshold()), __uint_as_float(l.triangle()), __uint_as_float(pair + 1u));
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
    hipLaunchKernelGGL(a.lds_surfaces ? relisten_records_kernel<true> : relisten_records_kernel<false>, dim3((unsigned) RelistenLds::groups(a.nrays)),
                       dim3(WAVE), RelistenLds::bytes(a.lds_surfaces), s, a, kept, listen);
}
