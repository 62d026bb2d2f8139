// image_kernels.hip — the IMAGE-SOURCE stage of the trace, reference rayverb/kernel.cpp:379-457 (path stage: trace_kernels.hip, shadow
// stage: shadow_kernels.hip, shared device code: traversal.h).
//   image_plan_kernel / image_check_kernel
//                  image-source validation of a ray's first nine bounces: one lane per ray lists the (ray, bounce) pairs whose image
//                  ray crosses every mirrored triangle, four lanes per listed pair and query run the closest-hit / any-hit checks.  The
//                  inputs are only the triangles the ray hit, so this runs beside the record grouping instead of inside the ray's loop.
#include "traversal.h"

namespace {

// reference kernel.cpp:243-265 (add_image) for a known-valid slot; returns INIT_DIST, the length of the image path (what a re-shade
// keeps beside the impulse: TraceArgs::image_dist)
__device__ __forceinline__ float make_image(const TraceArgs & a, v3 mic, v3 mic_reflection, v3 source,
                                           const float volume[8], rvb_impulse & out)
{
    const v3 diff = source - mic_reflection;
    const float dist = length3(diff);
#pragma unroll
    for (int b = 0; b < 8; ++b)
        out.volume[b] = volume[b] * (air_attenuation(dist, a.air[b]) * 1.0f);
    const v3 pos = mic + diff;
    out.position[0] = pos.x; out.position[1] = pos.y; out.position[2] = pos.z; out.position[3] = 0.0f;
    out.time = seconds_per_meter() * dist;
    out.pad_[0] = out.pad_[1] = out.pad_[2] = 0.0f;
    return dist;
}

__device__ __forceinline__ TriVerts load_corners(const SceneDev & sc, uint32_t tri)
{
    const float4 * c = reinterpret_cast<const float4 *>(sc.corners + tri);
    const float4 a = c[0], b = c[1], e = c[2];
    TriVerts t;
    t.v0 = mk3(a.x, a.y, a.z);
    t.v1 = mk3(a.w, b.x, b.y);
    t.v2 = mk3(b.z, b.w, e.x);
    return t;
}

// A mirror plane of the image-source chain: the unit normal of a (mirrored) triangle and its first vertex.
// mirror_point (rvb_math.h, kernel.cpp:216-221) recomputes that normal — a cross product, a square root and three divisions —
// for every point it mirrors; here it is computed ONCE per plane with the same operations on the same operands, so the
// mirrored points are bit-identical.
struct MirrorPlane { v3 n, v0; };
__device__ __forceinline__ MirrorPlane mirror_plane(const TriVerts & t)
{
    MirrorPlane m;
    m.n = verts_normal(t);
    m.v0 = t.v0;
    return m;
}
__device__ __forceinline__ void mirror_point_on(v3 & p, const MirrorPlane & m)
{
    const float d = dot3(m.n, p - m.v0);
    p = p + ((-m.n) * d) * 2.0f;
}

// Image-source validation (kernel.cpp:379-457) in two kernels.
//
// A (ray, bounce) pair yields an image source iff (1) the ray from the source to the mirrored microphone crosses every mirrored
// triangle of the chain (Möller–Trumbore on the image triangles: arithmetic only), (2) each segment of the un-mirrored path is the
// closest hit of the real scene within +-EPSILON per component (a closest-hit query per segment), and (3) the last point sees the
// microphone (an any-hit query).  Hardly any pair passes (1) — a few hundred of 900 000 at workload C2 — and round 2's kernel (one lane
// per ray doing everything) took as long as its unluckiest LANE needed for up to eleven one-lane traversals in a row: 0.35 ms at 0.19
// lane use.  Now:
//   image_plan_kernel   one lane per ray walks its first nine bounces as before — the chain of mirrored triangles grown bounce by
//                       bounce, one mirror plane per bounce — but only evaluates (1) and appends the pairs that pass to a list;
//   image_check_kernel  FOUR lanes per listed pair and QUERY: rebuilds the pair's chain (all four lanes alike) and runs one of the
//                       queries of (2) and (3) with the quad traversal of the path kernel (four children / triangles per step instead
//                       of one); the pair's last query writes the image impulse.  The direct path (slot 0, one per source /
//                       microphone pair) is one more list entry.
// The operations on every value are the same as before, in the same order: results are bit-identical (tests/test_gpu_parity.py goldens).
#define RVB_IMAGE_DIRECT 0xFFFFFFFFu

// the ray's pair geometry (several (source, microphone) pairs may share a launch)
__device__ __forceinline__ void image_pair_of(const TraceArgs & a, uint32_t ray, uint32_t & pair, v3 & mic, v3 & source)
{
    pair = 0;
    mic = ld3(a.mic);
    source = ld3(a.source);
    if (a.npairs > 1) {
        pair = ray / a.rays_per_pair;
        const float4 m4 = a.pair_mics[pair], s4 = a.pair_sources[pair];
        mic = mk3(m4.x, m4.y, m4.z);
        source = mk3(s4.x, s4.y, s4.z);
    }
}

// One step of the chain (kernel.cpp:381-394): bounce `index`'s triangle through the planes so far, then the microphone through it.
struct ImageChain {
    TriVerts prev[RVB_NUM_IMAGE_SOURCE - 1];
    MirrorPlane plane[RVB_NUM_IMAGE_SOURCE - 1];
    v3 mic_reflection;
    __device__ __forceinline__ void extend(const SceneDev & sc, uint32_t index, uint32_t tri_here)
    {
        TriVerts current = load_corners(sc, tri_here);
        for (uint32_t j = 0; j < index; ++j) {
            mirror_point_on(current.v0, plane[j]);
            mirror_point_on(current.v1, plane[j]);
            mirror_point_on(current.v2, plane[j]);
        }
        prev[index] = current;
        plane[index] = mirror_plane(current);
        mirror_point_on(mic_reflection, plane[index]);
    }
    // the k-th crossing of the image ray, un-mirrored (kernel.cpp:406-414); false: the image ray misses image triangle k
    __device__ __forceinline__ bool crossing(uint32_t k, const v3 source, const v3 dir, v3 & ip) const
    {
        const float to_intersection = mt_intersect_verts(prev[k], source, dir);
        if (to_intersection <= RVB_EPSILON)
            return false;
        ip = source + dir * to_intersection;
        for (int l = (int) k - 1; l != -1; --l)
            mirror_point_on(ip, plane[l]);
        return true;
    }
};

__global__ __launch_bounds__(WAVE) void image_plan_kernel(TraceArgs a)
{
    const uint64_t ray = (uint64_t) blockIdx.x * WAVE + threadIdx.x;
    if (a.npairs <= 1 && ray == 0) {              // slot 0, the direct path (defined even for an empty ray set)
        const uint32_t at = atomicAdd(a.image_item_count, 1u);
        a.image_items[at] = ImageItem{0u, RVB_IMAGE_DIRECT};
    }
    if (ray >= a.nrays)
        return;
    uint32_t pair;
    v3 mic, source;
    image_pair_of(a, (uint32_t) ray, pair, mic, source);
    if (a.npairs > 1 && (uint32_t) ray == pair * a.rays_per_pair) {       // ... once per pair of a multi-pair launch
        const uint32_t at = atomicAdd(a.image_item_count, 1u);
        a.image_items[at] = ImageItem{pair, RVB_IMAGE_DIRECT};
    }
    const uint32_t per_ray = RVB_NUM_IMAGE_SOURCE - 1;
    const uint32_t * early = a.early + ray * per_ray;
    const uint32_t last = a.nreflections < per_ray ? a.nreflections : per_ray;
    ImageChain chain;
    chain.mic_reflection = mic;
    for (uint32_t index = 0; index < last; ++index) {
        const uint32_t tri_here = early[index];
        if (tri_here == NONE)
            break;                                // the ray escaped before this bounce
        chain.extend(a.scene, index, tri_here);
        const v3 dir = normalize3(chain.mic_reflection - source);      // kernel.cpp:396
        bool crosses = true;
        for (uint32_t k = 0; k != index + 1 && crosses; ++k) {
            v3 ip;
            crosses = chain.crossing(k, source, dir, ip);
        }
        if (crosses) {
            const uint32_t at = atomicAdd(a.image_item_count, 1u);     // (at most nrays * 9 + npairs entries: the list's capacity)
            a.image_items[at] = ImageItem{(uint32_t) ray, index};
            a.image_state[at] = 0u;
        }
    }
}

// reference kernel.cpp:274-296 (point_intersection) by the quad's four lanes
__device__ __forceinline__ bool point_visible_quad(const SceneDev & sc, v3 begin, v3 point, uint32_t * stack)
{
    const v3 b2p = point - begin;
    const float mag = length3(b2p);
    Hit h;
    return !traverse_quad<true>(sc, begin, normalize3(b2p), mag, stack, h);
}

// Four lanes per (listed pair, query): a pair at bounce `index` owns index + 1 closest-hit queries and one any-hit query, which do not
// depend on each other's results (the points come from the mirror chain, not from the queries), so they run side by side in
// RVB_IMAGE_QUERIES quad slots per pair instead of one after the other (one quad walking a ninth-bounce pair's ten queries took as long
// as round 2's whole kernel).  Every query adds its verdict to the pair's state word — low half: queries done, high half: queries
// failed — and the one whose add completes the pair writes the image impulse if none failed.
#define RVB_IMAGE_QUERIES (RVB_NUM_IMAGE_SOURCE + 1)
__global__ __launch_bounds__(WAVE) void image_check_kernel(TraceArgs a)
{
    extern __shared__ __attribute__((aligned(16))) uint32_t stack_lds[];   // [stack_entries][QUADS_PER_BLOCK]
    const uint32_t q = threadIdx.x >> 2, c = threadIdx.x & 3u;
    uint32_t * stack = stack_lds + q;
    const uint64_t slots = (uint64_t) *a.image_item_count * RVB_IMAGE_QUERIES;
    for (uint64_t slot = (uint64_t) blockIdx.x * QUADS_PER_BLOCK + q; slot < slots; slot += (uint64_t) gridDim.x * QUADS_PER_BLOCK) {
        const uint32_t item = (uint32_t) (slot / RVB_IMAGE_QUERIES), k = (uint32_t) (slot % RVB_IMAGE_QUERIES);
        const ImageItem it = a.image_items[item];
        uint32_t pair;
        v3 mic, source;
        if (it.index == RVB_IMAGE_DIRECT) {
            if (k != 0)
                continue;
            // slot 0 (kernel.cpp:335-357): identical for every ray of the pair, computed once
            image_pair_of(a, it.ray * a.rays_per_pair, pair, mic, source);
            rvb_impulse direct;
            for (int b = 0; b < 8; ++b) direct.volume[b] = 0.0f;
            for (int b = 0; b < 4; ++b) direct.position[b] = 0.0f;
            direct.time = 0.0f;
            direct.pad_[0] = direct.pad_[1] = direct.pad_[2] = 0.0f;
            const bool visible = point_visible_quad(a.scene, source, mic, stack);
            if (c == 0) {
                float dist = -1.0f;                 // (kept for a re-shade: negative = the direct path is hidden)
                if (visible) {
                    float one[8] = {1, 1, 1, 1, 1, 1, 1, 1};
                    dist = make_image(a, mic, mic, source, one, direct);
                }
                a.direct[it.ray] = direct;
                if (a.image_dist) a.image_dist[a.nrays * (RVB_NUM_IMAGE_SOURCE - 1) + it.ray] = dist;
            }
            continue;
        }
        if (k > it.index + 1)
            continue;                             // this pair has fewer queries than slots
        image_pair_of(a, it.ray, pair, mic, source);
        const uint32_t * early = a.early + (uint64_t) it.ray * (RVB_NUM_IMAGE_SOURCE - 1);
        ImageChain chain;
        chain.mic_reflection = mic;
        for (uint32_t index = 0; index <= it.index; ++index)
            chain.extend(a.scene, index, early[index]);
        // kernel.cpp:396-440: query k < index + 1 is the k-th segment of the un-mirrored path, query index + 1 the view of the microphone
        const v3 dir = normalize3(chain.mic_reflection - source);
        v3 begin = source, ip = source;
        bool ok = true;
        if (k > 0) ok = chain.crossing(k - 1, source, dir, begin);        // (cannot fail: image_plan_kernel evaluated the same expression)
        if (k <= it.index) {
            ok = ok && chain.crossing(k, source, dir, ip);
            const v3 idir = normalize3(ip - begin);
            Hit h;
            const bool found = traverse_quad<false>(a.scene, begin, idir, 0.0f, stack, h);
            const float hd = found ? h.t : 0.0f;                          // Intersection {0, 0, false}
            const v3 nip = begin + idir * hd;
            const bool lo = (nip.x - RVB_EPSILON < ip.x) && (nip.y - RVB_EPSILON < ip.y) && (nip.z - RVB_EPSILON < ip.z);
            const bool hi = (ip.x < nip.x + RVB_EPSILON) && (ip.y < nip.y + RVB_EPSILON) && (ip.z < nip.z + RVB_EPSILON);
            ok = ok && found && lo && hi;
        } else {
            ok = point_visible_quad(a.scene, begin, mic, stack) && ok;    // kernel.cpp:431-440
        }
        if (c != 0)
            continue;
        const uint32_t before = atomicAdd(a.image_state + item, ok ? 1u : 0x10001u);
        if ((before & 0xFFFFu) + 1u != it.index + 2u || (before >> 16) != 0u || !ok)
            continue;                             // not the pair's last query, or one of them failed
        // kernel.cpp:442-456: the ray's volume BEFORE this bounce's surface is applied
        float volume[8];
        if (it.index == 0) {
            for (int b = 0; b < 8; ++b) volume[b] = 1.0f;
        } else {
            const float4 * rec = reinterpret_cast<const float4 *>(a.impulses + (uint64_t) it.ray * a.nreflections + (it.index - 1));
            const float4 v0 = rec[0], v1 = rec[1];
            volume[0] = v0.x; volume[1] = v0.y; volume[2] = v0.z; volume[3] = v0.w;
            volume[4] = v1.x; volume[5] = v1.y; volume[6] = v1.z; volume[7] = v1.w;
        }
        rvb_image_candidate cand;
        cand.ray = a.ray_offset + it.ray;
        cand.slot = it.index + 1;
        cand.index = early[it.index] + 1;
        const float dist = make_image(a, mic, chain.mic_reflection, source, volume, cand.impulse);
        const uint32_t at = atomicAdd(a.candidate_count, 1u);
        a.candidates[at] = cand;
        if (a.image_dist) a.image_dist[at] = dist;
    }
}

}  // namespace

void rvb_launch_images(const TraceArgs & a, hipStream_t s)
{
    const unsigned blocks = (unsigned) ((a.nrays + WAVE - 1) / WAVE);     // one lane per ray
    hipLaunchKernelGGL(image_plan_kernel, dim3(blocks ? blocks : 1), dim3(WAVE), 0, s, a);
    // a few hundred list entries at workload C2: 256 single-wave workgroups of 16 quads walk the list whatever its length
    hipLaunchKernelGGL(image_check_kernel, dim3(256), dim3(WAVE), TraceLds::make(a.stack_entries, 0, 4, false).bytes, s, a);
}
