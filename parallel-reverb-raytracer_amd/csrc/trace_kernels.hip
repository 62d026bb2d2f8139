// trace_kernels.hip — the PATH stage of the per-ray trace of reference rayverb/kernel.cpp:304-503 (kernel `raytrace`), re-organised for
// CDNA4 as three stages over one 4-wide BVH.  The other two are image_kernels.hip (image-source validation, kernel.cpp:379-457) and
// shadow_kernels.hip (shadow rays and final Impulses, kernel.cpp:463-490); what they share — traversal loops, LDS layout — is traversal.h.
//   path_kernel / path_pair_group_kernel / path_lane_group_kernel
//                  the inherently sequential chain closest hit -> reflect (kernel.cpp:359-375, :459-461, :478, :492-501).
//                  Latency-bound: SEVERAL LANES PER RAY — four (100k rays are 6250 waves instead of 1563: enough waves to hide the
//                  dependent node fetches), two (a quarter fewer instructions per bounce; chosen when the rays in flight fill the chip
//                  anyway, rvb_path_lanes_for) or one (group launches of about 400 k rays).  Per bounce it leaves a 64-byte work
//                  record in the ray's Impulse slot.
#include "traversal.h"

#include <algorithm>
#include <cstdlib>

namespace {

// ------------------------------------------------------------------------------------------------
// Work record left by path_kernel in impulses[ray*nrefl + bounce] (64 B; quad lane c stores chunk c):
//   chunk 0,1  newVol = -volume * specular                        (kernel.cpp:461)
//   chunk 2    intersection.xyz, DIFF = |dot(normal, dir)|         (kernel.cpp:459, :478)
//   chunk 3    newDist, own-plane threshold of the shadow ray, triangle index, pair + 1 = valid   (kernel.cpp:460)
// shadow_kernel turns it into the final Impulse in place.
// One ray's bounce chain as a Job: next() hands out the current ray, done() shades the hit
// (kernel.cpp:459-461, :478), stores the work record and reflects (kernel.cpp:492-501).
// LANES = 4: quad lane c stores chunk c.  LANES = 2: lane c of the pair stores chunks c and c + 2.
// (The lane's band volumes and path length kept in LDS between bounces instead of in registers — "cold ray state" — lose in the
// pipeline: DESIGN.md §3.)
__device__ __forceinline__ uint32_t lane_id_here()
{
    uint32_t lane;      // (volatile: recomputed where it is used instead of being kept in a register across the traversal loop)
    asm volatile("v_mbcnt_lo_u32_b32 %0, -1, 0\n\tv_mbcnt_hi_u32_b32 %0, -1, %0" : "=v"(lane));
    return lane;
}
// A ray's lanes write one key run (see PathJob) as whole 16-byte pieces of a 64-byte segment.  LANES = 4: lane c writes piece c, 2: pieces
// 2c and 2c + 1, 1: all four.
template <int LANES>
__device__ __forceinline__ void flush_key_run(const TraceArgs & a, const uint32_t c, const uint16_t * row, const uint64_t first_record)
{
    const uint4 * src = reinterpret_cast<const uint4 *>(row);
    uint4 * dst = reinterpret_cast<uint4 *>(a.sort_keys16 + first_record);
    if (LANES == 4) {
        dst[c] = src[c];
    } else if (LANES == 2) {
        dst[2 * c] = src[2 * c];
        dst[2 * c + 1] = src[2 * c + 1];
    } else {
        dst[0] = src[0]; dst[1] = src[1]; dst[2] = src[2]; dst[3] = src[3];
    }
}
template <bool SURF_LDS, int LANES = 4>
struct PathJob {
    const TraceArgs & a;
    uint32_t ray;                        // < 2^32 / 9 (rvb_trace checks)
    uint32_t c;
    v3 o, d;
    float distance;
    float4 vol;                          // lane 0 (and 2): bands 0-3, lane 1 (and 3): bands 4-7 — the chunk the lane stores
    uint32_t index;
    bool alive;
    lds_float4_ptr surf_lds;             // the surface table staged in LDS (stage_surfaces); unused when !SURF_LDS
    uint32_t pair_tag;                   // (source, microphone) pair of this ray + 1: what marks its work records as valid
    uint32_t skip;                       // own-plane subtree of the triangle the current segment starts on (TriShade, bvh.h)
    bool unit;                           // the ray's direction has unit length (the own-plane rule is derived for |d| = 1)
    uint16_t * key_rows;                 // key runs (TraceArgs::sort_keys16): this workgroup's [rays][RVB_KEY_RUN] 16-bit keys in LDS

    // Record-grouping keys as 64-byte RUNS.  The grouping key of a record (the leaf position of the triangle hit, 16 significant
    // bits) used to leave as one 4-byte store per record, 8 KB apart in a ray's row: 51 MB of keys cost 0.4 GB of HBM writes (a
    // partial-line write each; WRITE_SIZE 1.29 GB per launch for 0.87 GB of records and keys).  Now lane 1 of the ray parks the
    // 16-bit key in LDS and, every RVB_KEY_RUN bounces, the ray's lanes write the run as whole 16-byte pieces of one 64-byte segment.
    __device__ __forceinline__ uint16_t * key_row() const { return key_rows + (lane_id_here() >> (LANES == 4 ? 2 : 1)) * RVB_KEY_RUN; }

    __device__ __forceinline__ uint32_t skip_ref() const { return skip; }
    __device__ __forceinline__ bool next(v3 & o_, v3 & d_, float & tmax)
    {
        if (!alive || index >= a.nreflections)
            return false;
        o_ = o;
        d_ = d;
        tmax = 0.0f;
        return true;
    }
    __device__ __forceinline__ void done(bool hit, const Hit & h)
    {
        if (!hit) {                                                  // kernel.cpp:372-375
            alive = false;
            return;
        }
        const float4 * shade = reinterpret_cast<const float4 *>(a.scene.shade + h.tri);       // 32 B: normal + surface, own-plane skip
        const float4 sh = shade[0], sk = shade[1];
        const v3 normal = mk3(sh.x, sh.y, sh.z);
        const uint32_t surface = __float_as_uint(sh.w);
        // the specular row hangs off a dependent load (triangle -> surface -> row): from LDS it costs ~64 cycles
        // instead of another L2 round trip; each lane reads the half row of the four bands it carries
        const uint32_t half = c & 1u;
        const float4 sp = surface_row<SURF_LDS>(a, surf_lds, surface, half);
        const v3 p = o + d * h.t;                                    // kernel.cpp:459
        const float new_dist = distance + h.t;                       // kernel.cpp:460
        vol = make_float4(-vol.x * sp.x, -vol.y * sp.y, -vol.z * sp.z, -vol.w * sp.w);   // kernel.cpp:461
        const float diff = fabsf(dot3(normal, d));                   // kernel.cpp:478
        // Own-plane skip (bvh.h): the rays that START at p — the reflected ray and the shadow ray — may pass over the subtree of
        // this triangle's plane patch when they leave the plane steeply enough: |cos| > skip_a + skip_b * (segment length).  The
        // reflected ray's |cos| is `diff` (reflection keeps it); the shadow kernel compares its own against the threshold the
        // record carries (+inf: no skip).
        const float threshold = unit ? fmaf(sk.z, h.t, sk.y) : __builtin_inff();
        skip = diff > threshold ? __float_as_uint(sk.x) : RVB_BVH_EMPTY;
        float4 chunk = vol;
        const float4 tail = make_float4(new_dist, threshold, __uint_as_float(h.tri), __uint_as_float(pair_tag));   // tag: pair + 1, non-zero = valid
        if (LANES == 4) {
            if (c == 2) chunk = make_float4(p.x, p.y, p.z, diff);
            else if (c == 3) chunk = tail;
        }
        // (the product is formed here, one v_mad_u64_u32 per bounce: hoisted out of the loop it would hold two more VGPRs for
        // the whole traversal, which at the 64-register budget of 8 waves per SIMD means a spill)
        uint32_t ray_here = ray;
        asm volatile("" : "+v"(ray_here));
        const uint64_t record = (uint64_t) ray_here * a.nreflections + index;
        store_stream(reinterpret_cast<float4 *>(a.impulses + record) + c, chunk);
        if (LANES == 2)
            store_stream(reinterpret_cast<float4 *>(a.impulses + record) + c + 2, c == 0 ? make_float4(p.x, p.y, p.z, diff) : tail);
        if (c == 0 && index < RVB_NUM_IMAGE_SOURCE - 1)
            a.early[ray * (RVB_NUM_IMAGE_SOURCE - 1) + index] = h.tri;
        if (a.sort_keys16) {                                         // (wave-uniform) keys leave in runs, see flush_key_run
            uint16_t * row = key_row();
            const uint32_t at = index & (RVB_KEY_RUN - 1u);
            if (c == 1) row[at] = (uint16_t) (__float_as_uint(sk.w) >> a.key_shift);      // the triangle's position in leaf order (rvb_set_scene put it there)
            if (at == RVB_KEY_RUN - 1u) {
                __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");      // lane 1's 16-bit store before the 16-byte loads of the ray's other lane(s)
                flush_key_run<LANES>(a, c, row, record - at);
            }
        } else if (c == 1 && a.sort_keys) {
            a.sort_keys[record] = __float_as_uint(sk.w);
        }
        d = reflect3(normal, d);                                     // kernel.cpp:492-499
        o = p;
        distance = new_dist;
        ++index;
    }
};

// A ray's start: its pair (kernels.h, "several pairs in ONE launch"), the tag that marks its records valid, is the direction of unit length
struct RayStart { uint32_t pair, pair_tag; v3 source, dir; bool unit; };
__device__ __forceinline__ RayStart ray_start(const TraceArgs & a, const uint64_t ray)
{
    uint32_t pair = 0, local = (uint32_t) ray;
    v3 source = ld3(a.source);
    if (a.npairs > 1) {                           // wave-uniform
        pair = (uint32_t) ray / a.rays_per_pair;
        local = (uint32_t) ray - pair * a.rays_per_pair;
        const float4 s4 = a.pair_sources[pair];
        source = mk3(s4.x, s4.y, s4.z);
    }
    const float4 d4 = a.directions[local];
    const float len2 = d4.x * d4.x + d4.y * d4.y + d4.z * d4.z;
    return {pair, pair + 1u, source, mk3(d4.x, d4.y, d4.z), fabsf(len2 - 1.0f) < 1e-3f};
}

// After the traversal: an escaped ray leaves its remaining slots zero-filled (reference rayverb.cpp:600-603 zero-fills the whole
// buffer before every launch; here only the few slots that need it are written) and their grouping keys "no record".
// LANES = 4: quad lane c stores chunk c (and key piece c), 2: lane c of the pair chunks c and c + 2, 1: the lane stores all four.
// key_row(): the ray's key run in LDS, asked for only when there are key runs.
template <int LANES, class KeyRow>
__device__ __forceinline__ void finish_escaped_ray(const TraceArgs & a, const uint64_t ray, const uint32_t index, const uint32_t c, KeyRow key_row)
{
    if (index >= a.nreflections)
        return;
    const float4 zero = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
    for (uint32_t i = index; i < a.nreflections; ++i) {
        const uint64_t record = ray * a.nreflections + i;
        float4 * rec = reinterpret_cast<float4 *>(a.impulses + record);
        if (LANES == 1) { store_stream(rec + 0, zero); store_stream(rec + 1, zero); store_stream(rec + 2, zero); store_stream(rec + 3, zero); }
        else store_stream(rec + c, zero);
        if (LANES == 2) store_stream(rec + c + 2, zero);
        if ((LANES == 1 || c == 1) && a.sort_keys)
            a.sort_keys[LANES == 1 ? ray * a.nreflections + i : record] = NONE;      // (one lane: formed again, i.e. nreflections read again behind the stores, as that kernel's code has it)
    }
    if (a.sort_keys16) {
        // the run the ray was in: its remaining keys become "no record", then it leaves like any other; whole runs after it directly
        uint16_t * row = key_row();
        uint32_t i = index;
        const uint32_t at = i & (RVB_KEY_RUN - 1u);
        if (at) {
            if (LANES == 1 || c == 1)
                for (uint32_t k = at; k < RVB_KEY_RUN; ++k) row[k] = 0xFFFFu;
            __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
            flush_key_run<LANES>(a, c, row, ray * a.nreflections + (i - at));
            i += RVB_KEY_RUN - at;
        }
        const uint4 none = make_uint4(0xFFFFFFFFu, 0xFFFFFFFFu, 0xFFFFFFFFu, 0xFFFFFFFFu);
        for (; i < a.nreflections; i += RVB_KEY_RUN) {
            uint4 * dst = reinterpret_cast<uint4 *>(a.sort_keys16 + ray * a.nreflections + i);
            if (LANES == 4) dst[c] = none;
            else if (LANES == 2) { dst[2 * c] = none; dst[2 * c + 1] = none; }
            else { dst[0] = none; dst[1] = none; dst[2] = none; dst[3] = none; }
        }
    }
}

// 64 VGPRs = 8 waves per SIMD: one resident round holds 8 x 1024 x 16 = 131 072 rays, so the 125 k rays per GPU of
// workload C3 still run as one round (at 72 VGPRs / 7 waves they took 5.1 ms instead of 4.3 ms).
// WAVES = 7 (72 VGPRs) is the build for launches that fit in seven waves per SIMD (<= 114 688 rays: the 100 k rays of workload C2 are
// 6.1 waves per SIMD): with the registers of slab_select and no spill, 3.66 -> 3.50 ms at C2; the 8-wave build keeps larger launches
// (up to 131 072 rays) in one resident round (3.66 -> 3.58 ms at C2 with slab_select and two spilled registers).
template <bool SURF_LDS, int WAVES>
__global__ __launch_bounds__(WAVE, WAVES) void path_kernel(TraceArgs a)
{
    extern __shared__ __attribute__((aligned(16))) uint32_t stack_lds[];   // [stack_entries][QUADS_PER_BLOCK]
    const uint32_t q = threadIdx.x >> 2;
    const uint64_t ray = (uint64_t) blockIdx.x * QUADS_PER_BLOCK + q;
    const TraceLds lds = TraceLds::make(a.stack_entries, a.lds_surfaces, 4, true);
    const lds_float4_ptr surf_lds = stage_surfaces(a, lds.surfaces(stack_lds));
    if (ray >= a.nrays)
        return;                                   // whole quads leave together
    const RayStart r = ray_start(a, ray);
    PathJob<SURF_LDS> job = {a, (uint32_t) ray, threadIdx.x & 3u, r.source, r.dir, 0.0f,
                   make_float4(1.0f, 1.0f, 1.0f, 1.0f), 0u, true, surf_lds, r.pair_tag, RVB_BVH_EMPTY, r.unit, lds.key_runs(stack_lds)};
    traverse_jobs_cycle(a.scene, stack_lds + q, job);
    finish_escaped_ray<4>(a, ray, job.index, job.c, [&] { return job.key_row(); });
    if (job.c == 0)
        atomicAdd(a.executed, (unsigned long long) job.index);
}

// path_kernel with two lanes per ray (traverse_pairs_cycle): 32 rays per single-wave workgroup.
template <bool SURF_LDS>
__device__ __forceinline__ void path_pair_body(const TraceArgs & a, const uint32_t block)
{
    extern __shared__ __attribute__((aligned(16))) uint32_t stack_lds[];   // [stack_entries][PAIRS_PER_BLOCK]
    const uint32_t q = threadIdx.x >> 1;
    const uint64_t ray = (uint64_t) block * PAIRS_PER_BLOCK + q;
    const TraceLds lds = TraceLds::make(a.stack_entries, a.lds_surfaces, 2, true);
    const lds_float4_ptr surf_lds = stage_surfaces(a, lds.surfaces(stack_lds));
    if (ray >= a.nrays)
        return;                                   // whole pairs leave together
    const RayStart r = ray_start(a, ray);
    PathJob<SURF_LDS, 2> job = {a, (uint32_t) ray, threadIdx.x & 1u, r.source, r.dir, 0.0f,
                   make_float4(1.0f, 1.0f, 1.0f, 1.0f), 0u, true, surf_lds, r.pair_tag, RVB_BVH_EMPTY, r.unit, lds.key_runs(stack_lds)};
    traverse_pairs_cycle(a.scene, stack_lds + q, job);
    finish_escaped_ray<2>(a, ray, job.index, job.c, [&] { return job.key_row(); });
    if (job.c == 0)
        atomicAdd(a.executed, (unsigned long long) job.index);
}

// Several traces (contexts: their own rays, buffers, source and microphone) in ONE launch.  Two path kernels launched side by side
// are not scheduled alike — the first one's waves are older and issue first, the second runs on alone at half the occupancy (4.9 and
// 7.9 ms at workload C2) — whereas the waves of one launch advance together.  first_block[k] = first workgroup of trace k.
struct TraceGroup {
    uint32_t count;
    uint32_t first_block[RVB_MAX_GROUP + 1];
    TraceArgs trace[RVB_MAX_GROUP];
};
template <bool SURF_LDS>
__global__ __launch_bounds__(WAVE, RVB_PAIR_WAVES) void path_pair_group_kernel(TraceGroup g)
{
    uint32_t which = 0;                  // the trace this workgroup belongs to
    for (uint32_t k = 1; k < g.count; ++k)
        which += blockIdx.x >= g.first_block[k] ? 1u : 0u;
    path_pair_body<SURF_LDS>(g.trace[which], blockIdx.x - g.first_block[which]);
}

// ONE LANE PER RAY (path_lane_group_kernel, round 4): 64 rays per single-wave workgroup, every lane walks its own ray — it tests the
// four children of its node and the up-to-four triangles of its leaf itself, nothing is exchanged between lanes, and the stack is the
// lane's own column in LDS.  What the lanes of a pair (or quad) repeat per ray — the schedule's state, the stack pointer, the child
// keys, the lane exchange, the 64-bit key reductions — is paid once per ray, and a wave step serves 64 rays: tools/travforms.cpp
// replays C2 at 29.3 node + 5.4 leaf + 2.7 shading wave steps per 64 ray-bounces (pairs: 28.5 + 5.2 + 2.6 per 32), i.e. a quarter to
// a third fewer wave instructions per ray-bounce with the step costs of this kernel's ISA.  The price is half the waves again (100 k
// rays are 1.5 waves per SIMD) and longer steps, so a launch is bound by the latency of one wave's chain unless about 400 k rays are
// in flight: rvb_path_lanes_for picks it for group launches of that size only.  Same arithmetic, same records, same bytes as the
// other two path kernels (tests/test_gpu_parity.py runs every trace case with all three).
// (A cooperative node fetch — the four lanes of a quad load each other's nodes straight into LDS, one 64-byte access per node — was
// measured and is slower than the four 16-byte loads per lane below: DESIGN.md §3.)
template <bool SURF_LDS>
__device__ __forceinline__ void path_lane_body(const TraceArgs & a, const uint32_t block)
{
    // LDS of the workgroup: [stack_entries + 1][64] stack words (a lane's column; one slack row: pushes store first and advance if
    // kept), the surface table, [64][RVB_KEY_RUN] 16-bit grouping keys (TraceLds)
    extern __shared__ __attribute__((aligned(16))) uint32_t stack_lds[];
    const uint32_t IDLE = 0xFFFFFFFEu;
    const uint32_t lane = threadIdx.x;
    const uint64_t ray = (uint64_t) block * LANE_RAYS + lane;
    const TraceLds lds = TraceLds::make(a.stack_entries, a.lds_surfaces, 1, true);
    // (one named pointer behind the stack, the key runs 16 words per surface behind it: through lds.key_runs() this kernel's prologue is allocated differently)
    uint32_t * const after_stack = lds.surfaces(stack_lds);
    const lds_float4_ptr surf_lds = stage_surfaces(a, after_stack);
    uint16_t * const key_row = reinterpret_cast<uint16_t *>(after_stack + 16u * a.lds_surfaces) + lane * RVB_KEY_RUN;
    if (ray >= a.nrays)
        return;
    const RayStart r = ray_start(a, ray);
    v3 o = r.source, d = r.dir;
    const bool unit = r.unit;
    const uint32_t pair_tag = r.pair_tag;
    float4 vol_lo = make_float4(1.0f, 1.0f, 1.0f, 1.0f), vol_hi = vol_lo;      // kernel.cpp:322-323
    float distance = 0.0f;
    uint32_t index = 0, skip = RVB_BVH_EMPTY;

    const char * node_base = reinterpret_cast<const char *>(a.scene.nodes);
    const char * tri_base = reinterpret_cast<const char *>(a.scene.tris);
    const float neg_cull = -a.scene.cull_abs, cull_scale = 1.0f + a.scene.cull_rel;
    const unsigned long long NO_HIT_KEY = (0x7F800000ull << 32) | NONE;
    const lds_u32_ptr bottom = (lds_u32_ptr) stack_lds + lane;
    lds_u32_ptr sp = bottom;
    float ix = 0.0f, iy = 0.0f, iz = 0.0f, oix = 0.0f, oiy = 0.0f, oiz = 0.0f;
    uint32_t selx = 0, sely = 0, selz = 0;
    unsigned long long best_key = NO_HIT_KEY;
    uint32_t ref = IDLE;
#define RESET_QUERY_LANE()                                                               \
    {                                                                                    \
        ix = clamp_inv(d.x); iy = clamp_inv(d.y); iz = clamp_inv(d.z);                   \
        oix = o.x * ix; oiy = o.y * iy; oiz = o.z * iz;                                  \
        selx = slab_selector(ix); sely = slab_selector(iy); selz = slab_selector(iz);    \
        best_key = NO_HIT_KEY; sp = bottom; ref = 0;                                     \
    }
    if (index < a.nreflections) RESET_QUERY_LANE()
    for (;;) {
        RVB_MARK("vote");
        const unsigned long long m_node = __builtin_amdgcn_ballot_w64((int32_t) ref >= 0);
        const unsigned long long m_done = __builtin_amdgcn_ballot_w64(ref == NONE);
        const unsigned long long m_leaf = __builtin_amdgcn_ballot_w64((int32_t) ref < (int32_t) IDLE);
        const int n_node = scalar_popcount(m_node), n_done = scalar_popcount(m_done), n_leaf = scalar_popcount(m_leaf);
        if ((n_node | n_done | n_leaf) == 0)
            break;
        if (n_node >= n_leaf && n_node >= n_done) {
            RVB_MARK("node");
            if ((int32_t) ref >= 0) {
                const uint4 * np = reinterpret_cast<const uint4 *>(node_base + ref);
                const uint4 n0 = np[0], n1 = np[1], n2 = np[2], n3 = np[3];
                const float limit = fmaf(__uint_as_float((uint32_t) (best_key >> 32)), cull_scale, a.scene.cull_abs);
                float tn0, tn1, tn2, tn3;
                const bool ok0 = slab_select(n0, ix, iy, iz, oix, oiy, oiz, selx, sely, selz, limit, neg_cull, skip, tn0);
                const bool ok1 = slab_select(n1, ix, iy, iz, oix, oiy, oiz, selx, sely, selz, limit, neg_cull, skip, tn1);
                const bool ok2 = slab_select(n2, ix, iy, iz, oix, oiy, oiz, selx, sely, selz, limit, neg_cull, skip, tn2);
                const bool ok3 = slab_select(n3, ix, iy, iz, oix, oiy, oiz, selx, sely, selz, limit, neg_cull, skip, tn3);
                // nearest hit child first, by the same (entry distance | child) keys as the other path kernels: the visiting order, and
                // with it the culling, is theirs
                const uint32_t key0 = ok0 ? ((__float_as_uint(fmaxf(tn0, 0.0f)) & ~3u) | 0u) : NONE;
                const uint32_t key1 = ok1 ? ((__float_as_uint(fmaxf(tn1, 0.0f)) & ~3u) | 1u) : NONE;
                const uint32_t key2 = ok2 ? ((__float_as_uint(fmaxf(tn2, 0.0f)) & ~3u) | 2u) : NONE;
                const uint32_t key3 = ok3 ? ((__float_as_uint(fmaxf(tn3, 0.0f)) & ~3u) | 3u) : NONE;
                const uint32_t kmin = min(min(key0, key1), min(key2, key3));
                // the other hit children go on the stack in child order: store, then advance past the store if it is kept
                *sp = n0.w; sp += (ok0 && key0 != kmin) ? LANE_RAYS : 0;
                *sp = n1.w; sp += (ok1 && key1 != kmin) ? LANE_RAYS : 0;
                *sp = n2.w; sp += (ok2 && key2 != kmin) ? LANE_RAYS : 0;
                *sp = n3.w; sp += (ok3 && key3 != kmin) ? LANE_RAYS : 0;
                if (kmin == NONE) {
                    if (sp != bottom) { sp -= LANE_RAYS; ref = *sp; } else ref = NONE;
                } else {
                    const uint32_t lo = (kmin & 1u) ? n1.w : n0.w, hi = (kmin & 1u) ? n3.w : n2.w;
                    ref = (kmin & 2u) ? hi : lo;
                }
            }
        } else if (n_leaf >= n_done) {
            RVB_MARK("leaf");
            if ((int32_t) ref < (int32_t) IDLE) {      // (this leaf step, the four-child test and the push / pop exist again in shadow_lane_kernel: every shared helper tried moved instructions in one of the two)
                const uint32_t first = ref & 0x0FFFFFFFu;
                const uint32_t count = ((ref >> 28) & 7u) + 1u;
                const float4 * tp0 = reinterpret_cast<const float4 *>(tri_base + tri_byte_offset(first));
                const float4 * tp1 = reinterpret_cast<const float4 *>(tri_base + tri_byte_offset(first + (1u < count ? 1u : 0u)));
                const float4 * tp2 = reinterpret_cast<const float4 *>(tri_base + tri_byte_offset(first + (2u < count ? 2u : 0u)));
                const float4 * tp3 = reinterpret_cast<const float4 *>(tri_base + tri_byte_offset(first + (3u < count ? 3u : 0u)));
                float4 ta = tp0[0], tb = tp0[1], tc = tp0[2], ua = tp1[0], ub = tp1[1], uc = tp1[2];
                float4 va = tp2[0], vb = tp2[1], vc = tp2[2], wa = tp3[0], wb = tp3[1], wc = tp3[2];
                // all twelve loads leave before the first use (one round trip per leaf step, not four)
                asm volatile("" : "+v"(ta.x), "+v"(tb.x), "+v"(tc.x), "+v"(ua.x), "+v"(ub.x), "+v"(uc.x),
                                  "+v"(va.x), "+v"(vb.x), "+v"(vc.x), "+v"(wa.x), "+v"(wb.x), "+v"(wc.x));
                const float dist0 = mt_intersect(mk3(ta.x, ta.y, ta.z), mk3(ta.w, tb.x, tb.y), mk3(tb.z, tb.w, tc.x), o, d);
                const float dist1 = mt_intersect(mk3(ua.x, ua.y, ua.z), mk3(ua.w, ub.x, ub.y), mk3(ub.z, ub.w, uc.x), o, d);
                const float dist2 = mt_intersect(mk3(va.x, va.y, va.z), mk3(va.w, vb.x, vb.y), mk3(vb.z, vb.w, vc.x), o, d);
                const float dist3 = mt_intersect(mk3(wa.x, wa.y, wa.z), mk3(wa.w, wb.x, wb.y), mk3(wb.z, wb.w, wc.x), o, d);
                // kernel.cpp:180-188 — smallest distance wins, equal distances go to the lower index: one unsigned 64-bit key
                const bool valid0 = dist0 > RVB_EPSILON, valid1 = 1u < count && dist1 > RVB_EPSILON;
                const bool valid2 = 2u < count && dist2 > RVB_EPSILON, valid3 = 3u < count && dist3 > RVB_EPSILON;
                const unsigned long long k0 = valid0 ? (((unsigned long long) __float_as_uint(dist0) << 32) | __float_as_uint(tc.y)) : NO_HIT_KEY;
                const unsigned long long k1 = valid1 ? (((unsigned long long) __float_as_uint(dist1) << 32) | __float_as_uint(uc.y)) : NO_HIT_KEY;
                const unsigned long long k2 = valid2 ? (((unsigned long long) __float_as_uint(dist2) << 32) | __float_as_uint(vc.y)) : NO_HIT_KEY;
                const unsigned long long k3 = valid3 ? (((unsigned long long) __float_as_uint(dist3) << 32) | __float_as_uint(wc.y)) : NO_HIT_KEY;
                best_key = min_u64(min_u64(best_key, min_u64(k0, k1)), min_u64(k2, k3));
                if (sp != bottom) { sp -= LANE_RAYS; ref = *sp; } else ref = NONE;
            }
        } else {
            RVB_MARK("done");
            if (ref == NONE) {
                const uint32_t tri = (uint32_t) best_key;
                ref = IDLE;
                if (tri != NONE) {                                           // (else: the ray escaped, kernel.cpp:372-375)
                    const float t = __uint_as_float((uint32_t) (best_key >> 32));
                    // PathJob::done with one lane: the same operations on the same operands
                    const float4 * shade = reinterpret_cast<const float4 *>(a.scene.shade + tri);
                    const float4 sh = shade[0], sk = shade[1];
                    const v3 normal = mk3(sh.x, sh.y, sh.z);
                    const uint32_t surface = __float_as_uint(sh.w);
                    const float4 s_lo = surface_row<SURF_LDS>(a, surf_lds, surface, 0), s_hi = surface_row<SURF_LDS>(a, surf_lds, surface, 1);
                    const v3 p = o + d * t;                                  // kernel.cpp:459
                    const float new_dist = distance + t;                     // kernel.cpp:460
                    vol_lo = make_float4(-vol_lo.x * s_lo.x, -vol_lo.y * s_lo.y, -vol_lo.z * s_lo.z, -vol_lo.w * s_lo.w);   // kernel.cpp:461
                    vol_hi = make_float4(-vol_hi.x * s_hi.x, -vol_hi.y * s_hi.y, -vol_hi.z * s_hi.z, -vol_hi.w * s_hi.w);
                    const float diff = fabsf(dot3(normal, d));               // kernel.cpp:478
                    const float threshold = unit ? fmaf(sk.z, t, sk.y) : __builtin_inff();      // own-plane skip (bvh.h)
                    skip = diff > threshold ? __float_as_uint(sk.x) : RVB_BVH_EMPTY;
                    const uint64_t record = (uint64_t) (uint32_t) ray * a.nreflections + index;
                    float4 * rec = reinterpret_cast<float4 *>(a.impulses + record);
                    store_stream(rec + 0, vol_lo);
                    store_stream(rec + 1, vol_hi);
                    store_stream(rec + 2, make_float4(p.x, p.y, p.z, diff));
                    store_stream(rec + 3, make_float4(new_dist, threshold, __uint_as_float(tri), __uint_as_float(pair_tag)));
                    if (index < RVB_NUM_IMAGE_SOURCE - 1)
                        a.early[(uint32_t) ray * (RVB_NUM_IMAGE_SOURCE - 1) + index] = tri;
                    if (a.sort_keys16) {                                     // (wave-uniform) grouping keys leave in 64-byte runs
                        const uint32_t at = index & (RVB_KEY_RUN - 1u);
                        key_row[at] = (uint16_t) (__float_as_uint(sk.w) >> a.key_shift);
                        if (at == RVB_KEY_RUN - 1u) {
                            __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");      // the row's 16-bit stores before its 16-byte loads
                            flush_key_run<1>(a, 0u, key_row, record - at);
                        }
                    } else if (a.sort_keys) {
                        a.sort_keys[record] = __float_as_uint(sk.w);
                    }
                    d = reflect3(normal, d);                                 // kernel.cpp:492-499
                    o = p;
                    distance = new_dist;
                    ++index;
                    if (index < a.nreflections) RESET_QUERY_LANE()
                }
            }
        }
        RVB_MARK("loop_end");
    }
#undef RESET_QUERY_LANE
    finish_escaped_ray<1>(a, (uint64_t) (uint32_t) ray, index, 0u, [&] { return key_row; });
    atomicAdd(a.executed, (unsigned long long) index);
}

template <bool SURF_LDS>
__global__ __launch_bounds__(WAVE, RVB_LANE_WAVES) void path_lane_group_kernel(TraceGroup g)
{
    uint32_t which = 0;                  // (written out in both group kernels: a shared helper for this loop inverts a branch of this kernel)
    for (uint32_t k = 1; k < g.count; ++k)
        which += blockIdx.x >= g.first_block[k] ? 1u : 0u;
    path_lane_body<SURF_LDS>(g.trace[which], blockIdx.x - g.first_block[which]);
}

}  // namespace

uint32_t rvb_lds_surfaces(uint32_t stack_entries, uint64_t nsurfaces)
{
    // 8 waves/SIMD = 32 single-wave workgroups per CU must still fit in the CU's 160 KiB of LDS: stack + key runs + surface table
    static const bool off = getenv("RVB_LDS_SURFACES") && getenv("RVB_LDS_SURFACES")[0] == '0';
    const size_t budget = (160u * 1024u) / 32u;
    const size_t stack = TraceLds::make(stack_entries, 0, 4, true).bytes;
    // ... and the two-lane kernels (twice the stack and key runs per workgroup) want 5 waves/SIMD = 20 workgroups per CU
    const size_t pair_budget = (160u * 1024u) / 20u;
    const size_t pair_stack = TraceLds::make(stack_entries, 0, 2, true).bytes;
    if (off || nsurfaces == 0 || stack + nsurfaces * sizeof(rvb_surface) > budget || pair_stack + nsurfaces * sizeof(rvb_surface) > pair_budget)
        return 0;
    return (uint32_t) nsurfaces;
}

// Lanes per ray of the path kernel.  Per ray-bounce the pair kernel issues 17 % fewer VALU instructions than the quad kernel (the
// schedule, stack and reduction work is per ray and every lane of the ray repeats it), but it has half the waves: it pays when the rays
// in flight fill the chip without the extra waves — one resident round of pair waves at 6 waves per SIMD is 6 x 1024 x 32 rays.
// Measured at workload C2 sizes (path kernel alone, ms per 100 k rays, quads / pairs): 100 k rays 3.60 / 3.79, 200 k 3.12 / 3.13,
// 400 k 2.77 / 2.49, 1 M 2.51 / 2.16; two 100 k traces in flight (the bench pipeline): 5.32 / 5.11 ms per IR.
uint32_t rvb_path_lanes_for(uint64_t nrays, uint32_t concurrent)
{
    static const int forced = getenv("RVB_PATH_LANES") ? atoi(getenv("RVB_PATH_LANES")) : 0;     // diagnostic override
    if (forced == 1 || forced == 2 || forced == 4) return (uint32_t) forced;
    // one lane per ray (path_lane_group_kernel) once the rays in flight give every SIMD RVB_LANE_MIN_WAVES waves of 64 rays: below
    // that its launch is bound by the latency of one wave's chain of (longer) steps, above it by how few instructions a ray costs
    static const uint64_t lane_min_waves = getenv("RVB_LANE_MIN_WAVES") ? strtoull(getenv("RVB_LANE_MIN_WAVES"), nullptr, 10) : 0;
    const uint64_t in_flight = nrays * (concurrent ? concurrent : 1u);
    if (lane_min_waves && in_flight >= lane_min_waves * 1024ull * LANE_RAYS) return 1u;
    return in_flight >= 6ull * 1024ull * PAIRS_PER_BLOCK ? 2u : 4u;
}

void rvb_launch_path(const TraceArgs & a, hipStream_t s)
{
    if (a.nrays == 0) return;
    if (a.path_lanes <= 2) {
        // one trace through the group kernel: the form that takes its arguments from the group block needs 80 registers and no scratch
        // (six waves per SIMD); a kernel of its own with TraceArgs by value came out at 86 once the key runs were added
        rvb_launch_path_group(&a, 1, s);
        return;
    }
    const unsigned blocks = (unsigned) ((a.nrays + QUADS_PER_BLOCK - 1) / QUADS_PER_BLOCK);
    const bool seven = a.nrays <= 7ull * 1024ull * QUADS_PER_BLOCK;      // fits in seven waves per SIMD: the 72-register build
    launch_by_surfaces(seven ? path_kernel<true, 7> : path_kernel<true, 8>, seven ? path_kernel<false, 7> : path_kernel<false, 8>,
                       a.lds_surfaces, blocks, TraceLds::make(a.stack_entries, a.lds_surfaces, 4, a.sort_keys16 != nullptr).bytes, s, a);
}

// (the caller checked: every trace has the same lane count, stack depth, number of surfaces staged in LDS and key form)
void rvb_launch_path_group(const TraceArgs * traces, uint32_t count, hipStream_t s)
{
    TraceGroup g;
    g.count = count;
    const TraceArgs & a = traces[0];
    const uint32_t rays_per_block = WAVE / a.path_lanes;                 // 64 (one lane per ray) or 32
    uint32_t blocks = 0;
    for (uint32_t k = 0; k < count; ++k) {
        g.first_block[k] = blocks;
        g.trace[k] = traces[k];
        blocks += (uint32_t) ((traces[k].nrays + rays_per_block - 1) / rays_per_block);
    }
    for (uint32_t k = count; k <= RVB_MAX_GROUP; ++k) g.first_block[k] = blocks;
    for (uint32_t k = count; k < RVB_MAX_GROUP; ++k) g.trace[k] = traces[0];
    size_t lds = 0;                          // (the largest of the traces', should a caller ever group traces whose layouts differ in size)
    for (uint32_t k = 0; k < count; ++k) lds = std::max(lds, TraceLds::make(traces[k].stack_entries, traces[k].lds_surfaces, a.path_lanes, traces[k].sort_keys16 != nullptr).bytes);
    if (a.path_lanes == 1) launch_by_surfaces(path_lane_group_kernel<true>, path_lane_group_kernel<false>, a.lds_surfaces, blocks, lds, s, g);
    else launch_by_surfaces(path_pair_group_kernel<true>, path_pair_group_kernel<false>, a.lds_surfaces, blocks, lds, s, g);
}
