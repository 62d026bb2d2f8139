// shadow_kernels.hip — the SHADOW stage of the trace, reference rayverb/kernel.cpp:463-490 (path stage: trace_kernels.hip, image-source
// stage: image_kernels.hip, shared device code: traversal.h).
//   shadow_pair_kernel (shadow_kernel, shadow_lane_kernel: the four-lane and one-lane forms, kept for measurements)
//                  two lanes per (ray, bounce): the diffuse shadow ray to the microphone and the final Impulse.
//                  nrays*nreflections independent any-hit queries: this is where the chip fills up.
#include "traversal.h"

#include <algorithm>
#include <cstdlib>

namespace {

// The shadow rays as Jobs: a quad walks the work records g, g + stride, ...; next() loads a record
// (the quad reads its 64 bytes as one line, lane c = chunk c) and aims at the microphone
// (kernel.cpp:463-469), done() finishes the Impulse in place (kernel.cpp:471-490).
template <bool SURF_LDS>
struct ShadowJob {
    const TraceArgs & a;
    uint32_t c;
    uint64_t g, stride, total;
    v3 mic;
    float airA, airB;                    // bands 2c, 2c+1: every lane evaluates two of the eight attenuations
    float4 * rec;
    float4 mine;
    v3 p;
    float diff, new_dist, mag;
    uint32_t surface;
    float tmin, tmax_seen;               // arrival-time range of the non-zero impulses this lane's quad produced
    bool live;                           // the record that done() finished carries volume
    uint32_t pair;                       // pair of the current record (several pairs per launch only)
    lds_float4_ptr surf_lds;             // surface table in LDS; unused when !SURF_LDS
    uint32_t skip;                       // own-plane subtree of the triangle the shadow ray starts on, RVB_BVH_EMPTY = none

    __device__ __forceinline__ uint32_t skip_ref() const { return skip; }
    __device__ __forceinline__ bool next(v3 & o_, v3 & d_, float & tmax)
    {
        while (g < total) {
            // with a.sort_order the quads of a wave take consecutive records of one bucket: shadow rays that
            // start within one triangle and all aim at the microphone walk the same BVH nodes
            rec = reinterpret_cast<float4 *>(a.impulses + (a.sort_order ? (uint64_t) a.sort_order[g] : g));
            g += stride;
            mine = load_stream(rec + c);
            // chunk 3 = (newDist, surface, triangle, valid); chunk 2 = (intersection, DIFF)
            const uint32_t tag = quad_bcast_u<3>(__float_as_uint(mine.w));
            if (tag == 0u)
                continue;                         // ray had already escaped: slot keeps its zero fill
            if (a.npairs > 1) {                   // the record's pair: its microphone, its time range
                const float4 m4 = a.pair_mics[tag - 1u];
                mic = mk3(m4.x, m4.y, m4.z);
                pair = tag - 1u;
            }
            new_dist = quad_bcast_f<3>(mine.x);
            const float threshold = quad_bcast_f<3>(mine.y);
            // the triangle's shading record (the quad's lanes read the same 32 bytes): surface, and the own-plane skip
            const float4 * shade = reinterpret_cast<const float4 *>(a.scene.shade + quad_bcast_u<3>(__float_as_uint(mine.z)));
            const float4 sh = shade[0];
            const uint32_t skip_ref = __float_as_uint(shade[1].x);
            surface = __float_as_uint(sh.w);
            p = mk3(quad_bcast_f<2>(mine.x), quad_bcast_f<2>(mine.y), quad_bcast_f<2>(mine.z));
            diff = quad_bcast_f<2>(mine.w);
            const v3 b2p = mic - p;               // kernel.cpp:282-286
            mag = length3(b2p);
            o_ = p;
            d_ = normalize3(b2p);
            tmax = mag;
            skip = fabsf(dot3(mk3(sh.x, sh.y, sh.z), d_)) > threshold ? skip_ref : RVB_BVH_EMPTY;
            return true;
        }
        return false;
    }
    __device__ __forceinline__ void done(bool blocked, const Hit &)
    {
        const bool visible = !blocked;
        const float dist = visible ? new_dist + mag : 0.0f;          // kernel.cpp:471
        float4 o = make_float4(0, 0, 0, 0);
        // attenuation of bands 2c, 2c+1 in this lane; lanes 0/1 then collect bands 0-3 / 4-7 by DPP
        float eA = 0.0f, eB = 0.0f;
        if (visible) {
            eA = air_attenuation(dist, airA) * 1.0f;
            eB = air_attenuation(dist, airB) * 1.0f;
        }
        const float e0 = dpp_f<0xE8>(eA), e1 = dpp_f<0xE8>(eB);     // quad_perm [0,2,2,3]: lane 0 <- 0, lane 1 <- 2
        const float e2 = dpp_f<0xED>(eA), e3 = dpp_f<0xED>(eB);     // quad_perm [1,3,2,3]: lane 0 <- 1, lane 1 <- 3
        if (c < 2) {
            if (visible) {
                const float4 dc = surface_row<SURF_LDS>(a, surf_lds, surface, 2 + c);      // diffuse coefficients of this lane's four bands
                o.x = band_product(mine.x, e0, dc.x, diff);
                o.y = band_product(mine.y, e1, dc.y, diff);
                o.z = band_product(mine.z, e2, dc.z, diff);
                o.w = band_product(mine.w, e3, dc.w, diff);
            }
        } else if (c == 2) {
            o = make_float4(p.x, p.y, p.z, 0.0f);
        } else {
            o.x = seconds_per_meter() * dist;                        // kernel.cpp:489
        }
        store_stream(rec + c, o);
        // inputs of findPredelay / MAX_SAMPLE (rayverb.h:49-74, rayverb.cpp:54-57) for free: an impulse
        // takes part iff any band is non-zero (kernel.cpp:524)
        const bool nonzero = quad_any(c < 2 && (o.x != 0.0f || o.y != 0.0f || o.z != 0.0f || o.w != 0.0f));
        note_time(a, nonzero, c == 0, pair, seconds_per_meter() * dist, tmin, tmax_seen);
        live = nonzero;
        if (a.npairs > 1 && nonzero && c == 0) live_count_of_pair(a, pair);
    }
};

template <bool SURF_LDS>
__global__ __launch_bounds__(WAVE, RVB_SHADOW_WAVES) void shadow_kernel(TraceArgs a)
{
    extern __shared__ __attribute__((aligned(16))) uint32_t stack_lds[];   // [stack_entries][QUADS_PER_BLOCK]
    const uint32_t c = threadIdx.x & 3u;
    const uint32_t q = threadIdx.x >> 2;
    ShadowJob<SURF_LDS> job = {a};
    job.c = c;
    job.g = (uint64_t) blockIdx.x * QUADS_PER_BLOCK + q;
    job.stride = (uint64_t) gridDim.x * QUADS_PER_BLOCK;
    job.total = a.nrays * (uint64_t) a.nreflections;
    job.mic = ld3(a.mic);
    job.pair = 0;
    job.airA = a.air[2 * c];
    job.airB = a.air[2 * c + 1];
    job.tmin = __builtin_inff();
    job.tmax_seen = 0.0f;
    job.surf_lds = stage_surfaces(a, TraceLds::make(a.stack_entries, a.lds_surfaces, 4, false).surfaces(stack_lds));
    job.skip = RVB_BVH_EMPTY;
    // one record per quad per pass: the 16 quads of the wave start and finish a pass together
    v3 o, d;
    float tmax;
    uint32_t live = 0;
    while (job.next(o, d, tmax)) {
        Hit h;
        const bool blocked = traverse_quad<true>(a.scene, o, d, tmax, stack_lds + q, h, job.skip);
        job.done(blocked, h);
        live_count_step(a, job.live && c == 0, live);
    }
    time_range_of_wave(a, job.tmin, job.tmax_seen);
    live_count_of_wave(a, live);
}

// shadow_kernel with two lanes per record: lane 0 carries chunks 0 and 2 of the 64-byte record (bands 0-3; hit point, DIFF), lane 1
// chunks 1 and 3 (bands 4-7; distance, own-plane threshold, triangle, tag).  Each lane evaluates the four attenuations of its bands.
template <bool SURF_LDS>
__global__ __launch_bounds__(WAVE, RVB_SHADOW_PAIR_WAVES) void shadow_pair_kernel(TraceArgs a)
{
    extern __shared__ __attribute__((aligned(16))) uint32_t stack_lds[];   // [stack_entries][PAIRS_PER_BLOCK]
    const uint32_t h = threadIdx.x & 1u;
    const uint32_t q = threadIdx.x >> 1;
    uint32_t * stack = stack_lds + q;
    const lds_float4_ptr surf_lds = stage_surfaces(a, TraceLds::make(a.stack_entries, a.lds_surfaces, 2, false).surfaces(stack_lds));
    const uint64_t stride = (uint64_t) gridDim.x * PAIRS_PER_BLOCK, total = a.nrays * (uint64_t) a.nreflections;
    v3 mic = ld3(a.mic);
    const float air0 = a.air[4 * h], air1 = a.air[4 * h + 1], air2 = a.air[4 * h + 2], air3 = a.air[4 * h + 3];
    float tmin = __builtin_inff(), tmax_seen = 0.0f;
    uint32_t live = 0, nonzero = 0;             // live records of this wave so far (live_count_step); this record's verdict
    for (uint64_t g = (uint64_t) blockIdx.x * PAIRS_PER_BLOCK + q; g < total; g += stride, live_count_step(a, nonzero && h == 0, live)) {
        nonzero = 0u;
        float4 * rec = reinterpret_cast<float4 *>(a.impulses + (a.sort_order ? (uint64_t) a.sort_order[g] : g));
        const float4 vol = load_stream(rec + h), aux = load_stream(rec + h + 2);
        // (from here to `skip` the three kernels differ in the gathers only; a shared aim helper moved instructions in this one and in shadow_kernel)
        const uint32_t tag = dpp_u<QP_PAIR_HI>(__float_as_uint(aux.w));
        if (tag == 0u)
            continue;                             // ray had already escaped: slot keeps its zero fill
        uint32_t pair = 0;
        if (a.npairs > 1) {
            const float4 m4 = a.pair_mics[tag - 1u];
            mic = mk3(m4.x, m4.y, m4.z);
            pair = tag - 1u;
        }
        const float new_dist = dpp_f<QP_PAIR_HI>(aux.x), threshold = dpp_f<QP_PAIR_HI>(aux.y);
        const float4 * shade = reinterpret_cast<const float4 *>(a.scene.shade + dpp_u<QP_PAIR_HI>(__float_as_uint(aux.z)));
        const float4 sh = shade[0];
        const uint32_t skip_ref = __float_as_uint(shade[1].x);
        const uint32_t surface = __float_as_uint(sh.w);
        const v3 p = mk3(dpp_f<QP_PAIR_LO>(aux.x), dpp_f<QP_PAIR_LO>(aux.y), dpp_f<QP_PAIR_LO>(aux.z));
        const float diff = dpp_f<QP_PAIR_LO>(aux.w);
        const v3 b2p = mic - p;                   // kernel.cpp:282-286
        const float mag = length3(b2p);
        const v3 dir = normalize3(b2p);
        const uint32_t skip = fabsf(dot3(mk3(sh.x, sh.y, sh.z), dir)) > threshold ? skip_ref : RVB_BVH_EMPTY;
        const bool visible = !traverse_pair_any(a.scene, p, dir, mag, stack, skip);
        const float dist = visible ? new_dist + mag : 0.0f;          // kernel.cpp:471
        float4 o = make_float4(0, 0, 0, 0);
        if (visible) {
            const float4 dc = surface_row<SURF_LDS>(a, surf_lds, surface, 2 + h);      // diffuse coefficients of this lane's four bands
            o.x = band_product(vol.x, air_attenuation(dist, air0) * 1.0f, dc.x, diff);
            o.y = band_product(vol.y, air_attenuation(dist, air1) * 1.0f, dc.y, diff);
            o.z = band_product(vol.z, air_attenuation(dist, air2) * 1.0f, dc.z, diff);
            o.w = band_product(vol.w, air_attenuation(dist, air3) * 1.0f, dc.w, diff);
        }
        const float t = seconds_per_meter() * dist;                  // kernel.cpp:489
        store_stream(rec + h, o);
        store_stream(rec + h + 2, h == 0 ? make_float4(p.x, p.y, p.z, 0.0f) : make_float4(t, 0.0f, 0.0f, 0.0f));
        // inputs of findPredelay / MAX_SAMPLE (rayverb.h:49-74, rayverb.cpp:54-57): an impulse takes part iff any band is non-zero
        nonzero = (o.x != 0.0f || o.y != 0.0f || o.z != 0.0f || o.w != 0.0f) ? 1u : 0u;
        nonzero |= dpp_u<QP_SWAP1>(nonzero);
        if (nonzero) {
            if (a.npairs > 1) {
                if (h == 0) {       // time_range_of_pair, written out: through the helper this kernel's registers are allocated differently
                    const volatile uint32_t * seen = a.time_range + 2u * pair;
                    if (t != 0.0f && __float_as_uint(t) < seen[0]) atomicMin(a.time_range + 2u * pair, __float_as_uint(t));
                    if (__float_as_uint(t) > seen[1]) atomicMax(a.time_range + 2u * pair + 1u, __float_as_uint(t));
                    live_count_of_pair(a, pair);
                }
            } else {
                if (t != 0.0f) tmin = fminf(tmin, t);
                tmax_seen = fmaxf(tmax_seen, t);
            }
        }
    }
    time_range_of_wave(a, tmin, tmax_seen);
    live_count_of_wave(a, live);
}

// shadow_pair_kernel with ONE lane per record (round 4, RVB_SHADOW_LANES=1): 64 records per wave pass, every lane walks its own any-hit
// query — four children and up to four triangles per step — with its own LDS stack column, nothing exchanged between lanes.  The records of
// a wave are neighbours in grouped order (same wall, same microphone), so unlike the path kernel's rays the lanes read mostly the SAME
// nodes: few distinct lines per load instruction.  Same operations on the same values as the pair kernel: same bytes
// (tests/test_gpu_parity.py::test_quad_shadow_kernel_gives_the_same_bytes runs it in a child process).  MEASURED at workload C2
// (profiles/r04_shadow_lanes_n1.txt): 2.12 ms against 1.26 (pairs) and 1.47 (quads) per 100 k rays x 128, the bench pipeline 5.40 against
// 4.42 ms per IR — like the one-lane path kernel it pays for its shorter instruction stream in 16-byte-per-lane loads (a leaf step alone is
// twelve of them per lane).  Kept for measurements only; the shipped form is two lanes per record.
template <bool SURF_LDS>
__global__ __launch_bounds__(WAVE, RVB_LANE_WAVES) void shadow_lane_kernel(TraceArgs a)
{
    extern __shared__ __attribute__((aligned(16))) uint32_t stack_lds[];   // [stack_entries + 1][64], surface table
    const uint32_t lane = threadIdx.x;
    const lds_float4_ptr surf_lds = stage_surfaces(a, TraceLds::make(a.stack_entries, a.lds_surfaces, 1, false).surfaces(stack_lds));
    const uint64_t stride = (uint64_t) gridDim.x * LANE_RAYS, total = a.nrays * (uint64_t) a.nreflections;
    const char * node_base = reinterpret_cast<const char *>(a.scene.nodes);
    const char * tri_base = reinterpret_cast<const char *>(a.scene.tris);
    const float neg_cull = -a.scene.cull_abs;
    const lds_u32_ptr bottom = (lds_u32_ptr) stack_lds + lane;
    v3 mic = ld3(a.mic);
    float tmin = __builtin_inff(), tmax_seen = 0.0f;
    uint32_t live = 0;
    bool nonzero = false;
    for (uint64_t g = (uint64_t) blockIdx.x * LANE_RAYS + lane; g < total; g += stride, live_count_step(a, nonzero, live)) {
        nonzero = false;
        float4 * rec = reinterpret_cast<float4 *>(a.impulses + (a.sort_order ? (uint64_t) a.sort_order[g] : g));
        const float4 vol_lo = load_stream(rec + 0), vol_hi = load_stream(rec + 1), geo = load_stream(rec + 2), aux = load_stream(rec + 3);
        const uint32_t tag = __float_as_uint(aux.w);
        if (tag == 0u)
            continue;                             // ray had already escaped: slot keeps its zero fill
        uint32_t pair = 0;
        if (a.npairs > 1) {
            const float4 m4 = a.pair_mics[tag - 1u];
            mic = mk3(m4.x, m4.y, m4.z);
            pair = tag - 1u;
        }
        const float new_dist = aux.x, threshold = aux.y;
        const float4 * shade = reinterpret_cast<const float4 *>(a.scene.shade + __float_as_uint(aux.z));
        const float4 sh = shade[0];
        const uint32_t skip_ref = __float_as_uint(shade[1].x);
        const uint32_t surface = __float_as_uint(sh.w);
        const v3 p = mk3(geo.x, geo.y, geo.z);
        const float diff = geo.w;
        const v3 b2p = mic - p;                   // kernel.cpp:282-286
        const float mag = length3(b2p);
        const v3 dir = normalize3(b2p);
        const uint32_t skip = fabsf(dot3(mk3(sh.x, sh.y, sh.z), dir)) > threshold ? skip_ref : RVB_BVH_EMPTY;
        // any hit with EPSILON < distance <= mag? (traverse_pair_any with one lane: the lowest hit child is entered, the others pushed; the
        // steps are path_lane_body's, written out in both: every shared helper tried moved instructions in one of the two kernels)
        bool blocked = false;
        {
            const float limit = fmaf(mag, 1.0f + a.scene.cull_rel, a.scene.cull_abs);
            const float ix = clamp_inv(dir.x), iy = clamp_inv(dir.y), iz = clamp_inv(dir.z);
            const float oix = p.x * ix, oiy = p.y * iy, oiz = p.z * iz;
            const uint32_t selx = slab_selector(ix), sely = slab_selector(iy), selz = slab_selector(iz);
            lds_u32_ptr sp = bottom;
            uint32_t ref = 0;
            for (;;) {
                while (!(ref & RVB_BVH_LEAF)) {
                    const uint4 * np = reinterpret_cast<const uint4 *>(node_base + ref);
                    const uint4 n0 = np[0], n1 = np[1], n2 = np[2], n3 = np[3];
                    float tn;
                    const bool ok0 = slab_select(n0, ix, iy, iz, oix, oiy, oiz, selx, sely, selz, limit, neg_cull, skip, tn);
                    const bool ok1 = slab_select(n1, ix, iy, iz, oix, oiy, oiz, selx, sely, selz, limit, neg_cull, skip, tn);
                    const bool ok2 = slab_select(n2, ix, iy, iz, oix, oiy, oiz, selx, sely, selz, limit, neg_cull, skip, tn);
                    const bool ok3 = slab_select(n3, ix, iy, iz, oix, oiy, oiz, selx, sely, selz, limit, neg_cull, skip, tn);
                    // the lowest hit child is entered; the others go on the stack in child order (store, then advance if kept)
                    const bool first0 = ok0, first1 = ok1 && !ok0, first2 = ok2 && !(ok0 || ok1), first3 = ok3 && !(ok0 || ok1 || ok2);
                    *sp = n1.w; sp += (ok1 && !first1) ? LANE_RAYS : 0;
                    *sp = n2.w; sp += (ok2 && !first2) ? LANE_RAYS : 0;
                    *sp = n3.w; sp += (ok3 && !first3) ? LANE_RAYS : 0;
                    if (first0) ref = n0.w;
                    else if (first1) ref = n1.w;
                    else if (first2) ref = n2.w;
                    else if (first3) ref = n3.w;
                    else if (sp != bottom) { sp -= LANE_RAYS; ref = *sp; }
                    else ref = NONE;
                }
                if (ref == NONE)
                    break;
                const uint32_t first = ref & 0x0FFFFFFFu;
                const uint32_t count = ((ref >> 28) & 7u) + 1u;
                const float4 * tp0 = reinterpret_cast<const float4 *>(tri_base + tri_byte_offset(first));
                const float4 * tp1 = reinterpret_cast<const float4 *>(tri_base + tri_byte_offset(first + (1u < count ? 1u : 0u)));
                const float4 * tp2 = reinterpret_cast<const float4 *>(tri_base + tri_byte_offset(first + (2u < count ? 2u : 0u)));
                const float4 * tp3 = reinterpret_cast<const float4 *>(tri_base + tri_byte_offset(first + (3u < count ? 3u : 0u)));
                float4 ta = tp0[0], tb = tp0[1], tc = tp0[2], ua = tp1[0], ub = tp1[1], uc = tp1[2];
                float4 va = tp2[0], vb = tp2[1], vc = tp2[2], wa = tp3[0], wb = tp3[1], wc = tp3[2];
                asm volatile("" : "+v"(ta.x), "+v"(tb.x), "+v"(tc.x), "+v"(ua.x), "+v"(ub.x), "+v"(uc.x),
                                  "+v"(va.x), "+v"(vb.x), "+v"(vc.x), "+v"(wa.x), "+v"(wb.x), "+v"(wc.x));
                const float dist0 = mt_intersect(mk3(ta.x, ta.y, ta.z), mk3(ta.w, tb.x, tb.y), mk3(tb.z, tb.w, tc.x), p, dir);
                const float dist1 = mt_intersect(mk3(ua.x, ua.y, ua.z), mk3(ua.w, ub.x, ub.y), mk3(ub.z, ub.w, uc.x), p, dir);
                const float dist2 = mt_intersect(mk3(va.x, va.y, va.z), mk3(va.w, vb.x, vb.y), mk3(vb.z, vb.w, vc.x), p, dir);
                const float dist3 = mt_intersect(mk3(wa.x, wa.y, wa.z), mk3(wa.w, wb.x, wb.y), mk3(wb.z, wb.w, wc.x), p, dir);
                if ((dist0 > RVB_EPSILON && dist0 <= mag) || (1u < count && dist1 > RVB_EPSILON && dist1 <= mag)
                    || (2u < count && dist2 > RVB_EPSILON && dist2 <= mag) || (3u < count && dist3 > RVB_EPSILON && dist3 <= mag)) {
                    blocked = true;
                    break;
                }
                if (sp != bottom) { sp -= LANE_RAYS; ref = *sp; } else break;
            }
        }
        const bool visible = !blocked;
        const float dist = visible ? new_dist + mag : 0.0f;          // kernel.cpp:471
        float4 o_lo = make_float4(0, 0, 0, 0), o_hi = o_lo;
        if (visible) {
            const float4 d_lo = surface_row<SURF_LDS>(a, surf_lds, surface, 2), d_hi = surface_row<SURF_LDS>(a, surf_lds, surface, 3);      // diffuse coefficients
            o_lo.x = band_product(vol_lo.x, air_attenuation(dist, a.air[0]) * 1.0f, d_lo.x, diff);
            o_lo.y = band_product(vol_lo.y, air_attenuation(dist, a.air[1]) * 1.0f, d_lo.y, diff);
            o_lo.z = band_product(vol_lo.z, air_attenuation(dist, a.air[2]) * 1.0f, d_lo.z, diff);
            o_lo.w = band_product(vol_lo.w, air_attenuation(dist, a.air[3]) * 1.0f, d_lo.w, diff);
            o_hi.x = band_product(vol_hi.x, air_attenuation(dist, a.air[4]) * 1.0f, d_hi.x, diff);
            o_hi.y = band_product(vol_hi.y, air_attenuation(dist, a.air[5]) * 1.0f, d_hi.y, diff);
            o_hi.z = band_product(vol_hi.z, air_attenuation(dist, a.air[6]) * 1.0f, d_hi.z, diff);
            o_hi.w = band_product(vol_hi.w, air_attenuation(dist, a.air[7]) * 1.0f, d_hi.w, diff);
        }
        const float t = seconds_per_meter() * dist;                  // kernel.cpp:489
        store_stream(rec + 0, o_lo);
        store_stream(rec + 1, o_hi);
        store_stream(rec + 2, make_float4(p.x, p.y, p.z, 0.0f));
        store_stream(rec + 3, make_float4(t, 0.0f, 0.0f, 0.0f));
        nonzero = o_lo.x != 0.0f || o_lo.y != 0.0f || o_lo.z != 0.0f || o_lo.w != 0.0f
               || o_hi.x != 0.0f || o_hi.y != 0.0f || o_hi.z != 0.0f || o_hi.w != 0.0f;
        note_time(a, nonzero, true, pair, t, tmin, tmax_seen);
        if (a.npairs > 1 && nonzero) live_count_of_pair(a, pair);
    }
    time_range_of_wave(a, tmin, tmax_seen);
    live_count_of_wave(a, live);
}

// One wave behind a shadow kernel: pair by pair, lane t takes the stripes t, t + 64, ... of a.live_stripes — their partial counts, which
// it puts back to zero for the next launch — and the wave's sum is the pair's count, written (not added) behind the launch's time
// ranges.  (One wave, not a workgroup of 1024: in the pipeline, beside the other contexts' path kernels, sixteen waves that must fit
// one CU together waited 47 us for their place.)
__global__ __launch_bounds__(WAVE) void live_sum_kernel(uint32_t * __restrict__ stripes, uint32_t npairs, uint32_t * __restrict__ counts)
{
    for (uint32_t pair = 0; pair < npairs; ++pair) {
        uint32_t sum = 0;
        for (uint32_t stripe = threadIdx.x; stripe < RVB_LIVE_STRIPES; stripe += WAVE) {
            sum += stripes[stripe * npairs + pair];
            stripes[stripe * npairs + pair] = 0u;
        }
        for (int off = 32; off > 0; off >>= 1)
            sum += (uint32_t) __shfl_xor((int) sum, off);
        if (threadIdx.x == 0) counts[pair] = sum;
    }
}

}  // namespace

// Two lanes per record by default (shadow_pair_kernel): 12.8 M records fill the chip whatever the lane count, and a record costs
// 12 % less (C2: 1.45 -> 1.28 ms).  RVB_SHADOW_LANES=4 keeps the quad kernel (measurements).
uint32_t rvb_shadow_lanes()
{
    static const int lanes = getenv("RVB_SHADOW_LANES") ? atoi(getenv("RVB_SHADOW_LANES")) : 2;
    return lanes == 4 ? 4u : (lanes == 1 ? 1u : 2u);
}

void rvb_launch_shadow(const TraceArgs & a, hipStream_t s)
{
    const uint64_t total = a.nrays * (uint64_t) a.nreflections;
    if (total == 0) return;
    // single-wave workgroups per CU (RVB_SHADOW_WG_PER_CU, else the kernel's default); records beyond are grid-strided
    static const char * const per_cu_env = getenv("RVB_SHADOW_WG_PER_CU");
    static const uint64_t per_cu_set = per_cu_env ? strtoull(per_cu_env, nullptr, 10) : 0;
    const uint32_t lanes = rvb_shadow_lanes();
    const TraceLds layout = TraceLds::make(a.stack_entries, a.lds_surfaces, lanes, false);       // (no key runs: the path stage's)
    const uint32_t per_block = layout.rays;                                                      // records per workgroup
    const uint64_t per_cu = per_cu_env ? per_cu_set : (lanes == 1 ? 128 : 256);
    const uint64_t blocks = std::min<uint64_t>((total + per_block - 1) / per_block, 256u * per_cu);
    const size_t lds = layout.bytes;
    if (lanes == 1) launch_by_surfaces(shadow_lane_kernel<true>, shadow_lane_kernel<false>, a.lds_surfaces, blocks, lds, s, a);
    else if (lanes == 2) launch_by_surfaces(shadow_pair_kernel<true>, shadow_pair_kernel<false>, a.lds_surfaces, blocks, lds, s, a);
    else launch_by_surfaces(shadow_kernel<true>, shadow_kernel<false>, a.lds_surfaces, blocks, lds, s, a);
    const uint32_t npairs = a.npairs > 1 ? a.npairs : 1u;
    hipLaunchKernelGGL(live_sum_kernel, dim3(1), dim3(WAVE), 0, s, a.live_stripes, npairs, a.time_range + 2u * npairs);
}
