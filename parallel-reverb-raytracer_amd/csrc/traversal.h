// traversal.h — device code that more than one trace stage uses (trace_kernels.hip: the path stage, image_kernels.hip: image-source
// validation, shadow_kernels.hip: the shadow stage): the build knobs, the slab and triangle steps, the traversal loops over one 4-wide
// BVH, the LDS layout of a trace workgroup (TraceLds: the kernels' offsets and the launchers' byte counts).
//
// Lane-cooperative traversal: the lanes of a ray own the four children of a node (one contiguous 64-byte
// half line per visit, 16-byte loads) and the up-to-four triangles of a leaf; they combine results with
// DPP quad_perm moves (quad.h), never through memory.  (Nodes are 64 bytes: binary16 boxes rounded outward.)  The
// per-ray stack lives in LDS, 4 bytes per entry.  Every triangle test is the reference's Möller–Trumbore
// arithmetic (rvb_math.h); the BVH only prunes, so a query returns the brute-force answer.
#pragma once

#include "kernels.h"
#include "quad.h"
#include "rvb_math.h"

// ---- build knobs: single numbers (tools/build_variant.sh runs set them) and the two diagnostic builds; everything else is the shipped form ----
// step thresholds of the path kernels' schedule (traverse_jobs_cycle, traverse_pairs_cycle: "THE SCHEDULE")
#ifndef RVB_CYCLE_LEAF_NUM
#define RVB_CYCLE_LEAF_NUM 3       // a leaf step when NUM x (lanes at a leaf) >= DEN x (live lanes)
#define RVB_CYCLE_LEAF_DEN 1
#endif
#ifndef RVB_CYCLE_DONE_NUM
#define RVB_CYCLE_DONE_NUM 4       // a shading step when NUM x (lanes with a finished query) >= DEN x (live lanes)
#define RVB_CYCLE_DONE_DEN 1
#endif
// waves per SIMD the register budget of a kernel allows (its __launch_bounds__)
#ifndef RVB_PAIR_WAVES
#define RVB_PAIR_WAVES 6            // path_pair_group_kernel: 80 VGPRs, so that six waves fit a SIMD beside the other kernels' (see the node step of traverse_pairs_cycle);
                                    // 7 (72 VGPRs) spills ten registers: pipeline 4.52-4.54 ms against 4.37-4.40, and 4.70 against 4.47 when LDS
                                    // allows the seventh wave too (no key runs: profiles/r04c_occupancy_n1.txt); 8 (64 VGPRs): 5.9 ms
#endif
#ifndef RVB_SHADOW_PAIR_WAVES
#define RVB_SHADOW_PAIR_WAVES 5     // shadow_pair_kernel
#endif
#ifndef RVB_SHADOW_WAVES
#define RVB_SHADOW_WAVES 8          // shadow_kernel: 64 VGPRs (8 waves/SIMD): 1.845 -> 1.807 ms against 7
#endif
#ifndef RVB_LANE_WAVES
#define RVB_LANE_WAVES 4            // path_lane_group_kernel, shadow_lane_kernel: 128 VGPRs
#endif
// tools/isa_mix.py: -DRVB_ISA_MARKS=1 leaves comment lines in the ISA at the borders of the step kinds of the path loops (never in the shipped build)
#ifndef RVB_ISA_MARKS
#define RVB_ISA_MARKS 0
#endif
#if RVB_ISA_MARKS
#define RVB_MARK(name) asm volatile("; RVB_MARK " name)
#else
#define RVB_MARK(name)
#endif
// tools/pair_stamps.py: -DRVB_STAMPS=1 (never shipped) stamps the traversal loops with s_memtime, see STAMP below
#ifndef RVB_STAMPS
#define RVB_STAMPS 0
#endif

#define WAVE 64
#define QUADS_PER_BLOCK 16          // rays (or records) per 64-lane workgroup in the quad kernels
#define NONE 0xFFFFFFFFu
#define PAIRS_PER_BLOCK 32          // ... in the two-lane kernels
#define LANE_RAYS 64                // ... in the one-lane kernels
#define RVB_KEY_RUN 32u             // grouping keys per run (PathJob, trace_kernels.hip): 32 x 2 bytes = one 64-byte segment

namespace {

// Diagnostic build only (-DRVB_STAMPS=1, never shipped): per-wave s_memtime shares of the traversal
// loop, written to a side buffer that no other code reads (cdna_hip_programming.md §7 "In-kernel stamps").
#if RVB_STAMPS
#define STAMP(var) { __builtin_amdgcn_sched_barrier(0); var = __builtin_amdgcn_s_memtime(); __builtin_amdgcn_s_waitcnt(0xC07F); __builtin_amdgcn_sched_barrier(0); }
struct Stamps {
    unsigned long long node_steps = 0, node_cycles = 0, leaf_steps = 0, leaf_cycles = 0, done_calls = 0, done_cycles = 0;
    unsigned long long quad_node_steps = 0, quad_leaf_steps = 0, t0 = 0;
};
#else
#define STAMP(var)
#endif

struct Hit { float t; uint32_t tri; };

// Streaming accesses to the 64-byte work records / Impulses (written once, read once by a later kernel): non-temporal, the lines stay in
// the XCD's L2 until evicted (the write-through forms sc1 / sc0 sc1 of the stores were measured and are no faster: DESIGN.md §3).
typedef float nt_float4 __attribute__((ext_vector_type(4)));
typedef __attribute__((address_space(3))) uint32_t * lds_u32_ptr;
typedef __attribute__((address_space(3))) const nt_float4 * lds_float4_ptr;  // keeps ds_read: a generic pointer would load flat
__device__ __forceinline__ void store_stream(float4 * p, const float4 v)
{
    nt_float4 t = {v.x, v.y, v.z, v.w};
    __builtin_nontemporal_store(t, reinterpret_cast<nt_float4 *>(p));
}
__device__ __forceinline__ float4 load_stream(const float4 * p)
{
    const nt_float4 t = __builtin_nontemporal_load(reinterpret_cast<const nt_float4 *>(p));
    return make_float4(t.x, t.y, t.z, t.w);
}

// Inverse direction for the (conservative, padded) slab test only — never used by a triangle test,
// so the 1-ulp hardware reciprocal is enough.  Clamped to +-2^97: with coordinates up to 2^30 (rvb_build_scene's limit) the product
// o * inv stays finite (2^127), and so does a binary16 plane times inv (< 2^113).  A larger clamp (1e30 until the constructed scenes
// of tests/bvh_edges.py) made o * inv infinite above |o| = 3.4e8 for a ray with a zero direction component; the min / max form of the
// slab test then rejected every box: fmaf(finite plane, inv, -inf) = -inf on one side, NaN on the saturated other.  With a power of
// two the product is exact, so for such a component the sign of fmaf(plane, inv, -o * inv) is the sign of plane - o.
__device__ __forceinline__ float clamp_inv(float d)
{
    float inv = __builtin_amdgcn_rcpf(d);         // +-inf for d == 0
    return fminf(fmaxf(inv, -0x1p97f), 0x1p97f);  // keeps 0 * inf out of the slab test
}

// byte offset of leaf-order triangle i < 2^24 (rvb_build_scene's limit): one full-rate 24-bit multiply
// (the 32-bit v_mul_lo_u32 the compiler picks for i * 48 is a quarter-rate instruction)
__device__ __forceinline__ uint32_t tri_byte_offset(uint32_t i) { return __umul24(i, (uint32_t) sizeof(BvhTri)); }

// Slab test of one child box, t = lo*inv - o*inv as one FMA per plane.  A child record is 16 bytes:
// six binary16 planes rounded outward by the builder + the child reference.  Boxes are padded
// (BuiltScene::pad) and `limit` carries the cull slack, so the test is conservative with respect to
// the float triangle test (the FMA form moves a plane by <2e-3 of the padding).
// Folded: tn = max(entry, -cull_abs), tf = min(exit, limit); hit iff tn <= tf.  Empty child slots
// are rejected by their ref (minNum/maxNum would swallow a NaN box: max(NaN, -cull) = -cull).
typedef _Float16 half2_t __attribute__((ext_vector_type(2)));
__device__ __forceinline__ half2_t as_half2(uint32_t u) { return __builtin_bit_cast(half2_t, u); }

// `skip`: a child reference the query must not enter (the own-plane subtree of the triangle the ray starts on, TriShade in bvh.h;
// RVB_BVH_EMPTY = none, which doubles as the test for an empty slot).
__device__ __forceinline__ bool slab(const uint4 n, const float ix, const float iy, const float iz,
                                     const float oix, const float oiy, const float oiz,
                                     const float limit, const float neg_cull, const uint32_t skip, float & tn)
{
    const half2_t h0 = as_half2(n.x), h1 = as_half2(n.y), h2 = as_half2(n.z);   // (lo.x, hi.x) (lo.y, hi.y) (lo.z, hi.z)
    const float tx0 = fmaf((float) h0.x, ix, -oix), tx1 = fmaf((float) h0.y, ix, -oix);
    const float ty0 = fmaf((float) h1.x, iy, -oiy), ty1 = fmaf((float) h1.y, iy, -oiy);
    const float tz0 = fmaf((float) h2.x, iz, -oiz), tz1 = fmaf((float) h2.y, iz, -oiz);
    // The two folds with loop-invariant operands are written as instructions: fmaxf / fminf would first canonicalise
    // `neg_cull` and `limit` (values from another basic block are not known to be quiet) — two more VALU operations per
    // node step.  Neither is ever NaN; v_max / v_min return the other operand for a NaN box plane like fmaxf / fminf.
    float zn = fminf(tz0, tz1), zf = fmaxf(tz0, tz1);
    asm("v_max_f32 %0, %1, %2" : "=v"(zn) : "s"(neg_cull), "v"(zn));      // wave-uniform: stays in an SGPR
    asm("v_min_f32 %0, %1, %2" : "=v"(zf) : "v"(zf), "v"(limit));
    tn = fmaxf(fmaxf(fminf(tx0, tx1), fminf(ty0, ty1)), zn);
    const float tf = fminf(fminf(fmaxf(tx0, tx1), fmaxf(ty0, ty1)), zf);
    return tn <= tf && n.w != RVB_BVH_EMPTY && n.w != skip;
}

// The same test with the near / far plane of each axis SELECTED by the sign of the direction instead of computed as min / max of
// both products: one v_perm_b32 per axis swaps the halves of the (lo, hi) word when the ray runs towards -axis, after which the low
// half is the plane the ray meets first.  3 selects + 2 three-operand min / max replace 6 two-operand min / max and the EMPTY compare
// (an empty slot is an inverted infinite box: entry +inf, exit -inf).  The products are monotonic in the plane, so entry and exit
// are bit-identical to slab()'s.  sel*: slab_selector(inverse direction), 3 more registers per query — used by the two-lane
// kernels, whose register budget is not the 64 of the quad kernels.
__device__ __forceinline__ uint32_t slab_selector(float inv) { return inv < 0.0f ? 0x01000302u : 0x03020100u; }
__device__ __forceinline__ bool slab_select(const uint4 n, const float ix, const float iy, const float iz,
                                            const float oix, const float oiy, const float oiz,
                                            const uint32_t selx, const uint32_t sely, const uint32_t selz,
                                            const float limit, const float neg_cull, const uint32_t skip, float & tn)
{
    const half2_t hx = as_half2(__builtin_amdgcn_perm(n.x, n.x, selx)), hy = as_half2(__builtin_amdgcn_perm(n.y, n.y, sely)),
                  hz = as_half2(__builtin_amdgcn_perm(n.z, n.z, selz));      // (near, far) per axis
    const float nx = fmaf((float) hx.x, ix, -oix), fx = fmaf((float) hx.y, ix, -oix);
    const float ny = fmaf((float) hy.x, iy, -oiy), fy = fmaf((float) hy.y, iy, -oiy);
    const float nz = fmaf((float) hz.x, iz, -oiz), fz = fmaf((float) hz.y, iz, -oiz);
    float zn = nz, zf = fz;
    asm("v_max_f32 %0, %1, %2" : "=v"(zn) : "s"(neg_cull), "v"(zn));      // (written as instructions: see slab)
    asm("v_min_f32 %0, %1, %2" : "=v"(zf) : "v"(zf), "v"(limit));
    tn = fmaxf(fmaxf(nx, ny), zn);
    const float tf = fminf(fminf(fx, fy), zf);
    return tn <= tf && n.w != skip;
}

// Closest hit (ANY = false): the brute-force winner of reference kernel.cpp:167-192.
// Any hit (ANY = true): is there a triangle with EPSILON < distance <= tmax — the negation of
// reference kernel.cpp:295 "(!inter.intersects) || inter.distance > mag".
//
// Persistent job loop: a quad asks its Job for a query (job.next), traverses, hands the result
// back (job.done) and immediately asks for the next one, while the other quads of the wave keep
// traversing their own queries.  No quad ever waits for the slowest ray of its wave at a bounce /
// record boundary; the wave ends when every quad has run out of jobs.
//   bool Job::next(v3 & o, v3 & d, float & tmax)   set up the quad's next query, false = none left
//   void Job::done(bool hit, const Hit & h)          consume the result (quad-uniform control flow)
// stack: this quad's column of the LDS stack, entries QUADS_PER_BLOCK words apart.
template <bool ANY, class Job>
__device__ __forceinline__ void traverse_jobs(const SceneDev & sc, uint32_t * __restrict__ stack, Job & job)
{
    const uint32_t c = threadIdx.x & 3u;          // the child / leaf triangle this lane owns
    const uint32_t lane_base4 = (threadIdx.x & 60u) << 2;         // ds_bpermute address of the quad's lane 0
    const uint32_t lane_bit = 1u << c, lt_mask = lane_bit - 1u;
    const char * node_base = reinterpret_cast<const char *>(sc.nodes);   // wave-uniform: the load is base (SGPRs) + 32-bit lane offset
    const uint32_t child_off = 16u * c;
    const float neg_cull = -sc.cull_abs, cull_scale = 1.0f + sc.cull_rel;
    v3 o = mk3(0, 0, 0), d = mk3(0, 0, 0);
    float tmax = 0.0f;
    float ix = 0.0f, iy = 0.0f, iz = 0.0f, oix = 0.0f, oiy = 0.0f, oiz = 0.0f, best_t = 0.0f;
    uint32_t best_i = NONE, sp = 0, ref = 0;
#if RVB_STAMPS
    Stamps st;
    unsigned long long ta = 0, tb = 0;
    STAMP(st.t0)
#endif
    bool active = job.next(o, d, tmax);
#define RESET_QUERY_JOBS()                                                \
    {                                                                     \
        ix = clamp_inv(d.x); iy = clamp_inv(d.y); iz = clamp_inv(d.z);    \
        oix = o.x * ix; oiy = o.y * iy; oiz = o.z * iz;                   \
        best_t = ANY ? tmax : __builtin_inff();                           \
        best_i = NONE; sp = 0; ref = 0;                                   \
    }
    if (active) RESET_QUERY_JOBS()
    while (active) {
        while (!(ref & RVB_BVH_LEAF)) {
            STAMP(ta)
#if RVB_STAMPS
            st.quad_node_steps += (threadIdx.x & 3u) == 0 ? 1 : 0;
#endif
            const uint4 n = *reinterpret_cast<const uint4 *>(node_base + (ref | child_off));
            const float limit = fmaf(best_t, cull_scale, sc.cull_abs);
            float tn;
            const bool ok = slab(n, ix, iy, iz, oix, oiy, oiz, limit, neg_cull, job.skip_ref(), tn);
            const uint32_t cref = n.w;
            // key = entry distance (two mantissa bits traded for the lane id): the quad minimum names
            // the nearest hit child and the lane that owns it in two DPP steps
            uint32_t key = ok ? ((__float_as_uint(fmaxf(tn, 0.0f)) & ~3u) | c) : NONE;
            if (ANY) key = ok ? c : NONE;         // any-hit does not care about visiting order
            uint32_t kmin = min(key, dpp_u<QP_SWAP1>(key));
            kmin = min(kmin, dpp_u<QP_SWAP2>(kmin));
            if (kmin == NONE) {
                if (sp > 0) { --sp; ref = stack[sp * QUADS_PER_BLOCK]; } else ref = NONE;
#if RVB_STAMPS
                STAMP(tb)
                st.node_steps += 1; st.node_cycles += tb - ta;
#endif
                continue;
            }
            const uint32_t winner = kmin & 3u;
            // the quad's hit mask by two DPP ORs (a 64-bit ballot shifted down per quad costs a 64-bit VALU shift)
            uint32_t okmask = ok ? lane_bit : 0u;
            okmask |= dpp_u<QP_SWAP1>(okmask);
            okmask |= dpp_u<QP_SWAP2>(okmask);
            const uint32_t rest = okmask & ~(1u << winner);
            if (ok && c != winner)
                stack[(sp + __popc(rest & lt_mask)) * QUADS_PER_BLOCK] = cref;
            sp += __popc(rest);
            ref = (uint32_t) __builtin_amdgcn_ds_bpermute((int) (lane_base4 + (winner << 2)), (int) cref);
#if RVB_STAMPS
            STAMP(tb)
            st.node_steps += 1; st.node_cycles += tb - ta;
#endif
        }
        STAMP(ta)
        bool finished = true, found = false;
        if (ref != NONE) {
            const uint32_t first = ref & 0x0FFFFFFFu;
            const uint32_t count = ((ref >> 28) & 7u) + 1u;
            float dist = 0.0f;
            uint32_t idx = NONE;
            if (c < count) {
                const float4 * tp = reinterpret_cast<const float4 *>(reinterpret_cast<const char *>(sc.tris) + tri_byte_offset(first + c));
                float4 ta = tp[0], tb = tp[1], tc = tp[2];
                // all three loads leave before the first use: without this the compiler sinks the v0 load below the
                // |det| test of mt_intersect and a leaf step pays two dependent round trips instead of one
                asm volatile("" : "+v"(ta.x), "+v"(tb.x), "+v"(tc.x));
                dist = mt_intersect(mk3(ta.x, ta.y, ta.z), mk3(ta.w, tb.x, tb.y), mk3(tb.z, tb.w, tc.x), o, d);
                idx = __float_as_uint(tc.y);
            }
            if (ANY) {
                found = quad_any(c < count && dist > RVB_EPSILON && dist <= tmax);
            } else {
                // kernel.cpp:180-188 — smallest distance wins, equal distances go to the lower index.
                // Lexicographic (distance, index) minimum over the quad's valid lanes.
                const bool valid = c < count && dist > RVB_EPSILON;
                float rd = valid ? dist : __builtin_inff();
                uint32_t ri = valid ? idx : NONE;
                {
                    const float od = dpp_f<QP_SWAP1>(rd);
                    const uint32_t oi = dpp_u<QP_SWAP1>(ri);
                    if (od < rd || (od == rd && oi < ri)) { rd = od; ri = oi; }
                }
                {
                    const float od = dpp_f<QP_SWAP2>(rd);
                    const uint32_t oi = dpp_u<QP_SWAP2>(ri);
                    if (od < rd || (od == rd && oi < ri)) { rd = od; ri = oi; }
                }
                if (ri != NONE && (best_i == NONE || rd < best_t || (rd == best_t && ri < best_i))) {
                    best_t = rd;
                    best_i = ri;
                }
            }
            if (!found && sp > 0) {
                --sp;
                ref = stack[sp * QUADS_PER_BLOCK];
                finished = false;
            }
        }
#if RVB_STAMPS
        STAMP(tb)
        st.leaf_steps += 1; st.leaf_cycles += tb - ta;
        st.quad_leaf_steps += ((threadIdx.x & 3u) == 0 && ref != NONE) ? 1 : 0;
#endif
        if (finished) {
            STAMP(ta)
            Hit h;
            h.t = best_t;
            h.tri = best_i;
            job.done(ANY ? found : best_i != NONE, h);
            active = job.next(o, d, tmax);
            if (active) RESET_QUERY_JOBS()
#if RVB_STAMPS
            STAMP(tb)
            st.done_calls += 1; st.done_cycles += tb - ta;
#endif
        }
    }
#if RVB_STAMPS
    if (sc.stamps) {
        STAMP(tb)
        // wave-level values are the maximum over lanes (a lane counts the wave steps it took part in)
        unsigned long long v[9] = {st.node_steps, st.node_cycles, st.leaf_steps, st.leaf_cycles, st.done_calls, st.done_cycles,
                                   tb - st.t0, st.quad_node_steps, st.quad_leaf_steps};
        for (int i = 0; i < 7; ++i) {
            unsigned long long m = v[i];
            for (int off = 32; off > 0; off >>= 1) { unsigned long long o2 = __shfl_xor(m, off); m = o2 > m ? o2 : m; }
            if ((threadIdx.x & 63u) == 0) atomicAdd(sc.stamps + i, m);
        }
        atomicAdd(sc.stamps + 7, v[7]);
        atomicAdd(sc.stamps + 8, v[8]);
        if ((threadIdx.x & 63u) == 0) atomicAdd(sc.stamps + 9, 1ull);
    }
#endif
#undef RESET_QUERY_JOBS
}

// min of two unsigned 64-bit keys.  The compiler's form is v_cmp_lt_u64 -> VCC and two v_cndmask_b32 that read VCC; the SECOND
// select on one VCC value issues far slower than the first (tools/inst_probe.hip "cmpsel2_vcc": 3.0 ns against 0.9 ns for the
// same select on an SGPR-pair mask at 8 waves per SIMD, and 5-10x that at low occupancy).  Here the mask lives in an SGPR pair.
__device__ __forceinline__ unsigned long long min_u64(unsigned long long a, unsigned long long b)
{
    unsigned long long mask;
    uint32_t lo, hi;
    // (s_nop 1: a VALU-written SGPR needs two wait states before a VALU reads it as a mask)
    asm("v_cmp_lt_u64_e64 %0, %3, %4\n\ts_nop 1\n\tv_cndmask_b32_e64 %1, %6, %5, %0\n\tv_cndmask_b32_e64 %2, %8, %7, %0"
        : "=&s"(mask), "=&v"(lo), "=&v"(hi)
        : "v"(a), "v"(b), "v"((uint32_t) a), "v"((uint32_t) b), "v"((uint32_t) (a >> 32)), "v"((uint32_t) (b >> 32)));
    return ((unsigned long long) hi << 32) | lo;
}

// Population count of a wave mask as a 32-bit scalar (the builtin's 64-bit result drags the comparisons that follow
// onto the VALU as 64-bit compares).
__device__ __forceinline__ int scalar_popcount(unsigned long long mask)
{
    int n;
    asm("s_bcnt1_i32_b64 %0, %1" : "=s"(n) : "s"(mask) : "scc");
    return n;
}

// Closest-hit job loop with SCHEDULED step kinds over the wave's 16 quads (path_kernel).
// A quad is in one of four states, all encoded in `ref`: at a node (bit 31 clear), at a leaf (bit 31 set), query
// finished (NONE), out of jobs (IDLE).  The while-while loop above runs node steps until the LAST quad has reached a
// leaf, so on incoherent rays (every bounce after the first) only ~7 of 16 quads do useful work in a node step.  Here
// a step kind is executed for the quads in that state while the others keep theirs.  Rounds 1-3 chose the kind by a
// majority vote per iteration (host replay on workload C2, tools/travsim.cpp: wave-level node steps per bounce 37 -> 28,
// quads active per node step 6.7 -> 8.9, wave instructions per bounce -13 %); round 4 replaced the vote by a fixed
// cycle with thresholds (node step, leaf step if a third of the live lanes wait for one, shading step if a quarter do:
// 27.6 + 4.8 + 2.4 -> 22.0 + 5.7 + 3.8 steps per 16 ray-bounces, tools/travforms.cpp) — see traverse_pairs_cycle,
// "THE SCHEDULE", for the measurements.
template <class Job>
__device__ __forceinline__ void traverse_jobs_cycle(const SceneDev & sc, uint32_t * __restrict__ stack, Job & job)
{
    const uint32_t IDLE = 0xFFFFFFFEu;
    const uint32_t c = threadIdx.x & 3u;
    const uint32_t lane_base4 = (threadIdx.x & 60u) << 2;
    const uint32_t lane_bit = 1u << c, lt_mask = lane_bit - 1u;
    const char * node_base = reinterpret_cast<const char *>(sc.nodes);
    const uint32_t child_off = 16u * c;
    const float neg_cull = -sc.cull_abs, cull_scale = 1.0f + sc.cull_rel;
    v3 o = mk3(0, 0, 0), d = mk3(0, 0, 0);
    float tmax = 0.0f;
    const unsigned long long NO_HIT_KEY = (0x7F800000ull << 32) | NONE;
    const char * tri_base = reinterpret_cast<const char *>(sc.tris);      // wave-uniform base + 32-bit byte offset, like the nodes
    float ix = 0.0f, iy = 0.0f, iz = 0.0f, oix = 0.0f, oiy = 0.0f, oiz = 0.0f;
    unsigned long long best_key = NO_HIT_KEY;                              // (distance bits, triangle index) of the closest hit so far
    uint32_t sp = 0, ref = IDLE;
    uint32_t selx = 0, sely = 0, selz = 0;       // slab_select (near / far plane by the direction's sign) here as well
#define RESET_QUERY_QUADS()                                                              \
    {                                                                                    \
        ix = clamp_inv(d.x); iy = clamp_inv(d.y); iz = clamp_inv(d.z);                   \
        oix = o.x * ix; oiy = o.y * iy; oiz = o.z * iz;                                  \
        selx = slab_selector(ix); sely = slab_selector(iy); selz = slab_selector(iz);    \
        best_key = NO_HIT_KEY; sp = 0; ref = 0;                                          \
    }
    if (job.next(o, d, tmax)) RESET_QUERY_QUADS()
    int n_active = 0;                    // lanes that carry a ray (not IDLE): changes in shading steps only
    auto leaf_step = [&]() {
        if ((int32_t) ref < (int32_t) IDLE) {
            const uint32_t first = ref & 0x0FFFFFFFu;
            const uint32_t count = ((ref >> 28) & 7u) + 1u;
            float dist = 0.0f;
            uint32_t idx = NONE;
            if (c < count) {
                const float4 * tp = reinterpret_cast<const float4 *>(tri_base + tri_byte_offset(first + c));
                float4 ta = tp[0], tb = tp[1], tc = tp[2];
                asm volatile("" : "+v"(ta.x), "+v"(tb.x), "+v"(tc.x));     // all three loads leave before the first use
                dist = mt_intersect(mk3(ta.x, ta.y, ta.z), mk3(ta.w, tb.x, tb.y), mk3(tb.z, tb.w, tc.x), o, d);
                idx = __float_as_uint(tc.y);
            }
            // kernel.cpp:180-188 — smallest distance wins, equal distances go to the lower index.  A candidate
            // distance is > EPSILON > 0, and positive floats order like their bit patterns, so (distance, index)
            // is ONE unsigned 64-bit key: the quad minimum and the comparison with the best so far are three
            // 64-bit compares.  "No hit" is (+inf, NONE), the largest key a lane can hold.
            const bool valid = c < count && dist > RVB_EPSILON;
            unsigned long long key = valid ? (((unsigned long long) __float_as_uint(dist) << 32) | idx) : NO_HIT_KEY;
            key = min_u64(key, dpp_u64<QP_SWAP1>(key));
            key = min_u64(key, dpp_u64<QP_SWAP2>(key));
            best_key = min_u64(best_key, key);
            if (sp > 0) { --sp; ref = stack[sp * QUADS_PER_BLOCK]; } else ref = NONE;
        }
    };
    auto shading_step = [&]() {
        if (ref == NONE) {
            Hit h;
            h.t = __uint_as_float((uint32_t) (best_key >> 32));
            h.tri = (uint32_t) best_key;
            job.done(h.tri != NONE, h);
            ref = IDLE;
            if (job.next(o, d, tmax)) RESET_QUERY_QUADS()
        }
        n_active = scalar_popcount(__builtin_amdgcn_ballot_w64(ref != IDLE));
    };
    auto node_step = [&]() {
        if ((int32_t) ref >= 0) {
            const uint4 n = *reinterpret_cast<const uint4 *>(node_base + (ref | child_off));
            const float limit = fmaf(__uint_as_float((uint32_t) (best_key >> 32)), cull_scale, sc.cull_abs);
            float tn;
            const bool ok = slab_select(n, ix, iy, iz, oix, oiy, oiz, selx, sely, selz, limit, neg_cull, job.skip_ref(), tn);
            const uint32_t cref = n.w;
            const uint32_t key = ok ? ((__float_as_uint(fmaxf(tn, 0.0f)) & ~3u) | c) : NONE;
            uint32_t kmin = min(key, dpp_u<QP_SWAP1>(key));
            kmin = min(kmin, dpp_u<QP_SWAP2>(kmin));
            if (kmin == NONE) {
                if (sp > 0) { --sp; ref = stack[sp * QUADS_PER_BLOCK]; } else ref = NONE;
            } else {
                const uint32_t winner = kmin & 3u;
                uint32_t okmask = ok ? lane_bit : 0u;
                okmask |= dpp_u<QP_SWAP1>(okmask);
                okmask |= dpp_u<QP_SWAP2>(okmask);
                const uint32_t rest = okmask & ~(1u << winner);
                if (ok && c != winner)
                    stack[(sp + __popc(rest & lt_mask)) * QUADS_PER_BLOCK] = cref;
                sp += __popc(rest);
                ref = (uint32_t) __builtin_amdgcn_ds_bpermute((int) (lane_base4 + (winner << 2)), (int) cref);
            }
        }
    };
    n_active = scalar_popcount(__builtin_amdgcn_ballot_w64(ref != IDLE));
    // (the schedule of traverse_pairs_cycle: node step, leaf step if a third of the live lanes wait for one, shading step if a quarter do)
    for (;;) {
        if (n_active == 0)
            break;
        bool ran = __builtin_amdgcn_ballot_w64((int32_t) ref >= 0) != 0ull;
        node_step();
        const int n_leaf = scalar_popcount(__builtin_amdgcn_ballot_w64((int32_t) ref < (int32_t) IDLE));   // signed: leaves are < -2
        if (n_leaf && (RVB_CYCLE_LEAF_NUM * n_leaf >= RVB_CYCLE_LEAF_DEN * n_active || !ran)) {
            leaf_step();
            ran = true;
        }
        const int n_done = scalar_popcount(__builtin_amdgcn_ballot_w64(ref == NONE));
        if (n_done && (RVB_CYCLE_DONE_NUM * n_done >= RVB_CYCLE_DONE_DEN * n_active || !ran))
            shading_step();
    }
#undef RESET_QUERY_QUADS
}

// TWO LANES PER RAY (path_kernel at RVB_PATH_LANES = 2): a lane owns two children of a node and two triangles of a leaf, a wave
// carries 32 rays.  The schedule, the stack handling, the reductions and the loads' addressing are per-RAY work that every lane of
// the ray repeats: with two lanes instead of four a node step costs ~1.45x the instructions for twice the rays.  (One lane per
// ray would be cheaper still per ray, but 100 k rays are then 1.5 waves per SIMD, too few to cover a node fetch.)
// stack: this pair's column of the LDS stack, entries PAIRS_PER_BLOCK words apart.
// The node step of traverse_pairs_cycle is written for ISSUE COST (round 4; measured as the build flag RVB_PAIR_PUSH_COUNTS against the
// hit-mask form it replaced, like the short vote — RVB_PAIR_SHORT_VOTE — and the chained node step — RVB_PAIR_CHAIN — that led to
// THE SCHEDULE further down: the flags exist in the commits of those measurements only).  In the pipeline (traces of the
// next group beside the binning of this one) the SIMDs issue vector instructions three quarters of the time, and the node step is two
// thirds of the path kernel's instructions; tools/inst_probe.hip measures two classes of them on gfx950 — v_fma / v_add / v_mul_f32,
// v_mov, two-operand integer add / and / or / xor / right shift and v_bitop3 issue at the full rate, everything else (comparisons,
// selects, min / max, DPP, v_perm, v_fma_mix, three-operand integer forms) at 0.6 of it (profiles/r04b_inst_probe.log).  The step now:
//   - pushes from COUNTS: a lane keeps the children whose key is not the pair's minimum, the second lane's entries go on top of the
//     first lane's, so one two-bit count crosses the pair (one DPP move) instead of the four-bit hit mask and its population counts;
//   - keys of the UNCLAMPED entry distance, compared as signed integers (no max(t, 0) per child; tools/travforms.cpp replays the same
//     number of node visits), built with one v_bitop3_b32;
//   - the winner's reference as (mine | theirs) with 0 in the lane that does not own it;
//   - the culling distance is state (changes in leaf steps, five times rarer than node steps); the stack pointer is an LDS byte address.
// 75 -> 57 vector instructions, 118 -> 91 issue units per node step (tools/isa_mix.py); same visits, same records, same bytes.
// Measured (profiles/r04_push_counts_n1.txt): pipeline 4.47-4.50 -> 4.37-4.40 ms per impulse response with the kernel capped at 80
// VGPRs (RVB_PAIR_WAVES = 6); uncapped it takes 84, loses a wave per SIMD to the kernels beside it and the pipeline is 8 % SLOWER
// (4.82-4.87 ms) — the register count of the path kernel matters more than its instruction count.  Alone (one trace of 100 k rays,
// bound by the latency of its chains) the kernel takes 3.49 ms either way.
template <class Job>
__device__ __forceinline__ void traverse_pairs_cycle(const SceneDev & sc, uint32_t * __restrict__ stack, Job & job)
{
    const uint32_t IDLE = 0xFFFFFFFEu;
    const uint32_t h = threadIdx.x & 1u;
    uint32_t c0 = 2u * h, c1 = c0 + 1u;                                    // the children this lane owns
    asm volatile("" : "+v"(c0), "+v"(c1));                                 // lane constants that stay in their registers (else recomputed in every node step)
    const char * node_base = reinterpret_cast<const char *>(sc.nodes);
    const char * tri_base = reinterpret_cast<const char *>(sc.tris);
    uint32_t child_off = 32u * h;
    asm volatile("" : "+v"(child_off));
    uint32_t clear2 = ~3u;
    asm volatile("" : "+v"(clear2));
    const float neg_cull = -sc.cull_abs, cull_scale = 1.0f + sc.cull_rel;
    const unsigned long long NO_HIT_KEY = (0x7F800000ull << 32) | NONE;
    v3 o = mk3(0, 0, 0), d = mk3(0, 0, 0);
    float tmax = 0.0f;
    float ix = 0.0f, iy = 0.0f, iz = 0.0f, oix = 0.0f, oiy = 0.0f, oiz = 0.0f;
    unsigned long long best_key = NO_HIT_KEY;
    // the stack pointer is the LDS byte address of the pair's next free row (rows are PAIRS_PER_BLOCK words apart)
    const uint32_t PAIR_ROW = PAIRS_PER_BLOCK * (uint32_t) sizeof(uint32_t);
    const uint32_t bottom = (uint32_t) (uintptr_t) (lds_u32_ptr) stack;
    typedef uint32_t walk_t __attribute__((ext_vector_type(2)));
    walk_t walk = {IDLE, bottom};
#define ref walk.x
#define sp walk.y
#define RVB_PAIR_POP() { if (sp != bottom) { sp -= PAIR_ROW; ref = *(lds_u32_ptr) (uintptr_t) sp; } else ref = NONE; }
#define RVB_PAIR_EMPTY() sp = bottom
    uint32_t selx = 0, sely = 0, selz = 0;
    float limit = 0.0f;                  // culling distance of the best hit so far: changes in leaf steps, is read in node steps
#define RVB_PAIR_LIMIT() limit = fmaf(__uint_as_float((uint32_t) (best_key >> 32)), cull_scale, sc.cull_abs)
#define RESET_QUERY_PAIRS()                                                              \
    {                                                                                    \
        ix = clamp_inv(d.x); iy = clamp_inv(d.y); iz = clamp_inv(d.z);                   \
        oix = o.x * ix; oiy = o.y * iy; oiz = o.z * iz;                                  \
        selx = slab_selector(ix); sely = slab_selector(iy); selz = slab_selector(iz);    \
        best_key = NO_HIT_KEY; RVB_PAIR_EMPTY(); ref = 0; RVB_PAIR_LIMIT();              \
    }
#if RVB_STAMPS
    // diagnostic builds.  -DRVB_STAMPS=1: where a wave's cycles go — [0] the schedule's ballots and branches, [1] node step until its two loads are back, [2] the rest of the
    // node step (incl. the wait for the popped entry), [3] / [4] the same for leaf steps, [5] shading steps; [6..8] step counts.  Any RVB_STAMPS
    // (2 = these alone, the loop runs at its own pace): [9] shader cycles and [11] 100-MHz ticks of the whole loop — their quotient is the
    // clock the chip holds under this load (MI355X_MICROARCH.md "DVFS give-back") —, [10] waves
    unsigned long long sv[6] = {0, 0, 0, 0, 0, 0}, sn[3] = {0, 0, 0}, t_loop, r_loop, t_a = 0, t_b = 0, t_c = 0;
    STAMP(t_loop)
    { __builtin_amdgcn_sched_barrier(0); r_loop = __builtin_amdgcn_s_memrealtime(); __builtin_amdgcn_s_waitcnt(0xC07F); __builtin_amdgcn_sched_barrier(0); }
    t_c = t_loop;
#endif
    if (job.next(o, d, tmax)) RESET_QUERY_PAIRS()
    int n_active = 0;                    // lanes that carry a ray (not IDLE): changes in shading steps only
    // the three step kinds of the loop (inlined where the schedule below calls them)
    auto leaf_step = [&]() {
        RVB_MARK("leaf");
#if RVB_STAMPS == 1
        if ((int32_t) ref < (int32_t) IDLE) {
            const uint32_t first = ref & 0x0FFFFFFFu, count = ((ref >> 28) & 7u) + 1u;
            const float4 * q0 = reinterpret_cast<const float4 *>(tri_base + tri_byte_offset(first + (h < count ? h : 0u)));
            const float4 * q1 = reinterpret_cast<const float4 *>(tri_base + tri_byte_offset(first + (h + 2u < count ? h + 2u : 0u)));
            float4 w0 = q0[0], w1 = q0[2], w2 = q1[0], w3 = q1[2];
            asm volatile("s_waitcnt vmcnt(0)" : "+v"(w0.x), "+v"(w1.x), "+v"(w2.x), "+v"(w3.x) :: "memory");
        }
        STAMP(t_b)
        sv[3] += t_b - t_a; sn[1] += 1;
#endif
        if ((int32_t) ref < (int32_t) IDLE) {
            // triangles h and h + 2 of the leaf (a two-triangle leaf gives each lane one)
            const uint32_t first = ref & 0x0FFFFFFFu;
            const uint32_t count = ((ref >> 28) & 7u) + 1u;
            const uint32_t j0 = h, j1 = h + 2u;
            const float4 * tp0 = reinterpret_cast<const float4 *>(tri_base + tri_byte_offset(first + (j0 < count ? j0 : 0u)));
            const float4 * tp1 = reinterpret_cast<const float4 *>(tri_base + tri_byte_offset(first + (j1 < count ? j1 : 0u)));
            float4 ta = tp0[0], tb = tp0[1], tc = tp0[2], ua = tp1[0], ub = tp1[1], uc = tp1[2];
            asm volatile("" : "+v"(ta.x), "+v"(tb.x), "+v"(tc.x), "+v"(ua.x), "+v"(ub.x), "+v"(uc.x));   // all six loads leave before the first use
            const float dist0 = mt_intersect(mk3(ta.x, ta.y, ta.z), mk3(ta.w, tb.x, tb.y), mk3(tb.z, tb.w, tc.x), o, d);
            const float dist1 = mt_intersect(mk3(ua.x, ua.y, ua.z), mk3(ua.w, ub.x, ub.y), mk3(ub.z, ub.w, uc.x), o, d);
            // kernel.cpp:180-188 — smallest distance wins, equal distances go to the lower index: one unsigned 64-bit key
            const bool valid0 = j0 < count && dist0 > RVB_EPSILON, valid1 = j1 < count && dist1 > RVB_EPSILON;
            const unsigned long long k0 = valid0 ? (((unsigned long long) __float_as_uint(dist0) << 32) | __float_as_uint(tc.y)) : NO_HIT_KEY;
            const unsigned long long k1 = valid1 ? (((unsigned long long) __float_as_uint(dist1) << 32) | __float_as_uint(uc.y)) : NO_HIT_KEY;
            unsigned long long key = min_u64(k0, k1);
            key = min_u64(key, dpp_u64<QP_SWAP1>(key));
            best_key = min_u64(best_key, key);
            RVB_PAIR_LIMIT();
            RVB_PAIR_POP()
        }
#if RVB_STAMPS == 1
        STAMP(t_c)
        sv[4] += t_c - t_b;
#endif
    };
    auto shading_step = [&]() {
        RVB_MARK("done");
        if (ref == NONE) {
            Hit hit;
            hit.t = __uint_as_float((uint32_t) (best_key >> 32));
            hit.tri = (uint32_t) best_key;
            job.done(hit.tri != NONE, hit);
            ref = IDLE;
            if (job.next(o, d, tmax)) RESET_QUERY_PAIRS()
        }
        n_active = scalar_popcount(__builtin_amdgcn_ballot_w64(ref != IDLE));
#if RVB_STAMPS == 1
        STAMP(t_c)
        sv[5] += t_c - t_a; sn[2] += 1;
        t_a = t_c;
#endif
    };
    auto node_step = [&]() {
        RVB_MARK("node");
#if RVB_STAMPS == 1
        if ((int32_t) ref >= 0) {
            const uint4 * pp = reinterpret_cast<const uint4 *>(node_base + (ref | child_off));
            uint4 w0 = pp[0], w1 = pp[1];
            asm volatile("s_waitcnt vmcnt(0)" : "+v"(w0.x), "+v"(w1.x) :: "memory");     // the step's own loads hit the L1 afterwards
        }
        STAMP(t_b)
        sv[1] += t_b - t_a; sn[0] += 1;
#endif
        if ((int32_t) ref >= 0) {
            const uint4 * np = reinterpret_cast<const uint4 *>(node_base + (ref | child_off));
            const uint4 n0 = np[0], n1 = np[1];
            float tn0, tn1;
            const bool ok0 = slab_select(n0, ix, iy, iz, oix, oiy, oiz, selx, sely, selz, limit, neg_cull, job.skip_ref(), tn0);
            const bool ok1 = slab_select(n1, ix, iy, iz, oix, oiy, oiz, selx, sely, selz, limit, neg_cull, job.skip_ref(), tn1);
            // the hit children's keys: entry distance (its two low bits give way to the child number), compared as SIGNED integers —
            // negative distances (the origin is inside the box, or the box a rounding behind it) come before all others, in any
            // order; tools/travforms.cpp replays the same number of node visits as with keys of max(distance, 0)
            const uint32_t NO_CHILD = 0x7FFFFFFFu;
            // ((distance & ~3) | child) as one v_bitop3_b32 with register operands: issues at the rate of v_fma_f32, the and_or
            // form at 0.6 of it (profiles/r04b_inst_probe.log)
            const uint32_t key0 = ok0 ? __builtin_amdgcn_bitop3_b32(__float_as_uint(tn0), clear2, c0, 0xEA) : NO_CHILD;
            const uint32_t key1 = ok1 ? __builtin_amdgcn_bitop3_b32(__float_as_uint(tn1), clear2, c1, 0xEA) : NO_CHILD;
            uint32_t kmin = (uint32_t) min((int32_t) key0, (int32_t) key1);
            kmin = (uint32_t) min((int32_t) kmin, (int32_t) dpp_u<QP_SWAP1>(kmin));
            if (kmin == NO_CHILD) {
                RVB_PAIR_POP()
            } else {
                // the pair's pushes in child order (as below) from the lanes' COUNTS: a lane's kept children go on top of the other
                // lane's if it is the pair's second lane, so one 2-bit count crosses the pair instead of the hit mask, and a lane's
                // rows follow from its own two flags (the keys name the child: key == kmin is the winner)
                const bool other0 = key0 != kmin, other1 = key1 != kmin;
                const bool keep0 = ok0 && other0, keep1 = ok1 && other1;
                const uint32_t first = keep0 ? PAIR_ROW : 0u;                          // counts in bytes of stack rows
                const uint32_t n_mine = first + (keep1 ? PAIR_ROW : 0u);
                const uint32_t n_theirs = dpp_u<QP_SWAP1>(n_mine);
                const uint32_t row = __umul24(n_theirs, h) + sp;                       // sp + (h ? n_theirs : 0) as one v_mad_u32_u24
                if (keep0)
                    *(lds_u32_ptr) (uintptr_t) row = n0.w;
                if (keep1)
                    *(lds_u32_ptr) (uintptr_t) (row + first) = n1.w;
                // the winner is the child whose key IS kmin (keys carry the child number)
                const uint32_t mine = other1 ? (other0 ? 0u : n0.w) : n1.w;            // 0 in the lane that does not own it
                sp += n_mine + n_theirs;
                ref = mine | dpp_u<QP_SWAP1>(mine);
            }
        }
#if RVB_STAMPS == 1
        STAMP(t_c)
        sv[2] += t_c - t_b;
#endif
    };
    // THE SCHEDULE (round 4).  Rounds 1-3 voted: every iteration three ballots, and the step kind most lanes waited for was executed.  A wave's time,
    // though, goes into the LATENCY of its own instruction stream (tools/pair_stamps.py: 300 of an iteration's 1 900 cycles were the vote's dependent
    // scalar chain), so the vote was first shortened (one ballot while the lanes at a node are a majority: two-lane kernel alone 3.54 -> 3.46 ms,
    // four-lane kernel 3.54 -> 3.31), then a node step was chained behind every leaf and shading step (same steps, 28.7 votes instead of 36.2 per
    // 32 ray-bounces: 3.43 -> 3.27 / 3.32 -> 3.22 ms) — and then dropped: every iteration is a node step for the lanes at a node, then a leaf step if a
    // third of the live lanes wait for one, then a shading step if a quarter of them do (or if nothing else could run).  tools/travforms.cpp
    // (TRAVFORMS_CYCLE) replays 23.7 node + 6.3 leaf + 3.2 shading steps per 32 ray-bounces at C2 where the majority vote takes 28.6 + 5.2 + 2.6 (C4:
    // 26.5 + 5.9 + 3.3 against 32.0 + 4.9 + 2.6): lanes waiting at a leaf need not become the largest group before they are served, and the node steps
    // run fuller (0.61 of the lanes instead of 0.52).  Two-lane kernel alone 3.27 -> 3.16 ms (100 k rays), 1.86 -> 1.80 ms per 100 k rays at 800 k;
    // four-lane kernel 3.27 -> 3.13 ms; pipeline 4.22 -> 4.12 ms per IR (profiles/r04d_cycle*_n1.txt; thresholds of 25-40 % all within 1 %).
    // Same queries, same results: the schedule only decides WHEN a lane's next step runs.  What did not help a wave's latency: one dword of the next
    // node requested a step ahead (a third L1 access per step costs more than its head start: 3.40 -> 3.81 ms), two node steps per iteration.
    n_active = scalar_popcount(__builtin_amdgcn_ballot_w64(ref != IDLE));
    for (;;) {
        RVB_MARK("vote");               // (the schedule's block; tools/isa_mix.py knows it by this name)
        if (n_active == 0)
            break;
        bool ran = __builtin_amdgcn_ballot_w64((int32_t) ref >= 0) != 0ull;
#if RVB_STAMPS == 1
        STAMP(t_a)
        sv[0] += t_a - t_c;
#endif
        node_step();
#if RVB_STAMPS == 1
        t_a = t_c;
#endif
        const int n_leaf = scalar_popcount(__builtin_amdgcn_ballot_w64((int32_t) ref < (int32_t) IDLE));
        if (n_leaf && (RVB_CYCLE_LEAF_NUM * n_leaf >= RVB_CYCLE_LEAF_DEN * n_active || !ran)) {
            leaf_step();
            ran = true;
#if RVB_STAMPS == 1
            t_a = t_c;
#endif
        }
        const int n_done = scalar_popcount(__builtin_amdgcn_ballot_w64(ref == NONE));
        if (n_done && (RVB_CYCLE_DONE_NUM * n_done >= RVB_CYCLE_DONE_DEN * n_active || !ran))
            shading_step();
        RVB_MARK("loop_end");
    }
#if RVB_STAMPS
    if (sc.stamps) {
        STAMP(t_b)
        unsigned long long r_end;
        { __builtin_amdgcn_sched_barrier(0); r_end = __builtin_amdgcn_s_memrealtime(); __builtin_amdgcn_s_waitcnt(0xC07F); __builtin_amdgcn_sched_barrier(0); }
        if ((threadIdx.x & 63u) == 0) {
            for (int i = 0; i < 6; ++i) atomicAdd(sc.stamps + i, sv[i]);
            for (int i = 0; i < 3; ++i) atomicAdd(sc.stamps + 6 + i, sn[i]);
            atomicAdd(sc.stamps + 9, t_b - t_loop);
            atomicAdd(sc.stamps + 10, 1ull);
            atomicAdd(sc.stamps + 11, r_end - r_loop);
        }
    }
#endif
#undef RESET_QUERY_PAIRS
#undef RVB_PAIR_POP
#undef RVB_PAIR_EMPTY
#undef ref
#undef sp
#undef RVB_PAIR_LIMIT
}

// Any-hit query with two lanes per ray (shadow_pair_kernel): is there a triangle with EPSILON < distance <= tmax (the negation of
// reference kernel.cpp:295).  Lockstep like traverse_quad<true>: the 32 pairs of the wave start a query together and leave the
// loops as they finish; no visiting order (the lowest hit child is entered, the others pushed).
__device__ __forceinline__ bool traverse_pair_any(const SceneDev & sc, const v3 o, const v3 d, const float tmax,
                                                  uint32_t * __restrict__ stack, const uint32_t skip)
{
    const uint32_t h = threadIdx.x & 1u;
    const uint32_t c0 = 2u * h;
    const uint32_t bit0 = 1u << c0, bit1 = 2u << c0, lt0 = bit0 - 1u, lt1 = bit1 - 1u;
    const char * node_base = reinterpret_cast<const char *>(sc.nodes);
    const char * tri_base = reinterpret_cast<const char *>(sc.tris);
    const uint32_t child_off = 32u * h;                                    // (pinned in a register it would be the 81st: a wave per SIMD less)
    const float neg_cull = -sc.cull_abs;
    const float limit = fmaf(tmax, 1.0f + sc.cull_rel, sc.cull_abs);
    const float ix = clamp_inv(d.x), iy = clamp_inv(d.y), iz = clamp_inv(d.z);
    const float oix = o.x * ix, oiy = o.y * iy, oiz = o.z * iz;
    uint32_t sp = 0, ref = 0;
    for (;;) {
        while (!(ref & RVB_BVH_LEAF)) {
            const uint4 * np = reinterpret_cast<const uint4 *>(node_base + (ref | child_off));
            const uint4 n0 = np[0], n1 = np[1];
            float tn0, tn1;
            const bool ok0 = slab(n0, ix, iy, iz, oix, oiy, oiz, limit, neg_cull, skip, tn0);      // (slab_select: shadow pairs 1.28 -> 1.34 ms)
            const bool ok1 = slab(n1, ix, iy, iz, oix, oiy, oiz, limit, neg_cull, skip, tn1);
            uint32_t okmask = (ok0 ? bit0 : 0u) | (ok1 ? bit1 : 0u);
            okmask |= dpp_u<QP_SWAP1>(okmask);
            if (okmask == 0u) {
                if (sp > 0) { --sp; ref = stack[sp * PAIRS_PER_BLOCK]; } else ref = NONE;
                continue;
            }
            const uint32_t rest = okmask & (okmask - 1u);             // all hit children but the lowest
            const uint32_t winner_bit = okmask ^ rest;
            if (ok0 && bit0 != winner_bit)
                stack[(sp + __popc(rest & lt0)) * PAIRS_PER_BLOCK] = n0.w;
            if (ok1 && bit1 != winner_bit)
                stack[(sp + __popc(rest & lt1)) * PAIRS_PER_BLOCK] = n1.w;
            sp += __popc(rest);
            const uint32_t mine = (winner_bit & 0xAu) ? n1.w : n0.w;  // children 1, 3 are the lanes' second child
            const uint32_t theirs = dpp_u<QP_SWAP1>(mine);
            ref = (winner_bit & (bit0 | bit1)) ? mine : theirs;
        }
        if (ref == NONE)
            return false;
        // triangles h and h + 2 of the leaf
        const uint32_t first = ref & 0x0FFFFFFFu;
        const uint32_t count = ((ref >> 28) & 7u) + 1u;
        const uint32_t j0 = h, j1 = h + 2u;
        const float4 * tp0 = reinterpret_cast<const float4 *>(tri_base + tri_byte_offset(first + (j0 < count ? j0 : 0u)));
        const float4 * tp1 = reinterpret_cast<const float4 *>(tri_base + tri_byte_offset(first + (j1 < count ? j1 : 0u)));
        float4 ta = tp0[0], tb = tp0[1], tc = tp0[2], ua = tp1[0], ub = tp1[1], uc = tp1[2];
        asm volatile("" : "+v"(ta.x), "+v"(tb.x), "+v"(tc.x), "+v"(ua.x), "+v"(ub.x), "+v"(uc.x));
        const float dist0 = mt_intersect(mk3(ta.x, ta.y, ta.z), mk3(ta.w, tb.x, tb.y), mk3(tb.z, tb.w, tc.x), o, d);
        const float dist1 = mt_intersect(mk3(ua.x, ua.y, ua.z), mk3(ua.w, ub.x, ub.y), mk3(ub.z, ub.w, uc.x), o, d);
        uint32_t hit = ((j0 < count && dist0 > RVB_EPSILON && dist0 <= tmax) || (j1 < count && dist1 > RVB_EPSILON && dist1 <= tmax)) ? 1u : 0u;
        hit |= dpp_u<QP_SWAP1>(hit);
        if (hit)
            return true;
        if (sp > 0) { --sp; ref = stack[sp * PAIRS_PER_BLOCK]; } else return false;
    }
}

// A single query through the same loop (the quad's lanes return together).
struct OneShotJob {
    v3 o, d;
    float tmax;
    bool pending, hit;
    Hit result;
    uint32_t skip;
    __device__ __forceinline__ uint32_t skip_ref() const { return skip; }
    __device__ __forceinline__ bool next(v3 & o_, v3 & d_, float & tmax_)
    {
        if (!pending) return false;
        pending = false;
        o_ = o; d_ = d; tmax_ = tmax;
        return true;
    }
    __device__ __forceinline__ void done(bool h, const Hit & r) { hit = h; result = r; }
};

template <bool ANY>
__device__ __forceinline__ bool traverse_quad(const SceneDev & sc, const v3 o, const v3 d, const float tmax,
                                              uint32_t * __restrict__ stack, Hit & hit, const uint32_t skip = RVB_BVH_EMPTY)
{
    OneShotJob job = {o, d, tmax, true, false, {0.0f, NONE}, skip};
    traverse_jobs<ANY>(sc, stack, job);
    hit = job.result;
    return job.hit;
}

__device__ __forceinline__ v3 ld3(const float * p) { return mk3(p[0], p[1], p[2]); }

// Copies the scene's surface table (64 B per surface) behind the traversal stack in LDS when the launch reserved
// room for it (TraceArgs::lds_surfaces = number of surfaces staged, 0 = none).  Single-wave workgroups: the
// barrier is only the wait for the wave's own LDS writes.
__device__ __forceinline__ float4 lds_load4(lds_float4_ptr p, uint32_t i)
{
    const nt_float4 t = p[i];
    return make_float4(t.x, t.y, t.z, t.w);
}
__device__ __forceinline__ lds_float4_ptr stage_surfaces(const TraceArgs & a, uint32_t * lds_after_stack)
{
    if (!a.lds_surfaces)
        return nullptr;
    float4 * dst = reinterpret_cast<float4 *>(lds_after_stack);
    const float4 * src = reinterpret_cast<const float4 *>(a.scene.surfaces);
    for (uint32_t i = threadIdx.x; i < 4u * a.lds_surfaces; i += WAVE)
        dst[i] = src[i];
    __syncthreads();
    return (lds_float4_ptr) dst;
}

// 16-byte piece `chunk` of a surface's 64-byte row (0, 1: specular bands 0-3, 4-7; 2, 3: diffuse), from the staged table or from memory
template <bool SURF_LDS>
__device__ __forceinline__ float4 surface_row(const TraceArgs & a, const lds_float4_ptr surf_lds, const uint32_t surface, const uint32_t chunk)
{
    if (SURF_LDS) return lds_load4(surf_lds, 4 * surface + chunk);
    return reinterpret_cast<const float4 *>(a.scene.surfaces + surface)[chunk];
}

// ---- the final product of a record and the time range of a launch: shared by the shadow stage (shadow_kernels.hip) and the re-shade
// pass (reshade_kernels.hip), which repeats that stage's arithmetic without its traversal ----
// Arrival-time range of the non-zero diffuse impulses, the inputs of findPredelay / MAX_SAMPLE (rayverb.h:49-74, rayverb.cpp:54-57), in
// a.time_range as float bits (non-negative floats order like their bit patterns).  An atomic is skipped when a plain read says it cannot
// move the result (stale reads are harmless).
// Several pairs per launch: one range per pair, updated record by record.
__device__ __forceinline__ void time_range_of_pair(const TraceArgs & a, const uint32_t pair, const float t)
{
    const volatile uint32_t * seen = a.time_range + 2u * pair;
    if (t != 0.0f && __float_as_uint(t) < seen[0]) atomicMin(a.time_range + 2u * pair, __float_as_uint(t));
    if (__float_as_uint(t) > seen[1]) atomicMax(a.time_range + 2u * pair + 1u, __float_as_uint(t));
}
// One pair: every lane keeps its own range, the wave folds them at the kernel's end.
__device__ __forceinline__ void time_range_of_wave(const TraceArgs & a, float tmin, float tmax_seen)
{
    for (int off = 32; off > 0; off >>= 1) {
        tmin = fminf(tmin, __shfl_xor(tmin, off));
        tmax_seen = fmaxf(tmax_seen, __shfl_xor(tmax_seen, off));
    }
    if (threadIdx.x == 0 && a.npairs <= 1) {
        const volatile uint32_t * seen = a.time_range;
        if (tmin != __builtin_inff() && __float_as_uint(tmin) < seen[0]) atomicMin(a.time_range + 0, __float_as_uint(tmin));
        if (__float_as_uint(tmax_seen) > seen[1]) atomicMax(a.time_range + 1, __float_as_uint(tmax_seen));
    }
}

// How many diffuse impulses of a pair carry volume (the shadow stage only): the exact mode lists no more than these (SmallBlock::live_count,
// PairLaunch).  The waves add to a.live_stripes, the stripe of their workgroup; live_sum_kernel (shadow_kernels.hip) makes the counts.
__device__ __forceinline__ uint32_t * live_count_of(const TraceArgs & a, const uint32_t pair)
{
    const uint32_t stripe = blockIdx.x & (RVB_LIVE_STRIPES - 1u);
    return a.live_stripes + (a.npairs > 1 ? stripe * a.npairs + pair : stripe);
}
// One pair: the wave counts in the step of its record loop, where the lanes that skipped a record are back — `nz_writer` is set in one
// lane per live record, so the count is a population count of a ballot and needs no vector register inside the loop —, and adds once
// at the kernel's end.  The lanes still in the loop take a step together, so the lane that leaves last has taken every step and holds
// the wave's count: the largest of the lanes' values.
__device__ __forceinline__ void live_count_step(const TraceArgs & a, const bool nz_writer, uint32_t & live)
{
    if (a.npairs <= 1) live += (uint32_t) __popcll(__ballot(nz_writer));
}
__device__ __forceinline__ void live_count_of_wave(const TraceArgs & a, uint32_t live)
{
    for (int off = 32; off > 0; off >>= 1)
        live = max(live, (uint32_t) __shfl_xor((int) live, off));
    if (threadIdx.x == 0 && a.npairs <= 1 && live) atomicAdd(live_count_of(a, 0), live);
}
// Several pairs per launch: called by the writer lane of a live record; one add per pair among them (a wave's records are neighbours in
// grouped order: nearly always one pair).
__device__ __forceinline__ void live_count_of_pair(const TraceArgs & a, const uint32_t pair)
{
    for (;;) {
        const uint32_t p = (uint32_t) __builtin_amdgcn_readfirstlane((int) pair);
        const unsigned long long same = __ballot(pair == p);
        if (pair == p) {
            if ((uint32_t) __builtin_amdgcn_mbcnt_hi((uint32_t) (same >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t) same, 0u)) == 0u)
                atomicAdd(live_count_of(a, p), (uint32_t) __popcll(same));
            break;
        }
    }
}

// kernel.cpp:480-485 for one band: newVol * attenuation * diffuse * DIFF, left to right.  (One band at a time: a float4 form changes all three kernels.)
__device__ __forceinline__ float band_product(const float vol, const float att, const float dc, const float diff) { return ((vol * att) * dc) * diff; }

// inputs of findPredelay / MAX_SAMPLE (rayverb.h:49-74, rayverb.cpp:54-57): an impulse takes part iff any band is non-zero
// (kernel.cpp:524).  Several pairs: the record's `writer` lane updates its pair's range; one pair: the lane's running range.
__device__ __forceinline__ void note_time(const TraceArgs & a, const bool nonzero, const bool writer, const uint32_t pair, const float t,
                                          float & tmin, float & tmax_seen)
{
    if (!nonzero)
        return;
    if (a.npairs > 1) {
        if (writer) time_range_of_pair(a, pair, t);
    } else {
        if (t != 0.0f) tmin = fminf(tmin, t);
        tmax_seen = fmaxf(tmax_seen, t);
    }
}

// The LDS of a trace workgroup (one wave): [stack_rows][rays] stack words — a ray's (or record's) column, entries `rays` words apart —,
// then the surface table (64 bytes per staged surface, stage_surfaces), then — path kernels with 16-bit keys only — [rays][RVB_KEY_RUN]
// grouping keys.  The kernels take their pointers from it and the launchers their byte counts, so the two cannot drift apart.
struct TraceLds {
    uint32_t rays;               // rays (records) per workgroup: WAVE / lanes per ray
    uint32_t stack_rows;         // stack entries per column; the one-lane kernels add a slack row (their pushes store first and advance if kept)
    uint32_t surfaces_at;        // word offset of the surface table
    uint32_t lds_surfaces;       // surfaces staged (16 words each)
    size_t bytes;                // of the whole workgroup
    static __host__ __device__ __forceinline__ TraceLds make(uint32_t stack_entries, uint32_t lds_surfaces, uint32_t lanes_per_ray, bool key_runs)
    {
        TraceLds l;
        l.rays = WAVE / lanes_per_ray;
        l.stack_rows = stack_entries + (lanes_per_ray == 1 ? 1u : 0u);
        l.surfaces_at = l.stack_rows * l.rays;
        l.lds_surfaces = lds_surfaces;
        l.bytes = ((size_t) l.surfaces_at + 16u * lds_surfaces) * sizeof(uint32_t) + (key_runs ? l.rays * RVB_KEY_RUN * sizeof(uint16_t) : 0u);
        return l;
    }
    // the two tables behind the stack, for a kernel whose dynamic LDS starts at `lds`
    __device__ __forceinline__ uint32_t * surfaces(uint32_t * lds) const { return lds + surfaces_at; }
    __device__ __forceinline__ uint16_t * key_runs(uint32_t * lds) const { return reinterpret_cast<uint16_t *>(lds + surfaces_at + 16u * lds_surfaces); }
};

// KERNEL<true> when the launch stages the surface table in LDS, KERNEL<false> otherwise: single-wave workgroups
template <class Args>
static void launch_by_surfaces(void (*staged)(Args), void (*plain)(Args), uint32_t lds_surfaces, uint64_t blocks, size_t lds, hipStream_t s,
                               const Args & args)
{
    hipLaunchKernelGGL(lds_surfaces ? staged : plain, dim3((unsigned) blocks), dim3(WAVE), lds, s, args);
}

}  // namespace
