// source_kernels.hip — directional sources: the per-band polar pattern of include/rvb_capi.h (rvb_source_pattern) applied to the final
// records of a trace.  No reference counterpart for the stage; the gain is the expression of the reference's kernel `attenuate`
// (rayverb/kernel.cpp:505-513) fed with a departure vector instead of an arrival vector.
//
//   source_pattern_kernel          the [pair][ray][bounce] diffuse records behind the shadow stage: volume_b *= g_b, v = the ray's own
//                                  direction; and the time range of the records that are still live afterwards (the inputs of
//                                  findPredelay / MAX_SAMPLE, rayverb.h:49-74, rayverb.cpp:54-57).  HBM-bound like attenuate_kernel, and
//                                  shaped like it: one workgroup per 4 KiB, 16 bytes per lane, four lanes per record (quad_record).
//   source_pattern_images_kernel   the image-source candidates and the direct slot of every pair: v = mic - position.  A few thousand
//                                  records at most, one lane each.
#include "attenuation.h"

#include <cmath>
#include <cstring>

namespace {

// (g_b of the contract: band_gain of attenuation.h)

// kernel.cpp:511 / :528 on the departure vector `v`: normalize3(normalize3(v)) with lane k of the quad dividing component k, as
// attenuate_chunk_speaker does (one correctly rounded division per normalisation and wave instead of three; same operations on the
// same operands as normalize3).
__device__ __forceinline__ v3 quad_normalize_twice(const uint32_t q, const v3 v)
{
    const float len = length3(v);
    const float own = q == 0 ? v.x : (q == 1 ? v.y : v.z);
    const float n_own = len == 0.0f ? own : own / len;             // normalize3: a zero vector stays zero
    const v3 n = mk3(dpp_f<QP_BCAST(0)>(n_own), dpp_f<QP_BCAST(1)>(n_own), dpp_f<QP_BCAST(2)>(n_own));
    const float len2 = length3(n);
    const float u_own = len2 == 0.0f ? n_own : n_own / len2;
    return mk3(dpp_f<QP_BCAST(0)>(u_own), dpp_f<QP_BCAST(1)>(u_own), dpp_f<QP_BCAST(2)>(u_own));
}

// Every wave walks whole 1 KiB runs of 16 records (uniform trip count: the DPP moves and the wave reduction below see all 64 lanes;
// lanes past the end hold a zero record and store nothing).  FULL: all four chunks of the record are stored back, so that whole
// 64-byte records leave the wave; otherwise only the two volume chunks.  NT: non-temporal stores.
// WIDE: more than 2^32 - 1 records (the ray number then needs a 64-bit division).
template <bool FULL, bool NT, bool WIDE>
__global__ __launch_bounds__(256) void source_pattern_kernel(float4 * __restrict__ records, const uint64_t nrecords, const float4 * __restrict__ directions,
                                                             const SourcePatternDev * __restrict__ patterns, const uint32_t pattern_stride,
                                                             const uint32_t nreflections, const uint32_t rays_per_pair, const uint32_t npairs,
                                                             uint32_t * range)
{
    const uint32_t q = threadIdx.x & 3u, lane = threadIdx.x & 63u;
    const uint64_t nchunks = nrecords * 4;
    const uint64_t stride = (uint64_t) gridDim.x * blockDim.x;
    for (uint64_t w0 = (uint64_t) blockIdx.x * blockDim.x + (threadIdx.x & ~63u); w0 < nchunks; w0 += stride) {
        const uint64_t c = w0 + lane;
        const bool inside = c < nchunks;
        const uint64_t rec = (inside ? c : nchunks - 1) >> 2;      // (lanes past the end: the last record's ray, a valid address)
        const uint32_t ray = WIDE ? (uint32_t) (rec / nreflections) : (uint32_t) rec / nreflections;
        const uint32_t pair = npairs > 1 ? ray / rays_per_pair : 0u;
        const uint32_t dir = npairs > 1 ? ray - pair * rays_per_pair : ray;
        float4 v = make_float4(0, 0, 0, 0);
        if (inside) v = records[c];
        const float4 dv = directions[dir];
        const SourcePatternDev * pat = patterns + (size_t) pair * pattern_stride;
        const v3 u = quad_normalize_twice(q, mk3(dv.x, dv.y, dv.z));
        const float d = dot3(u, mk3(pat->direction[0], pat->direction[1], pat->direction[2]));
        float4 o = v;
        if (q < 2) {
            const float4 s = reinterpret_cast<const float4 *>(pat->shape)[q];
            o = make_float4(v.x * band_gain(s.x, d), v.y * band_gain(s.y, d), v.z * band_gain(s.z, d), v.w * band_gain(s.w, d));
        }
        if (inside && (FULL || q < 2)) {
            if (NT) {
                const nt_float4_t t = {o.x, o.y, o.z, o.w};
                __builtin_nontemporal_store(t, reinterpret_cast<nt_float4_t *>(records + c));
            } else {
                records[c] = o;
            }
        }
        // the time range of the records that still carry volume (kernel.cpp:524 any(volume != 0) on the scaled record)
        const QuadRecord r = quad_record(q, o);
        const bool live = inside && r.nonzero;
        float tmin = live && r.time != 0.0f ? r.time : __builtin_inff();
        float tmax = live ? r.time : 0.0f;
        // one pair per wave run (always, for a single pair): one wave reduction, then one atomic per bound that can still move — with one
        // workgroup per 4 KiB there are millions of waves (time_range_kernel, flat_keys_kernel); a stale read only costs a redundant atomic
        const uint64_t rec_first = w0 >> 2, rec_last = (w0 + 63 < nchunks ? w0 + 63 : nchunks - 1) >> 2;
        const uint64_t per_pair = (uint64_t) rays_per_pair * nreflections;
        const bool one_pair = npairs <= 1 || rec_first / per_pair == rec_last / per_pair;         // (wave-uniform)
        if (one_pair) {
            for (int off = 32; off > 0; off >>= 1) {
                tmin = fminf(tmin, __shfl_xor(tmin, off));
                tmax = fmaxf(tmax, __shfl_xor(tmax, off));
            }
            if (lane == 0) {
                uint32_t * mine = range + 2u * pair;
                const volatile uint32_t * seen = mine;
                if (tmin != __builtin_inff() && __float_as_uint(tmin) < seen[0]) atomicMin(mine + 0, __float_as_uint(tmin));
                if (__float_as_uint(tmax) > seen[1]) atomicMax(mine + 1, __float_as_uint(tmax));
            }
        } else if (live && q == 0) {
            // the run straddles two pairs (once per pair boundary): record by record, each into its own pair's range
            uint32_t * mine = range + 2u * pair;
            if (tmin != __builtin_inff()) atomicMin(mine + 0, __float_as_uint(tmin));
            atomicMax(mine + 1, __float_as_uint(tmax));
        }
    }
}

// The image-source candidates [0, *count) and the direct slot of every pair: v = mic - position, component by component.
__global__ __launch_bounds__(256) void source_pattern_images_kernel(rvb_image_candidate * __restrict__ candidates, const uint32_t * __restrict__ count,
                                                                    rvb_impulse * __restrict__ direct, const uint32_t npairs, const uint32_t rays_per_pair,
                                                                    const uint64_t ray_offset, const float4 * __restrict__ pair_mics, const v3 mic,
                                                                    const SourcePatternDev * __restrict__ patterns, const uint32_t pattern_stride)
{
    const uint32_t ncand = *count, ndirect = npairs > 1 ? npairs : 1u;
    const uint64_t total = (uint64_t) ncand + ndirect;
    for (uint64_t i = (uint64_t) blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (uint64_t) gridDim.x * blockDim.x) {
        rvb_impulse * imp;
        uint32_t pair = 0;
        if (i < ncand) {
            imp = &candidates[i].impulse;
            if (npairs > 1) pair = (uint32_t) ((candidates[i].ray - ray_offset) / rays_per_pair);
        } else {
            pair = (uint32_t) (i - ncand);
            imp = direct + pair;
        }
        v3 m = mic;
        if (npairs > 1) { const float4 pm = pair_mics[pair]; m = mk3(pm.x, pm.y, pm.z); }
        const SourcePatternDev * pat = patterns + (size_t) pair * pattern_stride;
        const v3 v = m - mk3(imp->position[0], imp->position[1], imp->position[2]);
        const float d = dot3(normalize3(normalize3(v)), mk3(pat->direction[0], pat->direction[1], pat->direction[2]));
#pragma unroll
        for (int b = 0; b < 8; ++b) imp->volume[b] = imp->volume[b] * band_gain(pat->shape[b], d);
    }
}

// ---- the tabulated directivity of include/rvb_capi.h (rvb_set_source_table): a gain row per departure direction -------------------
//   source_table_rays_kernel       one row selection per (pair, ray), v = the ray's own direction: the diffuse gain never depends on
//                                  the bounce, so the row's 32 bytes go to ray_gains[pair][ray][8] once and the streaming pass reads them
//   source_table_kernel            source_pattern_kernel's sibling: volume_b *= ray_gains[pair][ray][b], the time range of the scaled records
//   source_table_images_kernel     candidates and direct slot(s): v = mic - position, the row per record, gathered from the table

// (the table row for a departure vector: departure_row of attenuation.h)

// One lane per (pair, ray).
__global__ __launch_bounds__(256) void source_table_rays_kernel(const float4 * __restrict__ directions, const float4 * __restrict__ table,
                                                                const float4 * __restrict__ bases, const uint32_t basis_stride,
                                                                const uint32_t rays_per_pair, const uint64_t nrays, float4 * __restrict__ ray_gains)
{
    for (uint64_t i = (uint64_t) blockIdx.x * blockDim.x + threadIdx.x; i < nrays; i += (uint64_t) gridDim.x * blockDim.x) {
        const uint64_t pair = i / rays_per_pair;
        const float4 dv = directions[i - pair * rays_per_pair];
        const float4 * basis = bases + pair * basis_stride;
        const uint32_t row = departure_row(basis[0], basis[1], basis[2], mk3(dv.x, dv.y, dv.z));
        ray_gains[2 * i + 0] = table[2 * (size_t) row + 0];
        ray_gains[2 * i + 1] = table[2 * (size_t) row + 1];
    }
}

// source_pattern_kernel with the gain read instead of computed: the same walk (whole 1 KiB runs of 16 records per wave, uniform trip
// count), the same stores (whole 64-byte records leave the wave; lanes past the end store nothing), the same reduction of the time range.
// A ray's gain row is read by its nreflections consecutive records: once from HBM, then from the caches.
template <bool WIDE>
__global__ __launch_bounds__(256) void source_table_kernel(float4 * __restrict__ records, const uint64_t nrecords, const float4 * __restrict__ ray_gains,
                                                           const uint32_t nreflections, const uint32_t rays_per_pair, const uint32_t npairs,
                                                           uint32_t * range)
{
    const uint32_t q = threadIdx.x & 3u, lane = threadIdx.x & 63u;
    const uint64_t nchunks = nrecords * 4;
    const uint64_t stride = (uint64_t) gridDim.x * blockDim.x;
    for (uint64_t w0 = (uint64_t) blockIdx.x * blockDim.x + (threadIdx.x & ~63u); w0 < nchunks; w0 += stride) {
        const uint64_t c = w0 + lane;
        const bool inside = c < nchunks;
        const uint64_t rec = (inside ? c : nchunks - 1) >> 2;      // (lanes past the end: the last record's ray, a valid address)
        const uint32_t ray = WIDE ? (uint32_t) (rec / nreflections) : (uint32_t) rec / nreflections;       // within the launch: [pair][ray]
        const uint32_t pair = npairs > 1 ? ray / rays_per_pair : 0u;
        float4 v = make_float4(0, 0, 0, 0);
        if (inside) v = records[c];
        float4 o = v;
        if (q < 2) {
            const float4 g = ray_gains[2 * (size_t) ray + q];
            o = make_float4(v.x * g.x, v.y * g.y, v.z * g.z, v.w * g.w);
        }
        if (inside) records[c] = o;
        // the time range of the records that still carry volume (kernel.cpp:524 any(volume != 0) on the scaled record)
        const QuadRecord r = quad_record(q, o);
        const bool live = inside && r.nonzero;
        float tmin = live && r.time != 0.0f ? r.time : __builtin_inff();
        float tmax = live ? r.time : 0.0f;
        // one pair per wave run, or record by record where the run straddles two pairs: as in source_pattern_kernel
        const uint64_t rec_first = w0 >> 2, rec_last = (w0 + 63 < nchunks ? w0 + 63 : nchunks - 1) >> 2;
        const uint64_t per_pair = (uint64_t) rays_per_pair * nreflections;
        const bool one_pair = npairs <= 1 || rec_first / per_pair == rec_last / per_pair;         // (wave-uniform)
        if (one_pair) {
            for (int off = 32; off > 0; off >>= 1) {
                tmin = fminf(tmin, __shfl_xor(tmin, off));
                tmax = fmaxf(tmax, __shfl_xor(tmax, off));
            }
            if (lane == 0) {
                uint32_t * mine = range + 2u * pair;
                const volatile uint32_t * seen = mine;
                if (tmin != __builtin_inff() && __float_as_uint(tmin) < seen[0]) atomicMin(mine + 0, __float_as_uint(tmin));
                if (__float_as_uint(tmax) > seen[1]) atomicMax(mine + 1, __float_as_uint(tmax));
            }
        } else if (live && q == 0) {
            uint32_t * mine = range + 2u * pair;
            if (tmin != __builtin_inff()) atomicMin(mine + 0, __float_as_uint(tmin));
            atomicMax(mine + 1, __float_as_uint(tmax));
        }
    }
}

// The image-source candidates [0, *count) and the direct slot of every pair, one lane each: v = mic - position, component by component.
__global__ __launch_bounds__(256) void source_table_images_kernel(rvb_image_candidate * __restrict__ candidates, const uint32_t * __restrict__ count,
                                                                  rvb_impulse * __restrict__ direct, const uint32_t npairs, const uint32_t rays_per_pair,
                                                                  const uint64_t ray_offset, const float4 * __restrict__ pair_mics, const v3 mic,
                                                                  const float4 * __restrict__ table, const float4 * __restrict__ bases, const uint32_t basis_stride)
{
    const uint32_t ncand = *count, ndirect = npairs > 1 ? npairs : 1u;
    const uint64_t total = (uint64_t) ncand + ndirect;
    for (uint64_t i = (uint64_t) blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (uint64_t) gridDim.x * blockDim.x) {
        rvb_impulse * imp;
        uint32_t pair = 0;
        if (i < ncand) {
            imp = &candidates[i].impulse;
            if (npairs > 1) pair = (uint32_t) ((candidates[i].ray - ray_offset) / rays_per_pair);
        } else {
            pair = (uint32_t) (i - ncand);
            imp = direct + pair;
        }
        if (pair >= ndirect) pair = ndirect - 1u;                    // (a candidate's ray is always one of the launch's)
        v3 m = mic;
        if (npairs > 1) { const float4 pm = pair_mics[pair]; m = mk3(pm.x, pm.y, pm.z); }
        const float4 * basis = bases + (size_t) pair * basis_stride;
        const v3 v = m - mk3(imp->position[0], imp->position[1], imp->position[2]);
        const float * g = reinterpret_cast<const float *>(table + 2 * (size_t) departure_row(basis[0], basis[1], basis[2], v));
#pragma unroll
        for (int b = 0; b < 8; ++b) imp->volume[b] = imp->volume[b] * g[b];
    }
}

// Which stores the streaming pass uses.  Measured at workload C2 (profiles/source_pattern_n1.txt); RVB_SOURCE_STORE = volumes | record |
// volumes_nt | record_nt chooses another form for measurements (read per launch; same bytes in memory either way).
enum StoreForm { STORE_VOLUMES = 0, STORE_RECORD = 1, STORE_VOLUMES_NT = 2, STORE_RECORD_NT = 3 };
StoreForm store_form()
{
    const char * e = getenv("RVB_SOURCE_STORE");
    if (!e) return STORE_RECORD;
    if (!strcmp(e, "volumes")) return STORE_VOLUMES;
    if (!strcmp(e, "volumes_nt")) return STORE_VOLUMES_NT;
    if (!strcmp(e, "record_nt")) return STORE_RECORD_NT;
    return STORE_RECORD;
}

template <bool FULL, bool NT>
void launch_records(const TraceArgs & a, const SourcePatternDev * patterns, uint32_t pattern_stride, uint64_t nrecords, hipStream_t s)
{
    const dim3 grid(stream_blocks(nrecords * 4, 256));
    float4 * records = reinterpret_cast<float4 *>(a.impulses);
    if (nrecords > 0xFFFFFFFFull)
        hipLaunchKernelGGL((source_pattern_kernel<FULL, NT, true>), grid, dim3(256), 0, s, records, nrecords, a.directions, patterns, pattern_stride,
                           a.nreflections, a.rays_per_pair, a.npairs, a.time_range);
    else
        hipLaunchKernelGGL((source_pattern_kernel<FULL, NT, false>), grid, dim3(256), 0, s, records, nrecords, a.directions, patterns, pattern_stride,
                           a.nreflections, a.rays_per_pair, a.npairs, a.time_range);
}

}  // namespace

// (the host forms of kernels.h, rvb_source_pattern_device_form and rvb_source_table_basis: source_state.hip)

void rvb_launch_source_table_rays(const TraceArgs & a, const SourceTableDev & t, hipStream_t s)
{
    if (!a.nrays) return;
    hipLaunchKernelGGL(source_table_rays_kernel, dim3(stream_blocks(a.nrays, 256)), dim3(256), 0, s, a.directions, reinterpret_cast<const float4 *>(t.table),
                       t.bases, t.basis_stride, a.rays_per_pair, a.nrays, reinterpret_cast<float4 *>(t.ray_gains));
}

void rvb_launch_source_table(const TraceArgs & a, const SourceTableDev & t, hipStream_t s)
{
    const uint64_t nrecords = a.nrays * a.nreflections;
    if (nrecords) {
        const dim3 grid(stream_blocks(nrecords * 4, 256));
        float4 * records = reinterpret_cast<float4 *>(a.impulses);
        const float4 * gains = reinterpret_cast<const float4 *>(t.ray_gains);
        if (nrecords > 0xFFFFFFFFull)
            hipLaunchKernelGGL((source_table_kernel<true>), grid, dim3(256), 0, s, records, nrecords, gains, a.nreflections, a.rays_per_pair, a.npairs, a.time_range);
        else
            hipLaunchKernelGGL((source_table_kernel<false>), grid, dim3(256), 0, s, records, nrecords, gains, a.nreflections, a.rays_per_pair, a.npairs, a.time_range);
    }
    // (the candidates: as in rvb_launch_source_pattern)
    const unsigned blocks = (unsigned) std::min<uint64_t>(std::max<uint64_t>((a.nrays * 9 + a.npairs + 255) / 256, 1), 64);
    hipLaunchKernelGGL(source_table_images_kernel, dim3(blocks), dim3(256), 0, s, a.candidates, a.candidate_count, a.direct, a.npairs, a.rays_per_pair,
                       a.ray_offset, a.pair_mics, mk3(a.mic[0], a.mic[1], a.mic[2]), reinterpret_cast<const float4 *>(t.table), t.bases, t.basis_stride);
}

void rvb_launch_source_pattern(const TraceArgs & a, const SourcePatternDev * patterns, uint32_t npatterns, hipStream_t s)
{
    const uint32_t pattern_stride = npatterns > 1 ? 1u : 0u;
    const uint64_t nrecords = a.nrays * a.nreflections;
    if (nrecords) {
        switch (store_form()) {
        case STORE_VOLUMES:    launch_records<false, false>(a, patterns, pattern_stride, nrecords, s); break;
        case STORE_VOLUMES_NT: launch_records<false, true>(a, patterns, pattern_stride, nrecords, s); break;
        case STORE_RECORD_NT:  launch_records<true, true>(a, patterns, pattern_stride, nrecords, s); break;
        default:               launch_records<true, false>(a, patterns, pattern_stride, nrecords, s); break;
        }
    }
    // candidates: at most nrays * 9, in practice a few thousand; the count is on the device, so a fixed small grid strides over them
    const unsigned blocks = (unsigned) std::min<uint64_t>(std::max<uint64_t>((a.nrays * 9 + a.npairs + 255) / 256, 1), 64);
    hipLaunchKernelGGL(source_pattern_images_kernel, dim3(blocks), dim3(256), 0, s, a.candidates, a.candidate_count, a.direct, a.npairs, a.rays_per_pair,
                       a.ray_offset, a.pair_mics, mk3(a.mic[0], a.mic[1], a.mic[2]), patterns, pattern_stride);
}
