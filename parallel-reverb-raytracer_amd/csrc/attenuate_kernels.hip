// attenuate_kernels.hip — the materialised per-impulse streaming stages: microphone / HRTF attenuation (reference rayverb/kernel.cpp:505-625,
// kernels `attenuate` and `hrtf`), the time range behind findPredelay (rayverb/rayverb.h:49-74) and fixPredelay (rayverb.h:76-90).
//
// These are HBM-bound: 64 B in (+ 64 B out) per impulse.  Impulses are 64-byte records, and four lanes share one — 16 B per lane, so
// that one wave instruction covers a contiguous 1 KiB; what the quad needs of the whole record goes round by DPP (quad_record).
#include "attenuation.h"

#define ATT_UNROLL 1      // 16-byte chunks per lane per pass; with one workgroup per 4 KiB the dispatcher provides the parallelism

namespace {

// One 16-byte chunk of one impulse per lane: chunk 0/1 = volume, 2 = position, 3 = time.
// Speaker model (kernel.cpp:505-535).  The two normalisations of kernel.cpp:511/:528 are three divisions each
// by the same length: lane k of the quad divides component k, so a wave spends ONE correctly rounded division
// per normalisation instead of three (same operations on the same operands: bit-identical results).
__device__ __forceinline__ float4 attenuate_chunk_speaker(const ModelDev & m, uint32_t ch, uint32_t q, const float4 v)
{
    const QuadRecord r = quad_record(q, v);                        // kernel.cpp:524 any(volume != 0)
    float4 o = make_float4(0, 0, 0, 0);
    if (r.nonzero) {
        const v3 d = r.pos - m.mic;                                // getDirection, kernel.cpp:528
        const float len = length3(d);
        const float own = q == 0 ? d.x : (q == 1 ? d.y : d.z);
        const float n_own = len == 0.0f ? own : own / len;         // normalize3: a zero vector stays zero
        const v3 n = mk3(dpp_f<QP_BCAST(0)>(n_own), dpp_f<QP_BCAST(1)>(n_own), dpp_f<QP_BCAST(2)>(n_own));
        const float len2 = length3(n);                             // kernel.cpp:511 normalises the unit vector again
        const float u_own = len2 == 0.0f ? n_own : n_own / len2;
        const v3 u = mk3(dpp_f<QP_BCAST(0)>(u_own), dpp_f<QP_BCAST(1)>(u_own), dpp_f<QP_BCAST(2)>(u_own));
        const float g = (1 - m.coeff[ch]) + m.coeff[ch] * dot3(u, m.sdir[ch]);
        if (q < 2) o = make_float4(v.x * g, v.y * g, v.z * g, v.w * g);
        else if (q == 2) o.x = r.time;
    }
    return o;
}

// HRTF model (kernel.cpp:586-625): table row by azimuth / elevation, per-ear arrival-time shift
__device__ __forceinline__ float4 attenuate_chunk_hrtf(const ModelDev & m, uint32_t ch, uint32_t q, const float4 v)
{
    const QuadRecord r = quad_record(q, v);                        // kernel.cpp:607
    float4 o = make_float4(0, 0, 0, 0);
    if (r.nonzero) {
        const int64_t row = hrtf_row_quad(m, r.pos, q);
        if (q < 2) {
            const float4 t = reinterpret_cast<const float4 *>(m.table + ((uint64_t) ch * RVB_HRTF_ROWS + (uint64_t) row) * 8)[q];
            o = make_float4(v.x * t.x, v.y * t.y, v.z * t.z, v.w * t.w);
        } else if (q == 2) {
            o.x = hrtf_time(m, ch, r.pos, r.time);
        }
    }
    return o;
}

// (the ATT_UNROLL loops stay although ATT_UNROLL is 1: a plain grid-stride loop compiles to slightly different code)
template <bool HRTF>
__global__ __launch_bounds__(256) void attenuate_kernel(ModelDev m, uint32_t ch, const float4 * __restrict__ in,
                                                        float4 * __restrict__ out, uint64_t n)
{
    const uint32_t q = threadIdx.x & 3u;
    const uint64_t nchunks = n * 4;                                // whole quads: a quad's four chunks are live together
    const uint64_t stride = (uint64_t) gridDim.x * blockDim.x;
    for (uint64_t c0 = (uint64_t) blockIdx.x * blockDim.x + threadIdx.x; c0 < nchunks; c0 += stride * ATT_UNROLL) {
        float4 v[ATT_UNROLL];
#pragma unroll
        for (int u = 0; u < ATT_UNROLL; ++u) {                    // all loads leave before the first result is needed
            const uint64_t c = c0 + (uint64_t) u * stride;
            v[u] = make_float4(0, 0, 0, 0);
            if (c < nchunks) {
                const nt_float4_t t = __builtin_nontemporal_load(reinterpret_cast<const nt_float4_t *>(in + c));
                v[u] = make_float4(t.x, t.y, t.z, t.w);
            }
        }
#pragma unroll
        for (int u = 0; u < ATT_UNROLL; ++u) {
            const uint64_t c = c0 + (uint64_t) u * stride;
            if (c < nchunks) {
                const float4 o = HRTF ? attenuate_chunk_hrtf(m, ch, q, v[u]) : attenuate_chunk_speaker(m, ch, q, v[u]);
                const nt_float4_t t = {o.x, o.y, o.z, o.w};
                __builtin_nontemporal_store(t, reinterpret_cast<nt_float4_t *>(out + c));
            }
        }
    }
}

// min non-zero / max attenuated time (the inputs of findPredelay, rayverb.h:49-74, and of MAX_SAMPLE, rayverb.cpp:57).
// Four lanes per impulse like attenuate_kernel: one 16-byte chunk per lane (1 KiB per wave instruction), position and
// time broadcast by DPP, so the per-ear time shift (two square roots per ear) is evaluated once per 16 impulses and wave
// instruction — the former 16-lanes-per-impulse layout spent four times the instructions on it and ran at 0.9 TB/s.
__global__ __launch_bounds__(256) void time_range_kernel(ModelDev m, const float4 * __restrict__ in, uint64_t n, uint32_t * range)
{
    const uint32_t q = threadIdx.x & 3u;
    const uint64_t nchunks = n * 4;
    float tmin = __builtin_inff(), tmax = 0.0f;
    for (uint64_t c = (uint64_t) blockIdx.x * blockDim.x + threadIdx.x; c < nchunks; c += (uint64_t) gridDim.x * blockDim.x) {
        const nt_float4_t t4 = __builtin_nontemporal_load(reinterpret_cast<const nt_float4_t *>(in + c));
        const QuadRecord r = quad_record(q, make_float4(t4.x, t4.y, t4.z, t4.w));
        if (!r.nonzero)
            continue;           // attenuated impulse is {0, 0}: no part in findPredelay / maxtime
        // speaker channels all keep the input time; of the two ears, the quad's even lanes take the left one and the odd lanes the
        // right one (the wave-wide reduction below joins them): one time shift — two square roots — per lane instead of two
        const float t = attenuated_time(m, q & 1u, r.pos, r.time);
        if (t != 0.0f) tmin = fminf(tmin, t);
        tmax = fmaxf(tmax, t);
    }
    for (int off = 32; off > 0; off >>= 1) {
        tmin = fminf(tmin, __shfl_xor(tmin, off));
        tmax = fmaxf(tmax, __shfl_xor(tmax, off));
    }
    // One atomic per wave only when it can still move the result: with one workgroup per 4 KiB there are millions of waves,
    // and that many atomics on two addresses serialise (70 ms at 12.8 M impulses).  A stale read only costs a redundant atomic.
    if ((threadIdx.x & 63u) == 0) {
        const volatile uint32_t * seen = range;
        if (tmin != __builtin_inff() && __float_as_uint(tmin) < seen[0]) atomicMin(range + 0, __float_as_uint(tmin));
        if (__float_as_uint(tmax) > seen[1]) atomicMax(range + 1, __float_as_uint(tmax));
    }
}

// fixPredelay (rayverb.h:76-90) on a resident AttenuatedImpulse array: the time is the first float of the third 16-byte chunk
__global__ __launch_bounds__(256) void fix_predelay_kernel(rvb_attenuated_impulse * __restrict__ a, uint64_t n, float seconds)
{
    for (uint64_t i = (uint64_t) blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (uint64_t) gridDim.x * blockDim.x) {
        const float t = a[i].time;
        a[i].time = t > seconds ? t - seconds : 0.0f;
    }
}

}  // namespace

void rvb_launch_attenuate(const AttenuationModel & m, uint32_t channel, const rvb_impulse * in, uint64_t n,
                          rvb_attenuated_impulse * out, hipStream_t s)
{
    if (n == 0) return;
    const dim3 grid(stream_blocks((n * 4 + ATT_UNROLL - 1) / ATT_UNROLL, 256));
    if (m.hrtf)
        hipLaunchKernelGGL(attenuate_kernel<true>, grid, dim3(256), 0, s, make_model(m), channel,
                           reinterpret_cast<const float4 *>(in), reinterpret_cast<float4 *>(out), n);
    else
        hipLaunchKernelGGL(attenuate_kernel<false>, grid, dim3(256), 0, s, make_model(m), channel,
                           reinterpret_cast<const float4 *>(in), reinterpret_cast<float4 *>(out), n);
}

void rvb_launch_time_range(const AttenuationModel & m, const rvb_impulse * in, uint64_t n, uint32_t * range, hipStream_t s)
{
    if (n == 0) return;
    // Every wave ends with two reads of the same two result words (and an atomic when it can still move them): with one workgroup
    // per 4 KiB — the launch shape the other streaming kernels want — that is 1.6 M reads of one line, which, not HBM, then sets the
    // kernel's time (0.34 ms at 12.8 M impulses; 0.17 ms with 2 048 grid-strided workgroups, 0.18 with 8 192, 0.25 with 65 536).
    hipLaunchKernelGGL(time_range_kernel, dim3(std::min(stream_blocks(n * 4, 256), 2048u)), dim3(256), 0, s, make_model(m),
                       reinterpret_cast<const float4 *>(in), n, range);
}

void rvb_launch_fix_predelay(rvb_attenuated_impulse * a, uint64_t n, float seconds, hipStream_t s)
{
    if (n == 0) return;
    hipLaunchKernelGGL(fix_predelay_kernel, dim3(stream_blocks(n, 256)), dim3(256), 0, s, a, n, seconds);
}
