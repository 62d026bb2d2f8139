// attenuation.h — what attenuate_kernels.hip, histogram_kernels.hip and exact_kernels.hip share: the microphone / HRTF attenuation model
// (reference rayverb/kernel.cpp:505-625), predelay and time bin (rayverb/rayverb.h:49-97, rayverb/rayverb.cpp:48-77), and the ways a wave
// reads the 64-byte impulse records.  All in an unnamed namespace: the kernels' symbols carry `(anonymous namespace)::ModelDev`.
#pragma once

#include <algorithm>
#include <cstdlib>

#include "kernels.h"
#include "quad.h"
#include "rvb_math.h"

namespace {

typedef float nt_float4_t __attribute__((ext_vector_type(4)));

struct ModelDev {
    int hrtf;
    uint32_t nchannels;
    v3 mic;
    v3 sdir[8];             // speaker directions, already normalised (kernel.cpp:511)
    float coeff[8];
    const float * table;    // [2][RVB_HRTF_ROWS][8]
    v3 pointing, up;
    v3 bx, by, bz;          // the listener's basis of kernel.cpp:538-549 — it depends on (pointing, up) only, so it is computed once
                            // on the host with the same operations (rvb_math.h is shared) instead of once per impulse
    v3 ear[2];              // kernel.cpp:599-603
    bool exact_rows;        // measurement / test switch RVB_HRTF_EXACT_ROWS=1: every table row through the binary64 atan2 (angle_deg)
};

// reference kernel.cpp:537-549
__host__ __device__ __forceinline__ v3 transform3(v3 pointing, v3 up, v3 d)
{
    v3 x = normalize3(cross3(up, pointing));
    v3 y = cross3(pointing, x);
    v3 z = pointing;
    return mk3(dot3(x, d), dot3(y, d), dot3(z, d));
}

// A speaker as the kernels take it: the direction normalised (kernel.cpp:511, on the host with the device's operations), then the
// coefficient.  The eight-channel kernels get these bits as kernel arguments (make_model), the wide fold from its table in device memory.
inline float4 speaker_device_form(const rvb_speaker & s)
{
    const v3 d = normalize3(mk3(s.direction[0], s.direction[1], s.direction[2]));
    return make_float4(d.x, d.y, d.z, s.coefficient);
}

ModelDev make_model(const AttenuationModel & m)
{
    ModelDev d;
    d.hrtf = m.hrtf;
    d.nchannels = m.nchannels;
    d.mic = mk3(m.mic[0], m.mic[1], m.mic[2]);
    for (int i = 0; i < 8; ++i) {
        const float4 s = speaker_device_form(m.speakers[i]);
        d.sdir[i] = mk3(s.x, s.y, s.z);
        d.coeff[i] = s.w;
    }
    d.table = m.hrtf_table;
    d.pointing = mk3(m.facing[0], m.facing[1], m.facing[2]);
    d.up = mk3(m.up[0], m.up[1], m.up[2]);
    d.bx = normalize3(cross3(d.up, d.pointing));
    d.by = cross3(d.pointing, d.bx);
    d.bz = d.pointing;
    const float width = 0.1f;                                   // kernel.cpp:597
    d.ear[0] = transform3(d.pointing, d.up, mk3(-width, 0.0f, 0.0f)) + d.mic;
    d.ear[1] = transform3(d.pointing, d.up, mk3(width, 0.0f, 0.0f)) + d.mic;
    const char * e = getenv("RVB_HRTF_EXACT_ROWS");          // (read per launch: a test flips it inside one process)
    d.exact_rows = e && e[0] == '1';
    return d;
}

__device__ __forceinline__ float atan2_cr(float y, float x) { return (float) atan2((double) y, (double) x); }

// reference kernel.cpp:505-513: gain of one speaker for an impulse at `pos`
__device__ __forceinline__ float speaker_gain(const ModelDev & m, uint32_t ch, v3 pos)
{
    const v3 direction = normalize3(pos - m.mic);               // getDirection, kernel.cpp:528
    return (1 - m.coeff[ch]) + m.coeff[ch] * dot3(normalize3(direction), m.sdir[ch]);
}

// speaker_gain in its two steps, for a kernel that takes the direction once per impulse and the gain once per channel
// (reshade_grad_kernels.hip): same operations on the same operands
__device__ __forceinline__ v3 arrival_direction(const ModelDev & m, v3 pos) { return normalize3(normalize3(pos - m.mic)); }
__device__ __forceinline__ float speaker_gain_toward(const ModelDev & m, uint32_t ch, v3 direction)
{
    return (1 - m.coeff[ch]) + m.coeff[ch] * dot3(direction, m.sdir[ch]);
}

// rvb_source_pattern's gain of one band (source_kernels.hip): from the band's shape and d = dot3(normalize3(normalize3(v)), direction)
__device__ __forceinline__ float band_gain(const float shape, const float d) { return (1 - shape) + shape * d; }

// reference kernel.cpp:563-584: table row selected for an impulse at `pos` (same for both ears)
// transform (kernel.cpp:538-549) with the precomputed basis: the three dot products that remain per impulse
__device__ __forceinline__ v3 to_listener(const ModelDev & m, v3 d)
{
    return mk3(dot3(m.bx, d), dot3(m.by, d), dot3(m.bz, d));
}

// Table row = a * 180 + e with a = (long) (degrees(azimuth) + 180) % 360, e = 90 - (long) degrees(elevation) (kernel.cpp:569-584).
// Only the INTEGER parts of the two angles in degrees matter.  The oracle's atan2 is the correctly rounded binary32 value
// (evaluated in binary64: ~150 double-precision instructions per call); here the angle is first taken with the binary32 atan2f
// (~40 instructions) and the binary64 evaluation is kept for the cases where that could change the integer part:
//   deg_fast and deg_exact differ by at most 57.3 * |atan2f - atan2| + two roundings of a value <= 360
//   <= 57.3 * 1.5e-6 (atan2f: 6 ulp of pi at most, OpenCL / ocml accuracy) + 2 * 1.6e-5 < 1.2e-4 degrees,
// so an angle that is farther than kAngleMargin = 2e-3 degrees from every integer truncates to the same integer either way
// (about 0.4 % of the angles are nearer and take the binary64 path; NaN compares false and takes it too).
// tests/test_gpu_fullsize.py holds whole traces' rows against the always-exact evaluation (RVB_HRTF_EXACT_ROWS=1);
// tests/test_gpu_attenuation_edges.py holds all three evaluations against the oracle on angles constructed round every integer boundary.
#define RVB_DEG_PER_RAD 57.295779513082320877f
__device__ __forceinline__ float angle_deg(float y, float x, float offset, bool always_exact)
{
    float deg = atan2f(y, x) * RVB_DEG_PER_RAD + offset;
    const float kAngleMargin = 2e-3f;
    const bool sure = fabsf(deg - rintf(deg)) > kAngleMargin;
    if (!sure || always_exact)
        deg = atan2_cr(y, x) * RVB_DEG_PER_RAD + offset;        // the reference's operations on the correctly rounded angle
    return deg;
}

__device__ __forceinline__ int64_t row_of(float az_deg_plus_180, float el_deg)
{
    int64_t a = (int64_t) az_deg_plus_180;
    a %= 360;
    int64_t e = (int64_t) el_deg;
    e = 90 - e;
    return a * 180 + e;     // e == 180 runs into the next azimuth row (quirk Q5); row 360*180 is zero padding
}

__device__ __forceinline__ int64_t hrtf_row(const ModelDev & m, v3 pos)
{
    const v3 t = to_listener(m, normalize3(pos - m.mic));
    const float az = angle_deg(t.x, t.z, 180.0f, m.exact_rows);
    const float el = angle_deg(t.y, sqrtf(t.x * t.x + t.z * t.z), 0.0f, m.exact_rows);
    return row_of(az, el);
}

// The table row of a tabulated source directivity (source_kernels.hip, image_grad_kernels.hip) for the departure vector `v`: hrtf_row
// with pos - mic replaced by v — the listener's basis is the source's (bx, by, bz of rvb_source_table_basis), the margin scheme of angle_deg and quirk Q5 of row_of included.  A row outside the table
// (finite inputs give none) reads the zero row: no address outside the table is formed.
__device__ __forceinline__ uint32_t departure_row(const float4 bx, const float4 by, const float4 bz, const v3 v)
{
    const v3 d = normalize3(v);
    const v3 t = mk3(dot3(mk3(bx.x, bx.y, bx.z), d), dot3(mk3(by.x, by.y, by.z), d), dot3(mk3(bz.x, bz.y, bz.z), d));
    const float az = angle_deg(t.x, t.z, 180.0f, false);
    const float el = angle_deg(t.y, sqrtf(t.x * t.x + t.z * t.z), 0.0f, false);
    const int64_t row = row_of(az, el);
    return row >= 0 && row < RVB_HRTF_ROWS ? (uint32_t) row : (uint32_t) (RVB_HRTF_ROWS - 1);
}

// The same row for two neighbouring lanes that share one impulse (a quad of attenuate_kernel, the two lanes of a bin in
// ordered_sum_hrtf_kernel): azimuth and elevation are both atan2(y, x) of different arguments, so the even lane evaluates the
// azimuth and the odd lane the elevation with ONE call, then they swap by DPP.  Same operations on the same operands as hrtf_row.
__device__ __forceinline__ int64_t hrtf_row_quad(const ModelDev & m, v3 pos, uint32_t q)
{
    const v3 t = to_listener(m, normalize3(pos - m.mic));
    const bool odd = q & 1u;
    const float y = odd ? t.y : t.x;
    const float x = odd ? sqrtf(t.x * t.x + t.z * t.z) : t.z;
    const float deg = angle_deg(y, x, odd ? 0.0f : 180.0f, m.exact_rows);
    const float other = dpp_f<QP_SWAP1>(deg);               // quad_perm [1,0,3,2]: the pair lane's angle
    return row_of(odd ? other : deg, odd ? deg : other);
}

// reference kernel.cpp:616-622: arrival-time shift of one ear
__device__ __forceinline__ float hrtf_time(const ModelDev & m, uint32_t ch, v3 pos, float time)
{
    const float dist0 = length3(pos - m.mic);
    const float dist1 = length3(pos - m.ear[ch]);
    const float diff = dist1 - dist0;
    return time + diff * seconds_per_meter();
}

__device__ __forceinline__ float attenuated_time(const ModelDev & m, uint32_t ch, v3 pos, float time)
{
    return m.hrtf ? hrtf_time(m, ch, pos, time) : time;
}

// rayverb.h:89 fixPredelay, then rayverb.cpp:69 SAMPLE = round(time * samplerate)
__device__ __forceinline__ uint32_t time_bin(float time, float predelay, float sample_rate)
{
    const float t = time > predelay ? time - predelay : 0.0f;
    return (uint32_t) roundf(t * sample_rate);
}

// kernel.cpp:524 / :607 any(volume != 0) of a record's two volume chunks.  A macro, not a function: the || chain lets the compiler put
// off the later loads, and a function (arguments by value or by reference) changed the code of the kernels that use it.
#define ANY_VOLUME(v0, v1) ((v0).x != 0.0f || (v0).y != 0.0f || (v0).z != 0.0f || (v0).w != 0.0f \
                         || (v1).x != 0.0f || (v1).y != 0.0f || (v1).z != 0.0f || (v1).w != 0.0f)

// Four lanes per record, one 16-byte chunk `v` per lane (chunk 0/1 = volume, 2 = position, 3 = time): position and time broadcast to
// the quad by DPP, and whether any of the record's eight volumes is non-zero.
struct QuadRecord { v3 pos; float time; uint32_t nonzero; };
__device__ __forceinline__ QuadRecord quad_record(uint32_t q, const float4 v)
{
    QuadRecord r;
    r.pos = mk3(dpp_f<QP_BCAST(2)>(v.x), dpp_f<QP_BCAST(2)>(v.y), dpp_f<QP_BCAST(2)>(v.z));
    r.time = dpp_f<QP_BCAST(3)>(v.x);
    r.nonzero = (q < 2 && (v.x != 0.0f || v.y != 0.0f || v.z != 0.0f || v.w != 0.0f)) ? 1u : 0u;
    r.nonzero |= dpp_u<QP_SWAP1>(r.nonzero);
    r.nonzero |= dpp_u<QP_SWAP2>(r.nonzero);
    return r;
}

// Entries [k, k + N) of a bin's run [lo, hi) of the sorted list, for the lane that folds band half `half`: the N index loads, then the
// N record gathers (v: the lane's half of the volume, p: the position), leave together.  An entry past the run repeats its first
// record and the caller skips it.  Record numbers below ndiffuse are diffuse impulses, the rest images.
template <int N>
__device__ __forceinline__ void gather_records(const uint32_t * __restrict__ values, uint64_t k, uint64_t lo, uint64_t hi, const rvb_impulse * __restrict__ diffuse,
                                               uint64_t ndiffuse, const rvb_impulse * __restrict__ images, uint32_t half, float4 (&v)[N], float4 (&p)[N])
{
#pragma unroll
    for (int u = 0; u < N; ++u) {
        const uint64_t kk = k + u < hi ? k + u : lo;
        const uint64_t idx = values[kk];
        const rvb_impulse * imp = idx < ndiffuse ? diffuse + idx : images + (idx - ndiffuse);
        const float4 * r = reinterpret_cast<const float4 *>(imp);
        v[u] = r[half];
        p[u] = r[2];
    }
}

// first word of row (channel, band half * 4 + b) of the histogram [channel][8][nbins]
__device__ __forceinline__ uint64_t hist_row(uint32_t ch, uint32_t half, int b, uint64_t nbins) { return ((uint64_t) ch * 8 + half * 4 + b) * nbins; }

// Workgroups for a streaming kernel of `items` work-items: one per `per_block` items, at least one.  NOT capped at a few workgroups per
// CU: measured on MI355X (tools/copy_probe.hip, 819 MB -> 819 MB, 16 B per lane) a grid-strided 2048-workgroup launch moves
// 4.5-5.3 TB/s, one workgroup per 4 KiB moves 6.1-6.5 TB/s — the dispatcher then sweeps HBM as one moving window instead of 2048
// streams 8 MB apart.  The kernels keep their grid-stride loops for the (never reached in practice) 2^31-workgroup limit.
inline unsigned stream_blocks(uint64_t items, unsigned per_block)
{
    const uint64_t blocks = (items + per_block - 1) / per_block;
    return (unsigned) std::min<uint64_t>(std::max<uint64_t>(blocks, 1), 0x7FFFFFFFull);
}

}  // namespace
