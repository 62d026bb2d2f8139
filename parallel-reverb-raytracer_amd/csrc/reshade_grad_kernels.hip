// reshade_grad_kernels.hip — material gradients of a weighted impulse response from a kept trace (rvb_reshade_grad of
// include/rvb_capi.h): dL/dspecular, dL/ddiffuse of every surface and dL/dair of every band for L = sum w * H, H the histogram that the fast
// mode's binning adds for the diffuse records of one pair under a speaker model.  No reference counterpart.  A record's volume is the product
// of reshade_kernels.hip,
//     volume_b(k) = P_k * air_attenuation(dist_k, air_b) * diffuse[s_k][b] * DIFF(k) * pattern_b,   P_k = prod_{j<=k} -specular[s_j][b],
// so with a_k = air_attenuation * DIFF * pattern_b * sum_c w[c][b][bin_k] * gain_c(k) (0 for a record that is invisible or past the histogram)
//     dL/ddiffuse[s_k][b]  += P_k * a_k
//     dL/dair_b            += P_k * a_k * diffuse[s_k][b] * dist_k * ln((float) M_E)
//     dL/dspecular[s_j][b] += -P_{j-1} * B_j,   B_j = a_j * diffuse[s_j][b] + (-specular[s_{j+1}][b]) * B_{j+1}
// and no division by a coefficient anywhere: a coefficient that is 0 gets its derivative like any other.
//   reshade_grad_weights_kernel   the weights from the histogram's layout [channel][8][nbins] into the accumulation image's
//                                 [bin][channel][band]: a record then gathers ONE run of 32 * nchannels bytes.
//   reshade_grad_kernel           reshade_kernel's shape: a wave takes eight rays, lane (ray, band) owns a chain (the staged records' rows, the
//                                 side record, the chain step and the two-lane read of a record: kept_tiles.h).  A first sweep over
//                                 the side records' surfaces leaves P at every tile start in LDS; then the tiles in REVERSE: the tile's
//                                 records two lanes per record (distance, bin, arrival direction — what does not depend on the band) into
//                                 LDS, the lane's weight gathers of the tile, its chain forward over the tile (P, a_k, the diffuse and air
//                                 terms), then backward (B_j, the specular terms).  It stores no record.  Terms are binary32 with the trace's own functions; they are added
//                                 in binary64: the eight rays of a wave that hit the same surface are combined in ray order by the first
//                                 of them, which alone updates the wave's table in LDS — no atomics, one fixed order.
//   reshade_grad_reduce_kernel    the workgroups' tables added in a fixed order, rounded to binary32 once.
// A table in LDS holds GRAD_WINDOW surfaces; a scene with more is swept once per window of surfaces.
//   reshade_grad_kernel<.., true> the TERMS PASS of rvb_reshade_grad_map (reshade_grad_map_kernels.hip holds the fold behind it): the same
//                                 body, but a term goes to its record's row of 16 floats instead of into the table — the eight diffuse
//                                 terms P_k a_k behind the eight specular ones -P_{k-1} B_k —, staged per tile in LDS where the table
//                                 stands otherwise and stored as whole 64-byte rows, a ray's run of a tile in one piece; beside it the
//                                 record's sort key (its triangle, ntriangles for a slot without a record) and its number.
#include "grad_tiles.h"

#include <algorithm>

namespace {

// (GRAD_TILE, GradRows, GRAD_BIN_WORD, GRAD_GATHER, GRAD_STAGE_WORDS: grad_tiles.h, shared with source_grad_kernels.hip)
#define GRAD_WINDOW 64u             // surfaces per table in LDS (8 KiB of binary64 sums)
#define GRAD_MAX_BLOCKS 16384u       // (4096 left every wave three or four groups of rays at workload C2: 1.87 ms against 1.71 ms, profiles/reshade_grad_n1.txt)
#define GRAD_PARTIAL_BYTES (64ull << 20)        // the partial tables of a launch stay below this (or at 64 tables)
#define GRAD_TR_BINS 64u

struct GradDev {
    ModelDev m;
    ReshadeGradArgs g;
    uint32_t ngroups, ntiles;
    uint32_t surface0, window;       // this sweep's surfaces [surface0, surface0 + window)
    uint32_t entries;                // binary64 sums per partial table: nsurfaces * 16 + 8
    double * partials;
    // the terms pass (MAP): rows, keys and values by the record's number within the pair; listen by its number within the kept launch
    float4 * terms;
    uint32_t * keys, * values;
    const uint2 * listen;
    uint32_t ntriangles;
};

// LDS of a wave, in words: the table (window * 16 + 8 doubles), a GradRows region of staged records twice (float4 each), [TILE][WAVE] floats twice
// (a_k * diffuse and P_{k-1} of the forward sweep, for the backward one), [ntiles][WAVE] chain checkpoints, the surface table (stage_surfaces)
// (the terms pass: in the table's place the tile's term rows, [RAYS][TILE] rows of 16 floats, a ray's rows padded by 8 words so that the
// 64 lanes of a sweep's store fall into 64 banks)
#define GRAD_TERM_RAY_WORDS (GRAD_TILE * 16u + 8u)
#define GRAD_TERM_WORDS (GradRows::RAYS * GRAD_TERM_RAY_WORDS)
__host__ __device__ __forceinline__ uint32_t grad_table_words(uint32_t window, bool map = false) { return map ? GRAD_TERM_WORDS : (window * 16u + 8u) * 2u; }
__host__ __device__ __forceinline__ uint32_t grad_surfaces_at(uint32_t window, uint32_t ntiles, bool map = false)
{
    return grad_table_words(window, map) + 2u * GRAD_STAGE_WORDS + 2u * GRAD_TILE * WAVE + ntiles * WAVE;
}

// `v` of this lane's (ray, band) added to column `column` of its surface's row: the rays of the wave that hit the same surface are summed
// in ray order, in binary64, and the first of them updates the table — every address of one update is written by one lane.  Called by the
// whole wave (the shuffles read every lane); surface NONE adds nothing.
__device__ __forceinline__ void add_by_surface(double * table, const GradDev & d, const uint32_t lane, const uint32_t surface, const uint32_t column, const float v)
{
    const uint32_t band = lane & 7u, ray = lane >> 3;
    double sum = 0.0;
    bool first = true;
#pragma unroll
    for (uint32_t o = 0; o < GradRows::RAYS; ++o) {
        const uint32_t so = __shfl(surface, (int) (o * 8u + band));
        const float vo = __shfl(v, (int) (o * 8u + band));
        if (so == surface) {
            sum += (double) vo;
            first = first && o >= ray;
        }
    }
    const uint32_t local = surface - d.surface0;          // (NONE lands past every window)
    if (first && surface != NONE && local < d.window)
        table[local * 16u + column] += sum;
}

// Where a term goes: column `column` of surface `surface`'s row of the table (add_by_surface), or, MAP, of the row of record (r, k) of
// the tile staged in LDS.  Called by the whole wave.
template <bool MAP>
__device__ __forceinline__ void put_term(double * table, float * rows, const GradDev & d, const uint32_t lane, const uint32_t k, const uint32_t surface,
                                         const uint32_t column, const float v)
{
    if (MAP) {
        if (surface != NONE) rows[(lane >> 3) * GRAD_TERM_RAY_WORDS + k * 16u + column] = v;
    } else {
        add_by_surface(table, d, lane, surface, column, v);
    }
}

template <bool SURF_LDS, bool MAP>
__global__ __launch_bounds__(WAVE) void reshade_grad_kernel(TraceArgs a, GradDev d, const float4 * __restrict__ kept)
{
    extern __shared__ __attribute__((aligned(16))) uint32_t lds[];
    double * table = reinterpret_cast<double *>(lds);
    float * rows = reinterpret_cast<float *>(lds);                           // MAP: the tile's term rows instead
    uint32_t * side_words = lds + grad_table_words(d.window, MAP);
    float4 * side = reinterpret_cast<float4 *>(side_words);                  // staged records (GRAD_BIN_WORD)
    float4 * toward = side + GradRows::RECORDS;                              // the record's arrival direction at the microphone
    float * us = reinterpret_cast<float *>(toward + GradRows::RECORDS);      // a_k * diffuse[s_k][b]
    float * prevs = us + GRAD_TILE * WAVE;                                   // P_{k-1}
    float * starts = prevs + GRAD_TILE * WAVE;                               // P at the start of every tile
    const lds_float4_ptr surf_lds = stage_surfaces(a, lds + grad_surfaces_at(d.window, d.ntiles, MAP));
    const ReshadeGradArgs & g = d.g;
    const uint32_t lane = threadIdx.x, h = lane & 1u, r = lane >> 3, band = lane & 7u;
    const uint32_t nch = d.m.nchannels, cb = nch * 8u;
    const float air = a.air[band];
    const v3 mic = mk3(g.mic[0], g.mic[1], g.mic[2]);
    if (!MAP)
        for (uint32_t i = lane; i < d.window * 16u + 8u; i += WAVE) table[i] = 0.0;
    double air_sum = 0.0;
    for (uint32_t grp = blockIdx.x; grp < d.ngroups; grp += gridDim.x) {
        const uint32_t ray0 = grp * GradRows::RAYS;                             // within the pair
        // the source pattern's gain of this lane's band: constant along the ray (source_pattern_kernel, v = the ray's own direction)
        // (or the source table's, from the gains that source_table_rays_kernel left for the ray)
        float pattern_gain = 1.0f;
        if (g.ray_gains) {
            pattern_gain = g.ray_gains[(size_t) (ray0 + r < g.nrays ? ray0 + r : g.nrays - 1u) * 8u + band];
        } else if (g.has_pattern) {
            const float4 dv = a.directions[ray0 + r < g.nrays ? ray0 + r : g.nrays - 1u];
            const v3 u = normalize3(normalize3(mk3(dv.x, dv.y, dv.z)));
            pattern_gain = band_gain(g.pattern.shape[band], dot3(u, mk3(g.pattern.direction[0], g.pattern.direction[1], g.pattern.direction[2])));
        }
        // ---- the chain at every tile start: kernel.cpp:461 over the side records' surfaces alone
        {
            float vol = 1.0f;
            bool alive = true;
            for (uint32_t t = 0; t < d.ntiles; ++t) {
                starts[t * WAVE + lane] = vol;
                if (t + 1u == d.ntiles) break;
                __syncthreads();                                             // (the tile before has been read)
                for (uint32_t i = lane; i < GradRows::RAYS * GRAD_TILE; i += WAVE) {
                    const uint32_t rr = i / GRAD_TILE, k = i % GRAD_TILE, bounce = t * GRAD_TILE + k;
                    uint32_t s = NONE;
                    if (ray0 + rr < g.nrays && bounce < a.nreflections)
                        s = SideRecord::surface_of(kept, (g.first_ray + ray0 + rr) * a.nreflections + bounce);
                    side_words[GradRows::surface_word(rr, k)] = s;
                }
                __syncthreads();
                for (uint32_t k = 0; k < GRAD_TILE && alive; ++k) {
                    const uint32_t surface = side_words[GradRows::surface_word(r, k)];
                    if (surface == NONE) {                                   // escaped (or past the last ray): no record from here on
                        alive = false;
                        break;
                    }
                    vol = chain_step<SURF_LDS>(a, surf_lds, vol, surface, band);
                }
            }
        }
        // ---- the tiles in reverse
        float carry = 0.0f;                                                  // (-specular[s_{j+1}][b]) * B_{j+1}
        for (uint32_t t = d.ntiles; t-- > 0;) {
            const uint32_t first = t * GRAD_TILE;
            __syncthreads();                                                 // (what the wave read of the stage before)
            // (1) the tile's records, two lanes per record (FinishedRecord), as reshade_kernel reads them
            for (uint32_t j = lane >> 1; j < GradRows::RAYS * GRAD_TILE; j += WAVE / 2) {
                const uint32_t rr = j / GRAD_TILE, k = j % GRAD_TILE;
                const bool inside = ray0 + rr < g.nrays && first + k < a.nreflections;
                const uint64_t record = inside ? (g.first_ray + ray0 + rr) * a.nreflections + first + k : 0;
                float4 sd = SideRecord::none();
                if (inside) sd = load_stream(kept + record);
                const FinishedRecord fin = FinishedRecord::read(reinterpret_cast<const float4 *>(a.impulses + record), inside, h);
                const v3 p = fin.position();
                const float time = fin.time();
                const bool visible = fin.visible(sd);
                const float dist = dist_to_mic(sd, p, mic);
                const uint32_t bin = time_bin(time, g.predelay, g.sample_rate);
                const bool adds = visible && bin < g.nbins;
                const v3 dir = arrival_direction(d.m, p);
                float4 staged = SideRecord::make(dist, SideRecord::diff(sd), SideRecord::surface(sd));
                staged.w = __uint_as_float(adds ? bin : NONE);
                if (h == 0) side[GradRows::at(rr, k)] = staged;
                else toward[GradRows::at(rr, k)] = make_float4(dir.x, dir.y, dir.z, 0.0f);
                if (MAP && inside) {                                         // the record's sort entry: lane 0 the key, lane 1 the value
                    const uint64_t own = record - g.first_ray * a.nreflections;      // the record's number within the pair
                    if (h == 0) {
                        uint32_t key = d.ntriangles;
                        if (SideRecord::surface(sd) != NONE) key = min(ListenRecord::load(d.listen, record).triangle(), d.ntriangles);
                        d.keys[own] = key;
                    } else {
                        d.values[own] = (uint32_t) own;
                    }
                }
            }
            __syncthreads();
            // (2) the weight gather, sum_c w[c][b][bin_k] * gain_c(k) of this lane's band for the tile's records: channel by channel with
            // the tile's TILE gathers of a channel in flight together (inside the chain below every gather would be waited for alone).
            // A record that adds nothing reads bin 0 and its sum is not used.
#pragma unroll 1
            for (uint32_t k0 = 0; k0 < GRAD_TILE; k0 += GRAD_GATHER) {
                float wsum[GRAD_GATHER];
#pragma unroll
                for (uint32_t k = 0; k < GRAD_GATHER; ++k) wsum[k] = 0.0f;
                for (uint32_t c = 0; c < nch; ++c) {
#pragma unroll
                    for (uint32_t k = 0; k < GRAD_GATHER; ++k) {
                        const uint32_t bin = side_words[(GradRows::at(r, k0) + k) * 4u + GRAD_BIN_WORD];       // (k added last: a constant offset of the read)
                        const float4 t4 = toward[GradRows::at(r, k0) + k];
                        const float w = g.weights[(uint64_t) (bin != NONE ? bin : 0u) * cb + c * 8u + band];
                        wsum[k] += w * speaker_gain_toward(d.m, c, mk3(t4.x, t4.y, t4.z));
                    }
                }
#pragma unroll
                for (uint32_t k = 0; k < GRAD_GATHER; ++k) us[(k0 + k) * WAVE + lane] = wsum[k];
            }
            // (3) forward along the ray, one band per lane
            float vol = starts[t * WAVE + lane];
            for (uint32_t k = 0; k < GRAD_TILE; ++k) {
                const float4 sd = side[GradRows::at(r, k)];
                const uint32_t surface = SideRecord::surface(sd), bin = __float_as_uint(sd.w);
                const float dist = SideRecord::new_dist(sd), diff = SideRecord::diff(sd);
                const float prev = vol;
                float dc = 0.0f, ak = 0.0f;
                if (surface != NONE) {
                    vol = chain_step<SURF_LDS>(a, surf_lds, vol, surface, band);
                    dc = diffuse_band<SURF_LDS>(a, surf_lds, surface, band);
                    if (bin != NONE) ak = ((air_attenuation(dist, air) * diff) * pattern_gain) * us[k * WAVE + lane];
                }
                const float u = ak * dc;
                if (!MAP) air_sum += (double) ((vol * u) * dist);
                us[k * WAVE + lane] = u;
                prevs[k * WAVE + lane] = prev;
                put_term<MAP>(table, rows, d, lane, k, surface, 8u + band, vol * ak);
            }
            // (4) backward
            for (uint32_t k = GRAD_TILE; k-- > 0;) {
                const uint32_t surface = side_words[GradRows::surface_word(r, k)];
                float gs = 0.0f;
                if (surface != NONE) {
                    const float b = us[k * WAVE + lane] + carry;
                    gs = -prevs[k * WAVE + lane] * b;
                    carry = -specular_band<SURF_LDS>(a, surf_lds, surface, band) * b;
                } else {
                    carry = 0.0f;
                }
                put_term<MAP>(table, rows, d, lane, k, surface, band, gs);
            }
            if (MAP) {
                // the tile's rows out: ray rr's run of the tile is contiguous in memory, four lanes per 64-byte row; no row for a slot
                // without a record (nothing reads it)
                __syncthreads();
                const uint32_t k = lane >> 2, q = lane & 3u;
                for (uint32_t rr = 0; rr < GradRows::RAYS; ++rr) {
                    if (ray0 + rr >= g.nrays || first + k >= a.nreflections || side_words[GradRows::surface_word(rr, k)] == NONE) continue;
                    const float4 v = *reinterpret_cast<const float4 *>(rows + rr * GRAD_TERM_RAY_WORDS + k * 16u + q * 4u);
                    store_stream(d.terms + ((uint64_t) (ray0 + rr) * a.nreflections + first + k) * 4u + q, v);
                }
            }
        }
    }
    if (MAP) return;
    // the air derivative of a band: the wave's rays in ray order
    double air_total = 0.0;
#pragma unroll
    for (uint32_t o = 0; o < GradRows::RAYS; ++o) air_total += __shfl(air_sum, (int) (o * 8u + band));
    const double ln_e = 0x1.fffffefb245eap-1;                                // ln((float) M_E), rvb_math.h air_attenuation
    if (r == 0) table[d.window * 16u + band] = air_total * ln_e;
    __syncthreads();
    double * out = d.partials + (size_t) blockIdx.x * d.entries;
    for (uint32_t i = lane; i < d.window * 16u; i += WAVE) out[(size_t) d.surface0 * 16u + i] = table[i];
    if (d.surface0 == 0 && lane < 8u) out[d.entries - 8u + lane] = table[d.window * 16u + lane];
}

// [channel * 8 + band][nbins] -> [bin][channel * 8 + band], 64-bin tiles through LDS: reads in 256-byte runs, one contiguous span out
__global__ __launch_bounds__(256) void reshade_grad_weights_kernel(const float * __restrict__ in, float * __restrict__ out, const uint32_t cb, const uint64_t nbins)
{
    __shared__ float tile[64][GRAD_TR_BINS + 1];
    const uint64_t ntiles = (nbins + GRAD_TR_BINS - 1) / GRAD_TR_BINS;
    for (uint64_t t = blockIdx.x; t < ntiles; t += gridDim.x) {
        const uint64_t bin0 = t * GRAD_TR_BINS;
        const uint32_t width = (uint32_t) min((uint64_t) GRAD_TR_BINS, nbins - bin0);
        for (uint32_t i = threadIdx.x; i < cb * GRAD_TR_BINS; i += 256) {
            const uint32_t row = i / GRAD_TR_BINS, col = i % GRAD_TR_BINS;
            if (col < width) tile[row][col] = in[(uint64_t) row * nbins + bin0 + col];
        }
        __syncthreads();
        for (uint32_t i = threadIdx.x; i < width * cb; i += 256)
            out[bin0 * cb + i] = tile[i % cb][i / cb];
        __syncthreads();
    }
}

// entry e of the result: the workgroups' partial sums, thread t those of tables t, t + 256, ... in order, then a fixed tree
__global__ __launch_bounds__(256) void reshade_grad_reduce_kernel(const double * __restrict__ partials, const uint32_t blocks, const uint32_t entries,
                                                                  float * __restrict__ out)
{
    __shared__ double part[256];
    const uint32_t e = blockIdx.x;
    double sum = 0.0;
    for (uint32_t b = threadIdx.x; b < blocks; b += 256) sum += partials[(size_t) b * entries + e];
    part[threadIdx.x] = sum;
    __syncthreads();
    for (uint32_t off = 128; off > 0; off >>= 1) {
        if (threadIdx.x < off) part[threadIdx.x] += part[threadIdx.x + off];
        __syncthreads();
    }
    if (threadIdx.x == 0) out[e] = (float) part[0];
}

}  // namespace

uint32_t rvb_reshade_grad_blocks(uint64_t nrays, uint64_t nsurfaces)
{
    const uint64_t groups = GradRows::groups(nrays);
    const uint64_t fit = GRAD_PARTIAL_BYTES / ((nsurfaces * 16 + 8) * sizeof(double));
    return (uint32_t) std::max<uint64_t>(std::min<uint64_t>(groups, std::min<uint64_t>(std::max<uint64_t>(fit, 64), GRAD_MAX_BLOCKS)), 1);
}

void rvb_launch_reshade_grad_weights(const float * weights, float * transposed, uint32_t nchannels, uint64_t nbins, hipStream_t s)
{
    hipLaunchKernelGGL(reshade_grad_weights_kernel, dim3(stream_blocks((nbins + GRAD_TR_BINS - 1) / GRAD_TR_BINS * 256, 256)), dim3(256), 0, s,
                       weights, transposed, nchannels * 8u, nbins);
}

void rvb_launch_reshade_grad(const TraceArgs & a, const float4 * kept, const AttenuationModel & model, const ReshadeGradArgs & g, double * partials,
                             uint32_t blocks, hipStream_t s)
{
    GradDev d;
    d.m = make_model(model);
    d.g = g;
    d.ngroups = (uint32_t) GradRows::groups(g.nrays);
    d.ntiles = std::max((a.nreflections + GRAD_TILE - 1) / GRAD_TILE, 1u);
    d.entries = (uint32_t) (g.nsurfaces * 16 + 8);
    d.partials = partials;
    // (a pair without rays or bounces still leaves its zero tables: ngroups == 0 skips the sweep inside the kernel)
    for (uint64_t s0 = 0; s0 < std::max<uint64_t>(g.nsurfaces, 1); s0 += GRAD_WINDOW) {
        d.surface0 = (uint32_t) s0;
        d.window = (uint32_t) std::min<uint64_t>(GRAD_WINDOW, g.nsurfaces - std::min(s0, g.nsurfaces));
        const size_t lds = ((size_t) grad_surfaces_at(d.window, d.ntiles) + 16u * a.lds_surfaces) * sizeof(uint32_t);
        hipLaunchKernelGGL((a.lds_surfaces ? reshade_grad_kernel<true, false> : reshade_grad_kernel<false, false>), dim3(blocks), dim3(WAVE), lds, s, a, d, kept);
    }
}

void rvb_launch_reshade_grad_map_terms(const TraceArgs & a, const float4 * kept, const uint2 * listen, const AttenuationModel & model, const ReshadeGradArgs & g,
                                       uint32_t ntriangles, float * terms, uint32_t * keys, uint32_t * values, hipStream_t s)
{
    GradDev d = {};
    d.m = make_model(model);
    d.g = g;
    d.ngroups = (uint32_t) GradRows::groups(g.nrays);
    d.ntiles = std::max((a.nreflections + GRAD_TILE - 1) / GRAD_TILE, 1u);
    d.terms = reinterpret_cast<float4 *>(terms);
    d.keys = keys;
    d.values = values;
    d.listen = listen;
    d.ntriangles = ntriangles;
    if (d.ngroups == 0) return;
    const uint32_t blocks = std::min(d.ngroups, GRAD_MAX_BLOCKS);
    const size_t lds = ((size_t) grad_surfaces_at(0u, d.ntiles, true) + 16u * a.lds_surfaces) * sizeof(uint32_t);
    hipLaunchKernelGGL((a.lds_surfaces ? reshade_grad_kernel<true, true> : reshade_grad_kernel<false, true>), dim3(blocks), dim3(WAVE), lds, s, a, d, kept);
}

void rvb_launch_reshade_grad_reduce(const double * partials, uint32_t blocks, uint64_t nsurfaces, float * out, hipStream_t s)
{
    const uint32_t entries = (uint32_t) (nsurfaces * 16 + 8);
    hipLaunchKernelGGL(reshade_grad_reduce_kernel, dim3(entries), dim3(256), 0, s, partials, blocks, entries, out);
}
