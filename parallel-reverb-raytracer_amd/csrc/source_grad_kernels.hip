// source_grad_kernels.hip — source-end gradients of a weighted impulse response from a kept trace (include/rvb_capi_source_grad.h):
// dL/dg_b(r), the derivative of L = sum w * H with respect to the source gain of ray r in band b, the same per image source, and from
// them the derivatives with respect to the polar pattern (direction, shapes) that the records reflect.  No reference counterpart.  H is
// linear in the gain of every ray — volume_b(k) = P_k * air_attenuation(dist_k, air_b) * diffuse[s_k][b] * DIFF(k) * g_b(r) along ray r
// (reshade_grad_kernels.hip) —, so the derivative is the sum of the ray's terms with the gain left out: no stored (already scaled) volume
// is read and nothing is divided by a gain; a ray at a null of the pattern has its derivative like any other.
//   source_grad_rays_kernel           the forward sweep of reshade_grad_kernel (grad_tiles.h over kept_tiles.h): a wave takes eight rays,
//                                     lane (ray, band) owns a chain; tile by tile of GRAD_TILE bounces the records two lanes per record
//                                     into LDS, the lane's weight gathers, then the chain forward: the binary32 term
//                                     t_k = (P_k * ((air_attenuation(dist_k, air_b) * DIFF(k)) * u_k)) * diffuse[s_k][b] added in bounce
//                                     order in binary64.  No table in LDS, no backward sweep, no checkpoints: P runs on in a register.
//                                     Every (ray, band) is written — the sum rounded once, and the binary64 sum itself for the pattern
//                                     kernel —; lane (ray, 0) also selects the ray's row of a source table (departure_row of attenuation.h).
//   source_grad_images_kernel         one lane per image of the merged list, band by band: reshade_grad_images_kernel's weight gather, air
//                                     product and chain product in its order, the gain gamma_b(i) left out; the departure vector
//                                     mic - position, its unit form and its table row beside it.
//   source_grad_pattern_kernel        per ray (or image) u = normalize3(normalize3(v)), d = dot3(u, n) in binary32 as band_gain takes
//                                     them, then in binary64 Lambda_b (d - 1) for the eight shapes and (sum_b shape_b Lambda_b) u_j for the
//                                     direction: a tile of 256 items per workgroup, a fixed tree, one partial of 11 sums per tile.
//   source_grad_pattern_fold_kernel   the tiles' partials, thread t those of tiles t, t + 256, ... in order, then a fixed tree; rounded to
//                                     binary32 once.  No atomics anywhere: two calls return identical bytes.
#include "grad_tiles.h"

namespace {

#define SOURCE_GRAD_MAX_BLOCKS 16384u    // as reshade_grad_kernel's: every wave then takes a few groups of rays at 100 k rays
#define SOURCE_GRAD_SUMS 11u             // shape[8], direction[3]

// LDS of a wave, in words: a GradRows region of staged records twice (float4 each), [TILE][WAVE] floats (u_k), the surface table
#define SOURCE_GRAD_SURFACES_AT (2u * GRAD_STAGE_WORDS + GRAD_TILE * WAVE)

template <bool SURF_LDS>
__global__ __launch_bounds__(WAVE) void source_grad_rays_kernel(TraceArgs a, ModelDev m, ReshadeGradArgs g, SourceGradOut o, const uint32_t ngroups,
                                                                const uint32_t ntiles, const float4 * __restrict__ kept)
{
    extern __shared__ __attribute__((aligned(16))) uint32_t lds[];
    uint32_t * side_words = lds;
    float4 * side = reinterpret_cast<float4 *>(side_words);                  // staged records (GRAD_BIN_WORD)
    float4 * toward = side + GradRows::RECORDS;                              // the record's arrival direction at the microphone
    float * us = reinterpret_cast<float *>(toward + GradRows::RECORDS);      // u_k
    const lds_float4_ptr surf_lds = stage_surfaces(a, lds + SOURCE_GRAD_SURFACES_AT);
    const uint32_t lane = threadIdx.x, r = lane >> 3, band = lane & 7u;
    const float air = a.air[band];
    const v3 mic = mk3(g.mic[0], g.mic[1], g.mic[2]);
    for (uint32_t grp = blockIdx.x; grp < ngroups; grp += gridDim.x) {
        const uint32_t ray0 = grp * GradRows::RAYS;                          // within the pair
        const bool mine = ray0 + r < g.nrays;
        double lambda = 0.0;
        float vol = 1.0f;
        bool alive = true;
        for (uint32_t t = 0; t < ntiles; ++t) {
            __syncthreads();                                                 // (what the wave read of the tile before)
            stage_grad_records(a, m, g, kept, ray0, t * GRAD_TILE, mic, side, toward);
            __syncthreads();
            gather_tile_weights(m, g, side_words, toward, us);
            // forward along the ray, one band per lane; an escape (or the end of the ray) ends the chain
            for (uint32_t k = 0; k < GRAD_TILE && alive; ++k) {
                const float4 sd = side[GradRows::at(r, k)];
                const uint32_t surface = SideRecord::surface(sd), bin = __float_as_uint(sd.w);
                if (surface == NONE) {
                    alive = false;
                    break;
                }
                vol = chain_step<SURF_LDS>(a, surf_lds, vol, surface, band);
                if (bin == NONE) continue;                                   // invisible, or past the histogram: adds nothing
                const float dc = diffuse_band<SURF_LDS>(a, surf_lds, surface, band);
                const float ak = (air_attenuation(SideRecord::new_dist(sd), air) * SideRecord::diff(sd)) * us[k * WAVE + lane];
                lambda += (double) ((vol * ak) * dc);
            }
        }
        if (mine) {
            const size_t at = (size_t) (ray0 + r) * 8u + band;
            if (o.grad) o.grad[at] = (float) lambda;
            if (o.lambda) o.lambda[at] = lambda;
            if (o.rows && band == 0) {
                const float4 dv = a.directions[ray0 + r];
                o.rows[ray0 + r] = departure_row(o.table_basis[0], o.table_basis[1], o.table_basis[2], mk3(dv.x, dv.y, dv.z));
            }
        }
    }
}

#define IMAGE_GRAD_NONE 0xFFFFFFFFu

__global__ __launch_bounds__(64) void source_grad_images_kernel(TraceArgs a, ModelDev m, ImageGradArgs g, SourceGradOut o, float4 * __restrict__ departures,
                                                                float4 * __restrict__ units)
{
    const uint64_t i = (uint64_t) blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= g.n)
        return;
    const uint32_t w = g.winners[i];
    const rvb_impulse & image = g.images[i];
    const v3 pos = mk3(image.position[0], image.position[1], image.position[2]);
    uint32_t surface[RVB_IMAGE_GRAD_STEPS];
#pragma unroll
    for (uint32_t k = 0; k < RVB_IMAGE_GRAD_STEPS; ++k) surface[k] = IMAGE_GRAD_NONE;
    uint32_t nsteps = 0;
    float dist;
    if (w == RVB_IMAGE_WINNER_DIRECT) {
        dist = a.image_dist[g.direct_dist];                       // an empty chain
    } else {
        // reshade_images_kernel's chain: the surfaces of the ray's bounces 0 .. slot - 2
        const rvb_image_candidate & cand = a.candidates[w];
        const uint32_t * early = a.early + (cand.ray - a.ray_offset) * (RVB_NUM_IMAGE_SOURCE - 1);
        nsteps = cand.slot > 0 ? min(cand.slot - 1u, RVB_IMAGE_GRAD_STEPS) : 0u;
#pragma unroll
        for (uint32_t k = 0; k < RVB_IMAGE_GRAD_STEPS; ++k)
            if (k < nsteps) surface[k] = a.scene.shade[early[k]].surface;
        dist = a.image_dist[w];
    }
    const uint32_t bin = time_bin(image.time, g.predelay, g.sample_rate);
    const bool live = !(dist < 0.0f) && bin < g.nbins;           // a hidden direct path (negative distance) adds nothing
    const v3 toward = arrival_direction(m, pos);
    // the departure vector of the image: v = mic - position, as source_pattern_images_kernel / source_table_images_kernel take it
    const v3 v = mk3(g.mic[0], g.mic[1], g.mic[2]) - pos;
    departures[i] = make_float4(v.x, v.y, v.z, 0.0f);
    if (units) {
        const v3 u = normalize3(normalize3(v));
        units[i] = make_float4(u.x, u.y, u.z, 0.0f);
    }
    if (o.rows) o.rows[i] = departure_row(o.table_basis[0], o.table_basis[1], o.table_basis[2], v);
#pragma unroll 1
    for (uint32_t b = 0; b < 8; ++b) {
        float term = 0.0f;
        if (live) {
            float gathered = 0.0f;
            for (uint32_t c = 0; c < m.nchannels; ++c)
                gathered += g.weights[((uint64_t) c * 8u + b) * g.nbins + bin] * speaker_gain_toward(m, c, toward);
            const float alpha = (air_attenuation(dist, a.air[b]) * 1.0f) * gathered;
            // prod_j -specular[s_j][b], in the order of kernel.cpp:461
            float prefix = 1.0f;
#pragma unroll
            for (uint32_t k = 0; k < RVB_IMAGE_GRAD_STEPS; ++k)
                if (k < nsteps) prefix = -prefix * a.scene.surfaces[surface[k]].specular[b];
            term = prefix * alpha;
        }
        if (o.grad) o.grad[i * 8u + b] = term;
        if (o.lambda) o.lambda[i * 8u + b] = (double) term;
    }
}

// item i of a tile: v its departure vector (the ray's own direction, or mic - position of an image), lambda its eight binary64 sums
__global__ __launch_bounds__(256) void source_grad_pattern_kernel(const float4 * __restrict__ vectors, const double * __restrict__ lambda, const uint64_t n,
                                                                  const SourcePatternDev pattern, double * __restrict__ partials)
{
    __shared__ double part[SOURCE_GRAD_SUMS][256];
    const uint32_t t = threadIdx.x;
    const uint64_t i = (uint64_t) blockIdx.x * 256u + t;
    double sums[SOURCE_GRAD_SUMS];
#pragma unroll
    for (uint32_t e = 0; e < SOURCE_GRAD_SUMS; ++e) sums[e] = 0.0;
    if (i < n) {
        const float4 dv = vectors[i];
        const v3 u = normalize3(normalize3(mk3(dv.x, dv.y, dv.z)));
        const float d = dot3(u, mk3(pattern.direction[0], pattern.direction[1], pattern.direction[2]));
        const double d1 = (double) d - 1.0;
        double along = 0.0;                                                  // sum_b shape_b Lambda_b
#pragma unroll
        for (uint32_t b = 0; b < 8; ++b) {
            const double l = lambda[i * 8u + b];
            sums[b] = l * d1;
            along += (double) pattern.shape[b] * l;
        }
        sums[8] = along * (double) u.x;
        sums[9] = along * (double) u.y;
        sums[10] = along * (double) u.z;
    }
#pragma unroll
    for (uint32_t e = 0; e < SOURCE_GRAD_SUMS; ++e) part[e][t] = sums[e];
    __syncthreads();
    for (uint32_t off = 128; off > 0; off >>= 1) {
        if (t < off) {
#pragma unroll
            for (uint32_t e = 0; e < SOURCE_GRAD_SUMS; ++e) part[e][t] += part[e][t + off];
        }
        __syncthreads();
    }
    if (t < SOURCE_GRAD_SUMS) partials[(size_t) blockIdx.x * SOURCE_GRAD_SUMS + t] = part[t][0];
}

// out: rvb_source_pattern_grad as twelve floats, shape[8] then direction[4] with direction[3] = 0
__global__ __launch_bounds__(256) void source_grad_pattern_fold_kernel(const double * __restrict__ partials, const uint32_t ntiles, float * __restrict__ out)
{
    __shared__ double part[SOURCE_GRAD_SUMS][256];
    const uint32_t t = threadIdx.x;
    double sums[SOURCE_GRAD_SUMS];
#pragma unroll
    for (uint32_t e = 0; e < SOURCE_GRAD_SUMS; ++e) sums[e] = 0.0;
    for (uint32_t tile = t; tile < ntiles; tile += 256) {
#pragma unroll
        for (uint32_t e = 0; e < SOURCE_GRAD_SUMS; ++e) sums[e] += partials[(size_t) tile * SOURCE_GRAD_SUMS + e];
    }
#pragma unroll
    for (uint32_t e = 0; e < SOURCE_GRAD_SUMS; ++e) part[e][t] = sums[e];
    __syncthreads();
    for (uint32_t off = 128; off > 0; off >>= 1) {
        if (t < off) {
#pragma unroll
            for (uint32_t e = 0; e < SOURCE_GRAD_SUMS; ++e) part[e][t] += part[e][t + off];
        }
        __syncthreads();
    }
    if (t < 12u) out[t] = t < SOURCE_GRAD_SUMS ? (float) part[t][0] : 0.0f;
}

}  // namespace

void rvb_launch_source_grad_rays(const TraceArgs & a, const float4 * kept, const AttenuationModel & model, const ReshadeGradArgs & g, const SourceGradOut & o,
                                 hipStream_t s)
{
    const uint32_t ngroups = (uint32_t) GradRows::groups(g.nrays);
    if (ngroups == 0) return;
    const uint32_t ntiles = std::max((a.nreflections + GRAD_TILE - 1) / GRAD_TILE, 1u);
    const uint32_t blocks = std::min(ngroups, SOURCE_GRAD_MAX_BLOCKS);
    const size_t lds = ((size_t) SOURCE_GRAD_SURFACES_AT + 16u * a.lds_surfaces) * sizeof(uint32_t);
    hipLaunchKernelGGL((a.lds_surfaces ? source_grad_rays_kernel<true> : source_grad_rays_kernel<false>), dim3(blocks), dim3(WAVE), lds, s, a, make_model(model),
                       g, o, ngroups, ntiles, kept);
}

void rvb_launch_source_grad_images(const TraceArgs & a, const AttenuationModel & model, const ImageGradArgs & g, const SourceGradOut & o, float4 * departures,
                                   float4 * units, hipStream_t s)
{
    if (g.n == 0) return;
    hipLaunchKernelGGL(source_grad_images_kernel, dim3(stream_blocks(g.n, 64)), dim3(64), 0, s, a, make_model(model), g, o, departures, units);
}

void rvb_launch_source_grad_pattern(const float4 * vectors, const double * lambda, uint64_t n, const SourcePatternDev & pattern, double * partials, hipStream_t s)
{
    if (n == 0) return;
    hipLaunchKernelGGL(source_grad_pattern_kernel, dim3((unsigned) rvb_source_grad_tiles(n)), dim3(256), 0, s, vectors, lambda, n, pattern, partials);
}

void rvb_launch_source_grad_pattern_fold(const double * partials, uint64_t n, float * out, hipStream_t s)
{
    hipLaunchKernelGGL(source_grad_pattern_fold_kernel, dim3(1), dim3(256), 0, s, partials, (uint32_t) rvb_source_grad_tiles(n), out);
}
