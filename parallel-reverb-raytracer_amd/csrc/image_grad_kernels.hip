// image_grad_kernels.hip — the image sources of a kept trace on the device (include/rvb_capi_images.h): the merged list without the
// host, and its part of the material gradient.  No reference counterpart for the stages; the merge rule is the host's
// (merge_image_winners, trace.hip) and the arithmetic is reshade_images_kernel's (reshade_kernels.hip): the chain of kernel.cpp:461 over
// the ray's first bounces, then make_image's product with the kept INIT_DIST (kernel.cpp:260).
//   image_gather_kernel                 one lane per output impulse: the 64 bytes of the winning candidate's impulse, or of the pair's
//                                       direct slot, as four whole 16-byte chunks into the image list.
//   reshade_grad_images_kernel          one lane per image, band by band: the weight gather sum_c w[c][b][bin] gain_c, the source gain, the
//                                       air product; the chain's prefix products forward, the suffix product backward, a term per chain
//                                       step — never a division —, and the air term.  It stores a row of RVB_IMAGE_GRAD_ROW words per
//                                       image: the steps' surfaces, their terms, the air terms.  A dead image (a hidden direct path, a bin
//                                       past the histogram) stores a row without steps.
//   reshade_grad_images_reduce_kernel   a workgroup per surface and one for the air: thread t adds the rows t, t + 256, ... in list order
//                                       and chain order in binary64, then a fixed tree; one rounding.  Every workgroup reads all rows
//                                       (320 bytes each): a few hundred to a few thousand rows and a few surfaces are latency-bound, the
//                                       two launches of the gradient; a scene of very many surfaces has not been measured.
#include "attenuation.h"

#include <cstddef>

namespace {

static_assert(sizeof(rvb_image_candidate) == 80 && offsetof(rvb_image_candidate, impulse) == 16 && sizeof(rvb_impulse) == 64,
              "a candidate's impulse is four aligned 16-byte chunks");

__global__ __launch_bounds__(256) void image_gather_kernel(const rvb_image_candidate * __restrict__ candidates, const rvb_impulse * __restrict__ direct,
                                                           const uint32_t * __restrict__ winners, const uint64_t n, rvb_impulse * __restrict__ images)
{
    const uint64_t i = (uint64_t) blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n)
        return;
    const uint32_t w = winners[i];
    const float4 * from = reinterpret_cast<const float4 *>(w == RVB_IMAGE_WINNER_DIRECT ? direct : &candidates[w].impulse);
    float4 * to = reinterpret_cast<float4 *>(images + i);
    const float4 c0 = from[0], c1 = from[1], c2 = from[2], c3 = from[3];
    to[0] = c0; to[1] = c1; to[2] = c2; to[3] = c3;
}

#define IMAGE_GRAD_NONE 0xFFFFFFFFu

__global__ __launch_bounds__(64) void reshade_grad_images_kernel(TraceArgs a, ModelDev m, ImageGradArgs g, uint32_t * __restrict__ rows)
{
    const uint64_t i = (uint64_t) blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= g.n)
        return;
    uint32_t * row = rows + i * RVB_IMAGE_GRAD_ROW;
    float * terms = reinterpret_cast<float *>(row) + RVB_IMAGE_GRAD_STEPS;
    const uint32_t w = g.winners[i];
    const rvb_impulse & image = g.images[i];
    const v3 pos = mk3(image.position[0], image.position[1], image.position[2]);
    uint32_t surface[RVB_IMAGE_GRAD_STEPS];
#pragma unroll
    for (uint32_t k = 0; k < RVB_IMAGE_GRAD_STEPS; ++k) surface[k] = IMAGE_GRAD_NONE;
    uint32_t nsteps = 0;
    float dist;
    if (w == RVB_IMAGE_WINNER_DIRECT) {
        dist = a.image_dist[g.direct_dist];                       // an empty chain: the direct path adds to the air alone
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
    if (!live) nsteps = 0;
#pragma unroll
    for (uint32_t k = 0; k < RVB_IMAGE_GRAD_STEPS; ++k) row[k] = k < nsteps ? surface[k] : IMAGE_GRAD_NONE;
    const v3 toward = arrival_direction(m, pos);
    // the source gain of the image: v = mic - position, as source_pattern_images_kernel / source_table_images_kernel take it
    const v3 v = mk3(g.mic[0], g.mic[1], g.mic[2]) - pos;
    float pattern_d = 0.0f;
    const float * table_row = nullptr;
    if (g.has_pattern) pattern_d = dot3(normalize3(normalize3(v)), mk3(g.pattern.direction[0], g.pattern.direction[1], g.pattern.direction[2]));
    if (g.table) table_row = g.table + 8 * (size_t) departure_row(g.table_basis[0], g.table_basis[1], g.table_basis[2], v);
#pragma unroll 1
    for (uint32_t b = 0; b < 8; ++b) {
        float alpha = 0.0f;
        if (live) {
            float gathered = 0.0f;
            for (uint32_t c = 0; c < m.nchannels; ++c)
                gathered += g.weights[((uint64_t) c * 8u + b) * g.nbins + bin] * speaker_gain_toward(m, c, toward);
            float gamma = 1.0f;
            if (table_row) gamma = table_row[b];
            else if (g.has_pattern) gamma = band_gain(g.pattern.shape[b], pattern_d);
            alpha = ((air_attenuation(dist, a.air[b]) * 1.0f) * gamma) * gathered;
        }
        // prefix[k] = prod_{j < k} -specular[s_j][b], in the order of kernel.cpp:461
        float specular[RVB_IMAGE_GRAD_STEPS], prefix[RVB_IMAGE_GRAD_STEPS + 1];
        prefix[0] = 1.0f;
#pragma unroll
        for (uint32_t k = 0; k < RVB_IMAGE_GRAD_STEPS; ++k) {
            specular[k] = k < nsteps ? a.scene.surfaces[surface[k]].specular[b] : -1.0f;      // (past the chain: a factor of one)
            prefix[k + 1] = -prefix[k] * specular[k];
        }
        // d/dspecular[s_k][b] = (-1) * alpha * prod_{j != k} -specular[s_j][b]: the prefix before the step, the suffix behind it
        float suffix = 1.0f;
#pragma unroll
        for (uint32_t k = RVB_IMAGE_GRAD_STEPS; k-- > 0;) {
            terms[k * 8u + b] = k < nsteps ? -(alpha * (prefix[k] * suffix)) : 0.0f;
            suffix = -suffix * specular[k];
        }
        terms[RVB_IMAGE_GRAD_STEPS * 8u + b] = live ? (prefix[RVB_IMAGE_GRAD_STEPS] * alpha) * dist : 0.0f;
    }
}

// block s < nsurfaces: surface s; block nsurfaces: the air
__global__ __launch_bounds__(256) void reshade_grad_images_reduce_kernel(const uint32_t * __restrict__ rows, const uint64_t n, const uint32_t nsurfaces,
                                                                         float * __restrict__ out)
{
    __shared__ double part[8][256];
    const uint32_t s = blockIdx.x, t = threadIdx.x;
    const bool air = s == nsurfaces;
    double sum[8] = {0, 0, 0, 0, 0, 0, 0, 0};
    for (uint64_t i = t; i < n; i += 256) {
        const uint32_t * row = rows + i * RVB_IMAGE_GRAD_ROW;
        const float * terms = reinterpret_cast<const float *>(row) + RVB_IMAGE_GRAD_STEPS;
        if (air) {
#pragma unroll
            for (uint32_t b = 0; b < 8; ++b) sum[b] += (double) terms[RVB_IMAGE_GRAD_STEPS * 8u + b];
            continue;
        }
        for (uint32_t k = 0; k < RVB_IMAGE_GRAD_STEPS; ++k) {
            if (row[k] != s) continue;
#pragma unroll
            for (uint32_t b = 0; b < 8; ++b) sum[b] += (double) terms[k * 8u + b];
        }
    }
#pragma unroll
    for (uint32_t b = 0; b < 8; ++b) part[b][t] = sum[b];
    __syncthreads();
    for (uint32_t off = 128; off > 0; off >>= 1) {
        if (t < off) {
#pragma unroll
            for (uint32_t b = 0; b < 8; ++b) part[b][t] += part[b][t + off];
        }
        __syncthreads();
    }
    const double ln_e = 0x1.fffffefb245eap-1;                                // ln((float) M_E), rvb_math.h air_attenuation
    if (air) {
        if (t < 8) out[(size_t) nsurfaces * 16u + t] = (float) (part[t][0] * ln_e);
    } else if (t < 16) {
        out[(size_t) s * 16u + t] = t < 8 ? (float) part[t][0] : 0.0f;      // images never read a diffuse coefficient
    }
}

}  // namespace

void rvb_launch_image_gather(const rvb_image_candidate * candidates, const rvb_impulse * direct, const uint32_t * winners, uint64_t n,
                             rvb_impulse * images, hipStream_t s)
{
    if (n == 0) return;
    hipLaunchKernelGGL(image_gather_kernel, dim3(stream_blocks(n, 256)), dim3(256), 0, s, candidates, direct, winners, n, images);
}

void rvb_launch_reshade_grad_images(const TraceArgs & a, const AttenuationModel & model, const ImageGradArgs & g, uint32_t * rows, hipStream_t s)
{
    if (g.n == 0) return;
    hipLaunchKernelGGL(reshade_grad_images_kernel, dim3(stream_blocks(g.n, 64)), dim3(64), 0, s, a, make_model(model), g, rows);
}

void rvb_launch_reshade_grad_images_reduce(const uint32_t * rows, uint64_t n, uint64_t nsurfaces, float * out, hipStream_t s)
{
    hipLaunchKernelGGL(reshade_grad_images_reduce_kernel, dim3((unsigned) nsurfaces + 1u), dim3(256), 0, s, rows, n, (uint32_t) nsurfaces, out);
}
