// speech_kernels.hip — the modulation transfer function of rows of bins and its adjoint on the device (rvb_mtf / rvb_mtf_adjoint of
// include/rvb_capi_speech.h), in the tile shape of the decay kernels (decay_tiles.h): rows along gridDim.y, tiles of 4096 bins along x,
// 256 lanes with four chunks of four consecutive bins each.
//   mtf_sums_kernel     per tile the binary64 sums of e, e cos and e sin for every frequency, e = H^2          grid (tiles, rows)
//   mtf_fold_kernel     ONE WAVE per row adds the row's tiles in tile order: S, A_i, B_i, m_i, the adjoint's row block   grid (1, rows)
//   mtf_adjoint_kernel  the tile again: dL/dH of every bin from the row block, rounded to float once          grid (tiles, rows)
// THE ORDER of every sum is that of decay_tiles.h — per lane the bins of a chunk one after the other, chunks across a wave by the scan's
// ladder, the 16 (i, wave) segments of a tile one after the other, tiles by row_sum — never by which workgroup ran first: no atomics.
//
// THE PHASE.  For the first bin j of a chunk, u = j q in one binary64 product and sincospi(2 u): the library reduces the argument of
// a sine of pi x exactly.  The chunk's other three bins follow by rotations with the constant step (cos, sin)(2 pi q), four products and
// two sums each: a quarter of the library calls of the per-bin form, and every value within 2^-48 of the one at its exact phase.
// THE REGISTERS.  The frequencies are the outer loop: a lane holds its 16 squares and, per frequency, eight chunk sums which go through
// the ladder into LDS before the next frequency starts; no lane ever holds 33 accumulators, and the bytes do not depend on nfreqs.
#include "decay_tiles.h"
#include "speech_kernels.h"

#include <math.h>

namespace {

constexpr uint32_t kMaxSums = 1 + 2 * RVB_MTF_MAX_FREQS;

__device__ inline double square(float h) { const double d = (double) h; return d * d; }

// cos and sin of 2 pi j q at the chunk's first bin j
__device__ inline void phase_of(double bin, double q, double & c, double & s)
{
    const double u = bin * q;
    sincospi(2.0 * u, &s, &c);
}

// one bin further
__device__ inline void rotate(double & c, double & s, double step_cos, double step_sin)
{
    const double nc = c * step_cos - s * step_sin;
    const double ns = s * step_cos + c * step_sin;
    c = nc;
    s = ns;
}

// the four chunk values of this lane through the ladder: the (i, wave) segments' sums into totals[0 .. kSegments)
__device__ inline void segments_of(const double (&v)[kChunks], double * totals)
{
    const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
#pragma unroll
    for (uint32_t i = 0; i < kChunks; ++i) {
        const double incl = wave_scan<false>(v[i]);
        if (lane == 63u) totals[i * (kLanes / 64) + wave] = incl;
    }
}

__global__ __launch_bounds__(kLanes) void mtf_sums_kernel(const float * __restrict__ hist, uint64_t nbins, uint32_t ntiles, uint32_t nrows,
                                                          const MtfFreqs f, double * __restrict__ tiles)
{
    __shared__ double totals[kMaxSums][kSegments];
    const uint32_t tile = blockIdx.x, r = blockIdx.y;
    const float * row = hist + (size_t) r * nbins;
    double e[kChunks][4], bin[kChunks], v[kChunks];
#pragma unroll
    for (uint32_t i = 0; i < kChunks; ++i) {
        const uint64_t first = chunk_bin(tile, i);
        const float4 h = load4(row, first, nbins);
        e[i][0] = square(h.x); e[i][1] = square(h.y); e[i][2] = square(h.z); e[i][3] = square(h.w);
        bin[i] = (double) first;
        v[i] = ((e[i][0] + e[i][1]) + e[i][2]) + e[i][3];
    }
    segments_of(v, totals[0]);
    for (uint32_t k = 0; k < f.n; ++k) {
        const double q = f.q[k], step_cos = f.step_cos[k], step_sin = f.step_sin[k];
        double a[kChunks], b[kChunks];
#pragma unroll
        for (uint32_t i = 0; i < kChunks; ++i) {
            double c, s;
            phase_of(bin[i], q, c, s);
            a[i] = e[i][0] * c;
            b[i] = e[i][0] * s;
#pragma unroll
            for (uint32_t j = 1; j < 4; ++j) {
                rotate(c, s, step_cos, step_sin);
                a[i] = a[i] + e[i][j] * c;
                b[i] = b[i] + e[i][j] * s;
            }
        }
        segments_of(a, totals[1 + 2 * k]);
        segments_of(b, totals[2 + 2 * k]);
    }
    __syncthreads();
    if (threadIdx.x < 1 + 2 * f.n) {
        double total = 0.0;
        for (uint32_t s = 0; s < kSegments; ++s) total = total + totals[threadIdx.x][s];
        tiles[((size_t) threadIdx.x * nrows + r) * ntiles + tile] = total;
    }
}

__global__ __launch_bounds__(64) void mtf_fold_kernel(const double * __restrict__ tiles, uint32_t ntiles, uint32_t nrows, uint32_t nfreqs,
                                                      const double * __restrict__ coeffs, MtfRow * __restrict__ rows)
{
    const uint32_t r = blockIdx.y;
    MtfRow * out = rows + r;
    const double sum = row_sum(tiles + (size_t) r * ntiles, ntiles);
    if (threadIdx.x == 0) out->sums[0] = sum;
    double weighted = 0.0;                                       // sum_i c_i m_i
    for (uint32_t i = 0; i < nfreqs; ++i) {
        const double a = row_sum(tiles + ((size_t) (1 + 2 * i) * nrows + r) * ntiles, ntiles);
        const double b = row_sum(tiles + ((size_t) (2 + 2 * i) * nrows + r) * ntiles, ntiles);
        const double modulus = sqrt(a * a + b * b);
        const double m = modulus / sum;                           // 0 / 0: the quiet NaN of an empty row
        if (threadIdx.x == 0) {
            out->sums[1 + 2 * i] = a;
            out->sums[2 + 2 * i] = b;
            out->m[i] = m;
        }
        if (coeffs) {
            const double c = coeffs[(size_t) r * RVB_MTF_MAX_FREQS + i];
            const bool none = sum == 0.0 || modulus == 0.0;
            const double scale = none ? 0.0 : c / (modulus * sum);
            if (threadIdx.x == 0) {
                out->a[i] = none ? 0.0 : scale * a;
                out->b[i] = none ? 0.0 : scale * b;
            }
            if (!none) weighted = weighted + c * m;
        }
    }
    if (coeffs && threadIdx.x == 0) out->d = sum == 0.0 ? 0.0 : weighted / sum;
}

__global__ __launch_bounds__(kLanes) void mtf_adjoint_kernel(const float * __restrict__ hist, uint64_t nbins, const MtfFreqs f,
                                                             const MtfRow * __restrict__ rows, float * __restrict__ weights)
{
    const uint32_t tile = blockIdx.x, r = blockIdx.y;
    const float * row = hist + (size_t) r * nbins;
    const MtfRow * coefficients = rows + r;
    const double d = coefficients->d;
#pragma unroll 1
    for (uint32_t i = 0; i < kChunks; ++i) {
        const uint64_t first = chunk_bin(tile, i);
        if (first >= nbins) continue;
        const float4 h4 = load4(row, first, nbins);
        const float h[4] = {h4.x, h4.y, h4.z, h4.w};
        double g[4] = {0.0, 0.0, 0.0, 0.0};
        for (uint32_t k = 0; k < f.n; ++k) {
            const double a = coefficients->a[k], b = coefficients->b[k];
            double c, s;
            phase_of((double) first, f.q[k], c, s);
#pragma unroll
            for (uint32_t j = 0; j < 4; ++j) {
                if (j) rotate(c, s, f.step_cos[k], f.step_sin[k]);
                g[j] = g[j] + (a * c + b * s);
            }
        }
        float o[4];
#pragma unroll
        for (uint32_t j = 0; j < 4; ++j) o[j] = h[j] == 0.0f ? 0.0f : (float) (2.0 * (double) h[j] * (g[j] - d));
        store4(weights + (size_t) r * nbins, first, nbins, make_float4(o[0], o[1], o[2], o[3]));
    }
}

} // namespace

void rvb_launch_mtf_sums(const float * hist, uint64_t nrows, uint64_t nbins, const MtfFreqs & freqs, double * tiles, hipStream_t s)
{
    const uint32_t ntiles = rvb_decay_tiles(nbins);
    mtf_sums_kernel<<<dim3(ntiles, (uint32_t) nrows), kLanes, 0, s>>>(hist, nbins, ntiles, (uint32_t) nrows, freqs, tiles);
}

void rvb_launch_mtf_fold(uint64_t nrows, uint64_t nbins, uint32_t nfreqs, const double * tiles, const double * coeffs, MtfRow * rows, hipStream_t s)
{
    mtf_fold_kernel<<<dim3(1, (uint32_t) nrows), 64, 0, s>>>(tiles, rvb_decay_tiles(nbins), (uint32_t) nrows, nfreqs, coeffs, rows);
}

void rvb_launch_mtf_adjoint(const float * hist, uint64_t nrows, uint64_t nbins, const MtfFreqs & freqs, const MtfRow * rows, float * weights,
                            hipStream_t s)
{
    const uint32_t ntiles = rvb_decay_tiles(nbins);
    mtf_adjoint_kernel<<<dim3(ntiles, (uint32_t) nrows), kLanes, 0, s>>>(hist, nbins, freqs, rows, weights);
}
