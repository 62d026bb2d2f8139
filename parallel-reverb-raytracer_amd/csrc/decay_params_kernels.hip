// decay_params_kernels.hip — the room acoustic parameters of a decay curve on the device (rvb_decay_params / rvb_decay_params_loss of
// include/rvb_capi.h): EDT, T20, T30, C50, C80, D50 and Ts of every row of E in ONE sweep, a weighted squared loss against a table of
// targets, and its adjoint w = dL/dH.  The tile shape, the order of every sum and the helpers are those of decay_kernels.hip
// (decay_tiles.h); the launches:
//   decay_params_find_kernel     five first-index values per tile: the thresholds of all three windows in one pass   grid (tiles, rows)
//   decay_params_window_kernel   ONE WAVE per row: the five bin numbers of the row                                    grid (1, rows)
//   decay_params_sums_kernel     per tile sum xc level of each window that meets it, and sum E                        grid (tiles, rows)
//   decay_params_fit_kernel      ONE WAVE per row: the seven parameters, the loss, the row's DecayParamsRow           grid (1, rows)
//   decay_params_adjoint_sums_kernel / _carry_kernel / _scan_kernel: sum g per tile, the tiles before each tile, the tile again on top
//   of its carry — g[k] = dL/dE[k] evaluated from E[k] and the DecayParamsRow, never stored.
// The three times are decay_times_* with three windows at once: the same thresholds, the same products in the same order, so that
// every time is the float rvb_decay_times returns.  A level is taken once per bin, whatever the number of windows that hold the bin.
#include "decay_tiles.h"

#include <math.h>

namespace {

constexpr uint32_t kNone = 0xFFFFFFFFu;
constexpr double kC10 = 4.342944819032518;               // 10 / ln 10
constexpr uint32_t kTimes = 3;                            // EDT, T20, T30
constexpr uint32_t kFirst = 5;                            // thresholds: <= 0 dB, < -10 dB, <= -5 dB, < -25 dB, < -35 dB

// the windows of a row from its five bin numbers: EDT [w0, w1), T20 [w2, w3), T30 [w2, w4)
__device__ inline void windows_of(const uint32_t * __restrict__ w, uint32_t (&k0)[kTimes], uint32_t (&k1)[kTimes])
{
    k0[0] = w[0]; k1[0] = w[1];
    k0[1] = w[2]; k1[1] = w[3];
    k0[2] = w[2]; k1[2] = w[4];
}

__global__ __launch_bounds__(kLanes) void decay_params_find_kernel(const float * __restrict__ curve, uint64_t nbins, uint32_t ntiles, uint32_t nrows,
                                                                    DecayParamsRatios ratios, uint32_t * __restrict__ first)
{
    __shared__ uint32_t found[kFirst][kLanes / 64];
    const uint32_t tile = blockIdx.x, r = blockIdx.y;
    const float * row = curve + (size_t) r * nbins;
    const double e0 = (double) row[0];
    double level[kFirst];
#pragma unroll
    for (uint32_t w = 0; w < kFirst; ++w) level[w] = e0 * ratios.r[w];
    uint32_t mine[kFirst] = {kNone, kNone, kNone, kNone, kNone};
#pragma unroll
    for (uint32_t i = 0; i < kChunks; ++i) {
        const uint64_t bin = chunk_bin(tile, i);
        const float4 v = load4(row, bin, nbins);
        const float e[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
        for (uint32_t j = 0; j < 4; ++j) {
            if (bin + j >= nbins) continue;
            const double x = (double) e[j];
            const uint32_t k = (uint32_t) (bin + j);
            if (x <= level[0]) mine[0] = min(mine[0], k);
            if (x < level[1]) mine[1] = min(mine[1], k);
            if (x <= level[2]) mine[2] = min(mine[2], k);
            if (x < level[3]) mine[3] = min(mine[3], k);
            if (x < level[4]) mine[4] = min(mine[4], k);
        }
    }
#pragma unroll
    for (uint32_t w = 0; w < kFirst; ++w) {
        for (uint32_t d = 32; d; d >>= 1) mine[w] = min(mine[w], (uint32_t) __shfl_xor((int) mine[w], (int) d, 64));
        if ((threadIdx.x & 63u) == 0) found[w][threadIdx.x >> 6] = mine[w];
    }
    __syncthreads();
    if (threadIdx.x < kFirst) {
        const uint32_t * f = found[threadIdx.x];
        first[((size_t) threadIdx.x * nrows + r) * ntiles + tile] = min(min(f[0], f[1]), min(f[2], f[3]));
    }
}

// window[row][0 .. 5): the first bin of the row for each threshold (0xFFFFFFFF: none)
__global__ __launch_bounds__(64) void decay_params_window_kernel(const uint32_t * __restrict__ first, uint32_t ntiles, uint32_t nrows, uint32_t * __restrict__ window)
{
    const uint32_t r = blockIdx.y;
    for (uint32_t w = 0; w < kFirst; ++w) {
        const uint32_t * f = first + ((size_t) w * nrows + r) * ntiles;
        uint32_t m = kNone;
        for (uint32_t t = threadIdx.x; t < ntiles; t += 64) m = min(m, f[t]);
        for (uint32_t d = 32; d; d >>= 1) m = min(m, (uint32_t) __shfl_xor((int) m, (int) d, 64));
        if (threadIdx.x == 0) window[(size_t) r * kFirst + w] = m;
    }
}

// per tile, planes 0..2: sum over its bins k in [k0, k1) of xc * level, level = 10 log10(E[k] / E[0]), xc = (k - k0) - (k1 - k0 - 1) / 2
// (0 where the window does not meet the tile); plane 3: sum of E[k] over its bins k >= 1
__global__ __launch_bounds__(kLanes) void decay_params_sums_kernel(const float * __restrict__ curve, uint64_t nbins, uint32_t ntiles, uint32_t nrows,
                                                                    const uint32_t * __restrict__ window, double * __restrict__ tiles)
{
    __shared__ double totals[kTimes + 1][kSegments];
    const uint32_t tile = blockIdx.x, r = blockIdx.y;
    const float * row = curve + (size_t) r * nbins;
    uint32_t k0[kTimes], k1[kTimes];
    windows_of(window + (size_t) r * kFirst, k0, k1);
    const uint64_t lo = (uint64_t) tile * kTile, hi = lo + kTile;
    bool meets[kTimes];                                                    // (uniform over the workgroup)
    double centre[kTimes];
#pragma unroll
    for (uint32_t p = 0; p < kTimes; ++p) {
        meets[p] = k1[p] != kNone && k0[p] != kNone && k0[p] < k1[p] && lo < k1[p] && hi > k0[p];
        centre[p] = 0.5 * (double) (k1[p] - k0[p] - 1u);
    }
    const double e0 = (double) row[0];
    double sum[kTimes][kChunks], energy[kChunks];
#pragma unroll
    for (uint32_t i = 0; i < kChunks; ++i) {
        const uint64_t bin = chunk_bin(tile, i);
        const float4 v = load4(row, bin, nbins);
        const float e[4] = {v.x, v.y, v.z, v.w};
        sum[0][i] = 0.0; sum[1][i] = 0.0; sum[2][i] = 0.0; energy[i] = 0.0;
#pragma unroll
        for (uint32_t j = 0; j < 4; ++j) {
            const uint64_t k = bin + j;
            if (k >= 1) energy[i] = energy[i] + (double) e[j];             // (behind the row's end e is 0)
            bool in[kTimes];
#pragma unroll
            for (uint32_t p = 0; p < kTimes; ++p) in[p] = meets[p] && k >= k0[p] && k < k1[p];
            if (!(in[0] || in[1] || in[2])) continue;
            const double level = 10.0 * log10((double) e[j] / e0);
#pragma unroll
            for (uint32_t p = 0; p < kTimes; ++p) {
                if (!in[p]) continue;
                const double xc = (double) (k - k0[p]) - centre[p];
                sum[p][i] = sum[p][i] + xc * level;
            }
        }
    }
    double total[kTimes + 1];
#pragma unroll
    for (uint32_t p = 0; p < kTimes; ++p) total[p] = meets[p] ? tile_sum(sum[p], totals[p]) : 0.0;
    total[kTimes] = tile_sum(energy, totals[kTimes]);
    if (threadIdx.x == 0) {
        const size_t at = (size_t) r * ntiles + tile, plane = (size_t) nrows * ntiles;
#pragma unroll
        for (uint32_t p = 0; p <= kTimes; ++p) tiles[p * plane + at] = total[p];
    }
}

// One wave per row: the seven parameters in binary64, each rounded to float once; the loss over the parameters that count; and what the
// adjoint needs of the row.
__global__ __launch_bounds__(64) void decay_params_fit_kernel(const float * __restrict__ curve, uint64_t nbins, uint32_t ntiles, uint32_t nrows,
                                                               const uint32_t * __restrict__ window, const double * __restrict__ tiles, double sample_rate,
                                                               uint32_t ke50, uint32_t ke80, const float * __restrict__ targets,
                                                               const float * __restrict__ param_weights, float * __restrict__ params,
                                                               DecayParamsRow * __restrict__ rows, double * __restrict__ loss_rows)
{
    const uint32_t r = blockIdx.y;
    const size_t plane = (size_t) nrows * ntiles;
    double sxy[kTimes];
    for (uint32_t p = 0; p < kTimes; ++p) sxy[p] = row_sum(tiles + p * plane + (size_t) r * ntiles, ntiles);
    const double energy = row_sum(tiles + kTimes * plane + (size_t) r * ntiles, ntiles);
    if (threadIdx.x) return;
    const float * row = curve + (size_t) r * nbins;
    const float e0f = row[0];
    const double e0 = (double) e0f;
    const double nan = (double) __builtin_nanf("");
    double q[RVB_DECAY_NPARAMS] = {nan, nan, nan, nan, nan, nan, nan};
    uint32_t k0[kTimes], k1[kTimes];
    windows_of(window + (size_t) r * kFirst, k0, k1);
    double slope[kTimes] = {0.0, 0.0, 0.0}, sxx[kTimes] = {0.0, 0.0, 0.0};
    for (uint32_t p = 0; p < kTimes; ++p) {
        if (e0f > 0.0f && k0[p] != kNone && k1[p] != kNone && k1[p] > k0[p] && k1[p] - k0[p] >= 2u) {
            const double n = (double) (k1[p] - k0[p]);
            sxx[p] = n * (n * n - 1.0) / 12.0;                         // sum of xc^2 over n equally spaced points
            slope[p] = sxy[p] / sxx[p];                                // dB per bin
            q[p] = -60.0 / (slope[p] * sample_rate);
        }
    }
    const uint32_t ke[2] = {ke50, ke80};
    double early[2] = {0.0, 0.0}, late[2] = {0.0, 0.0};
    if (e0f > 0.0f) {
        for (uint32_t c = 0; c < 2; ++c) {
            if (ke[c] == kNone) continue;
            late[c] = (double) row[ke[c]];
            early[c] = e0 - late[c];
            if (early[c] > 0.0 && late[c] > 0.0) q[RVB_DECAY_C50 + c] = kC10 * (log(early[c]) - log(late[c]));
        }
        if (ke[0] != kNone) q[RVB_DECAY_D50] = early[0] / e0;
        q[RVB_DECAY_TS] = energy / (sample_rate * e0);
    }
    double c[RVB_DECAY_NPARAMS], loss = 0.0;
    bool any = false;
    for (uint32_t p = 0; p < RVB_DECAY_NPARAMS; ++p) {
        c[p] = 0.0;
        params[(size_t) r * RVB_DECAY_NPARAMS + p] = (float) q[p];
        if (!targets) continue;
        const float weight = param_weights[(size_t) r * RVB_DECAY_NPARAMS + p];
        if (!(weight > 0.0f) || !isfinite(q[p])) continue;
        const double d = q[p] - (double) targets[(size_t) r * RVB_DECAY_NPARAMS + p];
        c[p] = (2.0 * (double) weight) * d;
        loss = loss + ((double) weight * d) * d;
        any = true;
    }
    DecayParamsRow b;
    for (uint32_t p = 0; p < kTimes; ++p) {
        const bool counts = c[p] != 0.0;
        b.k0[p] = counts ? k0[p] : 0u;
        b.k1[p] = counts ? k1[p] : 0u;
        b.centre[p] = counts ? 0.5 * (double) (k1[p] - k0[p] - 1u) : 0.0;
        b.time_coef[p] = counts ? c[p] * (60.0 / ((slope[p] * slope[p]) * sample_rate)) * kC10 / sxx[p] : 0.0;
    }
    for (uint32_t i = 0; i < 2; ++i) {
        const bool counts = c[RVB_DECAY_C50 + i] != 0.0;                   // (then early > 0 and late > 0)
        b.c_zero[i] = counts ? c[RVB_DECAY_C50 + i] * kC10 / early[i] : 0.0;
        b.c_at[i] = counts ? (c[RVB_DECAY_C50 + i] * kC10) * (1.0 / early[i] + 1.0 / late[i]) : 0.0;
        b.ke[i] = ke[i];
    }
    const bool d_counts = c[RVB_DECAY_D50] != 0.0, ts_counts = c[RVB_DECAY_TS] != 0.0;     // (then E[0] > 0)
    b.d_zero = d_counts ? c[RVB_DECAY_D50] * late[0] / (e0 * e0) : 0.0;
    b.d_at = d_counts ? c[RVB_DECAY_D50] / e0 : 0.0;
    b.ts_zero = ts_counts ? c[RVB_DECAY_TS] * q[RVB_DECAY_TS] / e0 : 0.0;
    b.ts_each = ts_counts ? c[RVB_DECAY_TS] / (sample_rate * e0) : 0.0;
    b.counts = any ? 1u : 0u;
    rows[r] = b;
    loss_rows[r] = loss;
}

// ---- the adjoint -----------------------------------------------------------------------------------------------------------------------
// g[k] = dL/dE[k], the terms in the order of the parameter numbers; the three time terms share their division by E[k].

__device__ inline double adjoint_bin(const DecayParamsRow & b, uint64_t k, uint64_t nbins, float e)
{
    if (k >= nbins) return 0.0;
    double lin = 0.0;
    bool in = false;
#pragma unroll
    for (uint32_t p = 0; p < kTimes; ++p) {
        if (k >= b.k0[p] && k < b.k1[p]) {
            lin = lin + b.time_coef[p] * ((double) (k - b.k0[p]) - b.centre[p]);
            in = true;
        }
    }
    double g = in ? lin / (double) e : 0.0;                            // (inside a window that counts E[k] > 0)
    if (k == 0) g = g + b.c_zero[0];
    if (k == b.ke[0]) g = g - b.c_at[0];
    if (k == 0) g = g + b.c_zero[1];
    if (k == b.ke[1]) g = g - b.c_at[1];
    if (k == b.ke[0]) g = g - b.d_at;
    if (k == 0) g = (g + b.d_zero) - b.ts_zero;
    else g = g + b.ts_each;
    return g;
}

__device__ inline void adjoint_chunks(const DecayParamsRow & b, const float * __restrict__ e, uint32_t tile, uint64_t nbins, double (&g)[kChunks][4],
                                      double (&sum)[kChunks])
{
#pragma unroll
    for (uint32_t i = 0; i < kChunks; ++i) {
        const uint64_t bin = chunk_bin(tile, i);
        const float4 v = load4(e, bin, nbins);
        const float ee[4] = {v.x, v.y, v.z, v.w};
        sum[i] = 0.0;
#pragma unroll
        for (uint32_t j = 0; j < 4; ++j) {
            g[i][j] = adjoint_bin(b, bin + j, nbins, ee[j]);
            sum[i] = sum[i] + g[i][j];
        }
    }
}

__global__ __launch_bounds__(kLanes) void decay_params_adjoint_sums_kernel(const float * __restrict__ curve, uint64_t nbins, uint32_t ntiles,
                                                                            const DecayParamsRow * __restrict__ rows, double * __restrict__ tiles)
{
    __shared__ double totals[kSegments];
    const uint32_t tile = blockIdx.x, r = blockIdx.y;
    const DecayParamsRow b = rows[r];
    double g[kChunks][4], sum[kChunks];
    adjoint_chunks(b, curve + (size_t) r * nbins, tile, nbins, g, sum);
    const double total = tile_sum(sum, totals);
    if (threadIdx.x == 0) tiles[(size_t) r * ntiles + tile] = total;
}

__global__ __launch_bounds__(64) void decay_params_adjoint_carry_kernel(double * __restrict__ tiles, uint32_t ntiles)
{
    (void) row_carry<false>(tiles + (size_t) blockIdx.y * ntiles, ntiles, 0.0);
}

__global__ __launch_bounds__(kLanes) void decay_params_adjoint_scan_kernel(const float * __restrict__ hist, const float * __restrict__ curve, uint64_t nbins,
                                                                            uint32_t ntiles, const DecayParamsRow * __restrict__ rows,
                                                                            const double * __restrict__ tiles, float * __restrict__ weights)
{
    __shared__ double totals[kSegments];
    const uint32_t tile = blockIdx.x, r = blockIdx.y;
    const DecayParamsRow b = rows[r];
    const float * h = hist + (size_t) r * nbins;
    double g[kChunks][4], before[kChunks];
    adjoint_chunks(b, curve + (size_t) r * nbins, tile, nbins, g, before);
    (void) tile_scan<false>(before, totals);
    const double carry = tiles[(size_t) r * ntiles + tile];
    float * out = weights + (size_t) r * nbins;
#pragma unroll
    for (uint32_t i = 0; i < kChunks; ++i) {
        const uint64_t bin = chunk_bin(tile, i);
        const float4 vh = load4(h, bin, nbins);
        const float hh[4] = {vh.x, vh.y, vh.z, vh.w};
        float o[4];
        double s = carry + before[i];
#pragma unroll
        for (uint32_t j = 0; j < 4; ++j) {
            s = s + g[i][j];
            o[j] = (hh[j] == 0.0f || !b.counts) ? 0.0f : (float) ((2.0 * (double) hh[j]) * s);
        }
        store4(out, bin, nbins, make_float4(o[0], o[1], o[2], o[3]));
    }
}

} // namespace

void rvb_launch_decay_params_find(const float * curve, uint64_t nrows, uint64_t nbins, const DecayParamsRatios & ratios, uint32_t * first, hipStream_t s)
{
    const uint32_t ntiles = rvb_decay_tiles(nbins);
    decay_params_find_kernel<<<dim3(ntiles, (uint32_t) nrows), kLanes, 0, s>>>(curve, nbins, ntiles, (uint32_t) nrows, ratios, first);
}

void rvb_launch_decay_params_window(const uint32_t * first, uint64_t nrows, uint64_t nbins, uint32_t * window, hipStream_t s)
{
    decay_params_window_kernel<<<dim3(1, (uint32_t) nrows), 64, 0, s>>>(first, rvb_decay_tiles(nbins), (uint32_t) nrows, window);
}

void rvb_launch_decay_params_sums(const float * curve, uint64_t nrows, uint64_t nbins, const uint32_t * window, double * tiles, hipStream_t s)
{
    const uint32_t ntiles = rvb_decay_tiles(nbins);
    decay_params_sums_kernel<<<dim3(ntiles, (uint32_t) nrows), kLanes, 0, s>>>(curve, nbins, ntiles, (uint32_t) nrows, window, tiles);
}

void rvb_launch_decay_params_fit(const float * curve, uint64_t nrows, uint64_t nbins, const uint32_t * window, const double * tiles, double sample_rate,
                                 uint32_t ke50, uint32_t ke80, const float * targets, const float * param_weights, float * params,
                                 DecayParamsRow * rows, double * loss_rows, hipStream_t s)
{
    decay_params_fit_kernel<<<dim3(1, (uint32_t) nrows), 64, 0, s>>>(curve, nbins, rvb_decay_tiles(nbins), (uint32_t) nrows, window, tiles, sample_rate,
                                                                      ke50, ke80, targets, param_weights, params, rows, loss_rows);
}

void rvb_launch_decay_params_adjoint_sums(const float * curve, uint64_t nrows, uint64_t nbins, const DecayParamsRow * rows, double * tiles, hipStream_t s)
{
    const uint32_t ntiles = rvb_decay_tiles(nbins);
    decay_params_adjoint_sums_kernel<<<dim3(ntiles, (uint32_t) nrows), kLanes, 0, s>>>(curve, nbins, ntiles, rows, tiles);
}

void rvb_launch_decay_params_adjoint_carry(uint64_t nrows, uint64_t nbins, double * tiles, hipStream_t s)
{
    decay_params_adjoint_carry_kernel<<<dim3(1, (uint32_t) nrows), 64, 0, s>>>(tiles, rvb_decay_tiles(nbins));
}

void rvb_launch_decay_params_adjoint_scan(const float * hist, const float * curve, uint64_t nrows, uint64_t nbins, const DecayParamsRow * rows,
                                          const double * tiles, float * weights, hipStream_t s)
{
    const uint32_t ntiles = rvb_decay_tiles(nbins);
    decay_params_adjoint_scan_kernel<<<dim3(ntiles, (uint32_t) nrows), kLanes, 0, s>>>(hist, curve, nbins, ntiles, rows, tiles, weights);
}
