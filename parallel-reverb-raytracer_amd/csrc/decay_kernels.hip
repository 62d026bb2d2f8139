// decay_kernels.hip — energy decay curves on the device (rvb_decay_curve / rvb_decay_times / rvb_decay_loss of include/rvb_capi.h):
// the Schroeder integral of rows of bins, the reverberation time of a curve, and the loss against a target decay with its adjoint.
//
// ONE SHAPE for all three.  A row of nbins floats is cut into tiles of RVB_DECAY_TILE = 4096 bins; rows run along gridDim.y, tiles
// along x.  A workgroup of 256 lanes takes one tile as 1024 CHUNKS of 4 consecutive bins: lane t holds chunks i * 256 + t, i = 0..3, so
// that a wave's loads are 64 consecutive 16-byte pieces (a row starts wherever r * nbins puts it, so the pieces are 4-byte aligned
// only; the hardware takes that).  Every call is three or four launches and no workgroup ever waits for another:
//   *_sums_kernel    one binary64 sum (or first-index) per tile                            grid (tiles, rows)
//   *_carry_kernel   ONE WAVE per row walks the row's tile values in order, 64 at a time   grid (1, rows)
//   *_scan_kernel    the tile again, scanned in chunk order on top of its carry            grid (tiles, rows)
// THE ORDER of every sum is fixed by (tile, chunk, bin) alone — per lane the bins of a chunk one after the other, chunks across a wave
// by a shuffle ladder, the 16 (i, wave) segments of a tile one after the other, tiles one after the other — never by which workgroup
// ran first: no atomics, no flags, identical bytes from call to call.  All sums are binary64; a result is rounded to float once.
#include "decay_tiles.h"

#include <math.h>

namespace {

__device__ inline double square(float h) { const double d = (double) h; return d * d; }

// ---- the Schroeder integral ----------------------------------------------------------------------------------------------------------

__device__ inline void curve_chunks(const float * __restrict__ row, uint32_t tile, uint64_t nbins, double (&e)[kChunks][4], double (&sum)[kChunks])
{
#pragma unroll
    for (uint32_t i = 0; i < kChunks; ++i) {
        const float4 h = load4(row, chunk_bin(tile, i), nbins);
        e[i][0] = square(h.x); e[i][1] = square(h.y); e[i][2] = square(h.z); e[i][3] = square(h.w);
        sum[i] = ((e[i][3] + e[i][2]) + e[i][1]) + e[i][0];          // from the chunk's last bin to its first, as the scan walks
    }
}

__global__ __launch_bounds__(kLanes) void decay_curve_sums_kernel(const float * __restrict__ hist, uint64_t nbins, uint32_t ntiles, double * __restrict__ tiles)
{
    __shared__ double totals[kSegments];
    const uint32_t tile = blockIdx.x, r = blockIdx.y;
    double e[kChunks][4], sum[kChunks];
    curve_chunks(hist + (size_t) r * nbins, tile, nbins, e, sum);
    const double total = tile_scan<true>(sum, totals);
    if (threadIdx.x == 0) tiles[(size_t) r * ntiles + tile] = total;
}

__global__ __launch_bounds__(64) void decay_curve_carry_kernel(double * __restrict__ tiles, uint32_t ntiles)
{
    (void) row_carry<true>(tiles + (size_t) blockIdx.y * ntiles, ntiles, 0.0);
}

__global__ __launch_bounds__(kLanes) void decay_curve_scan_kernel(const float * __restrict__ hist, uint64_t nbins, uint32_t ntiles,
                                                                   const double * __restrict__ tiles, float * __restrict__ curve)
{
    __shared__ double totals[kSegments];
    const uint32_t tile = blockIdx.x, r = blockIdx.y;
    double e[kChunks][4], behind[kChunks];
    curve_chunks(hist + (size_t) r * nbins, tile, nbins, e, behind);
    (void) tile_scan<true>(behind, totals);
    const double carry = tiles[(size_t) r * ntiles + tile];
    float * out = curve + (size_t) r * nbins;
#pragma unroll
    for (uint32_t i = 0; i < kChunks; ++i) {
        double s = carry + behind[i];
        float4 o;
        s = s + e[i][3]; o.w = (float) s;
        s = s + e[i][2]; o.z = (float) s;
        s = s + e[i][1]; o.y = (float) s;
        s = s + e[i][0]; o.x = (float) s;
        store4(out, chunk_bin(tile, i), nbins, o);
    }
}

// ---- reverberation times -------------------------------------------------------------------------------------------------------------
// first[0][row][tile] / first[1][row][tile]: the first bin of the tile with E <= begin / E < end (0xFFFFFFFF: none), the thresholds
// E[0] * 10^(db / 10) per row.

__global__ __launch_bounds__(kLanes) void decay_times_find_kernel(const float * __restrict__ curve, uint64_t nbins, uint32_t ntiles, uint32_t nrows,
                                                                   double ratio_begin, double ratio_end, uint32_t * __restrict__ first)
{
    __shared__ uint32_t found[2][kLanes / 64];
    const uint32_t tile = blockIdx.x, r = blockIdx.y;
    const float * row = curve + (size_t) r * nbins;
    const double e0 = (double) row[0];
    const double begin = e0 * ratio_begin, end = e0 * ratio_end;
    uint32_t mine[2] = {0xFFFFFFFFu, 0xFFFFFFFFu};
#pragma unroll
    for (uint32_t i = 0; i < kChunks; ++i) {
        const uint64_t bin = chunk_bin(tile, i);
        const float4 v = load4(row, bin, nbins);
        const float e[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
        for (uint32_t j = 0; j < 4; ++j) {
            if (bin + j >= nbins) continue;
            const double x = (double) e[j];
            if (x <= begin) mine[0] = min(mine[0], (uint32_t) (bin + j));
            if (x < end) mine[1] = min(mine[1], (uint32_t) (bin + j));
        }
    }
#pragma unroll
    for (uint32_t w = 0; w < 2; ++w) {
        for (uint32_t d = 32; d; d >>= 1) mine[w] = min(mine[w], (uint32_t) __shfl_xor((int) mine[w], (int) d, 64));
        if ((threadIdx.x & 63u) == 0) found[w][threadIdx.x >> 6] = mine[w];
    }
    __syncthreads();
    if (threadIdx.x < 2) {
        const uint32_t * f = found[threadIdx.x];
        first[((size_t) threadIdx.x * nrows + r) * ntiles + tile] = min(min(f[0], f[1]), min(f[2], f[3]));
    }
}

// window[row] = {k0, k1}; k1 = 0xFFFFFFFF: the curve never falls below the end level
__global__ __launch_bounds__(64) void decay_times_window_kernel(const uint32_t * __restrict__ first, uint32_t ntiles, uint32_t nrows, uint2 * __restrict__ window)
{
    const uint32_t r = blockIdx.y;
    uint32_t k[2];
    for (uint32_t w = 0; w < 2; ++w) {
        const uint32_t * f = first + ((size_t) w * nrows + r) * ntiles;
        uint32_t m = 0xFFFFFFFFu;
        for (uint32_t t = threadIdx.x; t < ntiles; t += 64) m = min(m, f[t]);
        for (uint32_t d = 32; d; d >>= 1) m = min(m, (uint32_t) __shfl_xor((int) m, (int) d, 64));
        k[w] = m;
    }
    if (threadIdx.x == 0) window[r] = make_uint2(k[0], k[1]);
}

// per tile: sum over its bins k in [k0, k1) of xc * level, level = 10 log10(E[k] / E[0]), xc = (k - k0) - (k1 - k0 - 1) / 2
__global__ __launch_bounds__(kLanes) void decay_times_sums_kernel(const float * __restrict__ curve, uint64_t nbins, uint32_t ntiles,
                                                                   const uint2 * __restrict__ window, double * __restrict__ tiles)
{
    __shared__ double totals[kSegments];
    const uint32_t tile = blockIdx.x, r = blockIdx.y;
    const float * row = curve + (size_t) r * nbins;
    const uint2 w = window[r];
    const uint64_t lo = (uint64_t) tile * kTile, hi = lo + kTile;
    const bool any = w.y != 0xFFFFFFFFu && w.x != 0xFFFFFFFFu && w.x < w.y && lo < w.y && hi > w.x;      // (uniform over the workgroup)
    double sum[kChunks] = {0.0, 0.0, 0.0, 0.0};
    if (any) {
        const double e0 = (double) row[0];
        const double centre = 0.5 * (double) (w.y - w.x - 1u);
#pragma unroll
        for (uint32_t i = 0; i < kChunks; ++i) {
            const uint64_t bin = chunk_bin(tile, i);
            if (bin + 4 <= w.x || bin >= w.y) continue;
            const float4 v = load4(row, bin, nbins);
            const float e[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
            for (uint32_t j = 0; j < 4; ++j) {
                const uint64_t k = bin + j;
                if (k < w.x || k >= w.y) continue;
                const double level = 10.0 * log10((double) e[j] / e0);
                const double xc = (double) (k - w.x) - centre;
                sum[i] = sum[i] + xc * level;
            }
        }
    }
    const double total = tile_sum(sum, totals);
    if (threadIdx.x == 0) tiles[(size_t) r * ntiles + tile] = total;
}

__global__ __launch_bounds__(64) void decay_times_fit_kernel(const float * __restrict__ curve, uint64_t nbins, uint32_t ntiles, const uint2 * __restrict__ window,
                                                              const double * __restrict__ tiles, double sample_rate, float * __restrict__ seconds)
{
    const uint32_t r = blockIdx.y;
    const double sxy = row_sum(tiles + (size_t) r * ntiles, ntiles);
    if (threadIdx.x) return;
    const uint2 w = window[r];
    const float e0 = curve[(size_t) r * nbins];
    float out = __builtin_nanf("");
    if (e0 > 0.0f && w.x != 0xFFFFFFFFu && w.y != 0xFFFFFFFFu && w.y > w.x && w.y - w.x >= 2u) {
        const double n = (double) (w.y - w.x);
        const double sxx = n * (n * n - 1.0) / 12.0;                   // sum of xc^2 over n equally spaced points
        const double slope = sxy / sxx;                                // dB per bin
        out = (float) (-60.0 / (slope * sample_rate));
    }
    seconds[r] = out;
}

// ---- loss against a target decay, and its adjoint --------------------------------------------------------------------------------------
// Per bin that counts (m > 0, E > 0, T > 0, and the row counts): d = ln E - ln T - shift, g = 2 m d / E.  Tile values, three arrays of
// [rows][tiles]: sum m d^2, sum 2 m d, sum g.

struct LossRow { bool counts; double shift; };

__device__ inline LossRow loss_row(const float * __restrict__ e, const float * __restrict__ t, bool normalised)
{
    LossRow r = {true, 0.0};
    if (normalised) {
        const float e0 = e[0], t0 = t[0];
        r.counts = e0 > 0.0f && t0 > 0.0f;
        if (r.counts) r.shift = log((double) e0) - log((double) t0);
    }
    return r;
}

__device__ inline void loss_bin(float e, float t, float m, const LossRow & row, double & md2, double & md, double & g)
{
    md2 = 0.0; md = 0.0; g = 0.0;
    if (!(row.counts && m > 0.0f && e > 0.0f && t > 0.0f)) return;
    const double d = (log((double) e) - log((double) t)) - row.shift;
    const double two_md = (2.0 * (double) m) * d;
    md2 = ((double) m * d) * d;
    md = two_md;
    g = two_md / (double) e;
}

__global__ __launch_bounds__(kLanes) void decay_loss_sums_kernel(const float * __restrict__ curve, const float * __restrict__ target, const float * __restrict__ mask,
                                                                  uint64_t nbins, uint32_t ntiles, uint32_t nrows, int normalised, double * __restrict__ tiles)
{
    __shared__ double totals[3][kSegments];
    const uint32_t tile = blockIdx.x, r = blockIdx.y;
    const float * e = curve + (size_t) r * nbins, * t = target + (size_t) r * nbins, * m = mask + (size_t) r * nbins;
    const LossRow row = loss_row(e, t, normalised != 0);
    double s2[kChunks], s1[kChunks], sg[kChunks];
#pragma unroll
    for (uint32_t i = 0; i < kChunks; ++i) {
        const uint64_t bin = chunk_bin(tile, i);
        const float4 ve = load4(e, bin, nbins), vt = load4(t, bin, nbins), vm = load4(m, bin, nbins);
        const float ee[4] = {ve.x, ve.y, ve.z, ve.w}, tt[4] = {vt.x, vt.y, vt.z, vt.w}, mm[4] = {vm.x, vm.y, vm.z, vm.w};
        s2[i] = 0.0; s1[i] = 0.0; sg[i] = 0.0;
#pragma unroll
        for (uint32_t j = 0; j < 4; ++j) {
            double a, b, c;
            loss_bin(ee[j], tt[j], mm[j], row, a, b, c);
            s2[i] = s2[i] + a; s1[i] = s1[i] + b; sg[i] = sg[i] + c;
        }
    }
    const double t2 = tile_sum(s2, totals[0]), t1 = tile_sum(s1, totals[1]), tg = tile_sum(sg, totals[2]);
    if (threadIdx.x == 0) {
        const size_t at = (size_t) r * ntiles + tile, plane = (size_t) nrows * ntiles;
        tiles[at] = t2;
        tiles[plane + at] = t1;
        tiles[2 * plane + at] = tg;
    }
}

// One wave per row: the row's loss, and the sum of g over the tiles before each tile — with RVB_DECAY_NORMALISED on top of the term
// that E[0] adds to g[0], -(sum 2 m d) / E[0].
__global__ __launch_bounds__(64) void decay_loss_carry_kernel(const float * __restrict__ curve, uint64_t nbins, uint32_t ntiles, uint32_t nrows, int normalised,
                                                               double * __restrict__ tiles, double * __restrict__ loss_rows)
{
    const uint32_t r = blockIdx.y;
    const size_t plane = (size_t) nrows * ntiles;
    const double loss = row_sum(tiles + (size_t) r * ntiles, ntiles);
    double start = 0.0;
    if (normalised) {
        const double s = row_sum(tiles + plane + (size_t) r * ntiles, ntiles);
        const float e0 = curve[(size_t) r * nbins];
        if (e0 > 0.0f) start = -(s / (double) e0);                     // (a row that does not count has s == 0)
    }
    (void) row_carry<false>(tiles + 2 * plane + (size_t) r * ntiles, ntiles, start);
    if (threadIdx.x == 0) loss_rows[r] = loss;
}

__global__ __launch_bounds__(kLanes) void decay_loss_scan_kernel(const float * __restrict__ hist, const float * __restrict__ curve, const float * __restrict__ target,
                                                                  const float * __restrict__ mask, uint64_t nbins, uint32_t ntiles, uint32_t nrows, int normalised,
                                                                  const double * __restrict__ tiles, float * __restrict__ weights)
{
    __shared__ double totals[kSegments];
    const uint32_t tile = blockIdx.x, r = blockIdx.y;
    const float * h = hist + (size_t) r * nbins, * e = curve + (size_t) r * nbins, * t = target + (size_t) r * nbins, * m = mask + (size_t) r * nbins;
    const LossRow row = loss_row(e, t, normalised != 0);
    double g[kChunks][4], before[kChunks];
#pragma unroll
    for (uint32_t i = 0; i < kChunks; ++i) {
        const uint64_t bin = chunk_bin(tile, i);
        const float4 ve = load4(e, bin, nbins), vt = load4(t, bin, nbins), vm = load4(m, bin, nbins);
        const float ee[4] = {ve.x, ve.y, ve.z, ve.w}, tt[4] = {vt.x, vt.y, vt.z, vt.w}, mm[4] = {vm.x, vm.y, vm.z, vm.w};
        before[i] = 0.0;
#pragma unroll
        for (uint32_t j = 0; j < 4; ++j) {
            double a, b;
            loss_bin(ee[j], tt[j], mm[j], row, a, b, g[i][j]);
            before[i] = before[i] + g[i][j];
        }
    }
    (void) tile_scan<false>(before, totals);
    const double carry = tiles[2 * (size_t) nrows * ntiles + (size_t) r * ntiles + tile];
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
            o[j] = (hh[j] == 0.0f || !row.counts) ? 0.0f : (float) ((2.0 * (double) hh[j]) * s);
        }
        store4(out, bin, nbins, make_float4(o[0], o[1], o[2], o[3]));
    }
}

} // namespace

void rvb_launch_decay_curve_sums(const float * hist, uint64_t nrows, uint64_t nbins, double * tiles, hipStream_t s)
{
    const uint32_t ntiles = rvb_decay_tiles(nbins);
    decay_curve_sums_kernel<<<dim3(ntiles, (uint32_t) nrows), kLanes, 0, s>>>(hist, nbins, ntiles, tiles);
}

void rvb_launch_decay_curve_carry(uint64_t nrows, uint64_t nbins, double * tiles, hipStream_t s)
{
    decay_curve_carry_kernel<<<dim3(1, (uint32_t) nrows), 64, 0, s>>>(tiles, rvb_decay_tiles(nbins));
}

void rvb_launch_decay_curve_scan(const float * hist, uint64_t nrows, uint64_t nbins, const double * tiles, float * curve, hipStream_t s)
{
    const uint32_t ntiles = rvb_decay_tiles(nbins);
    decay_curve_scan_kernel<<<dim3(ntiles, (uint32_t) nrows), kLanes, 0, s>>>(hist, nbins, ntiles, tiles, curve);
}

void rvb_launch_decay_times_find(const float * curve, uint64_t nrows, uint64_t nbins, double ratio_begin, double ratio_end, uint32_t * first, hipStream_t s)
{
    const uint32_t ntiles = rvb_decay_tiles(nbins);
    decay_times_find_kernel<<<dim3(ntiles, (uint32_t) nrows), kLanes, 0, s>>>(curve, nbins, ntiles, (uint32_t) nrows, ratio_begin, ratio_end, first);
}

void rvb_launch_decay_times_window(const uint32_t * first, uint64_t nrows, uint64_t nbins, uint2 * window, hipStream_t s)
{
    decay_times_window_kernel<<<dim3(1, (uint32_t) nrows), 64, 0, s>>>(first, rvb_decay_tiles(nbins), (uint32_t) nrows, window);
}

void rvb_launch_decay_times_sums(const float * curve, uint64_t nrows, uint64_t nbins, const uint2 * window, double * tiles, hipStream_t s)
{
    const uint32_t ntiles = rvb_decay_tiles(nbins);
    decay_times_sums_kernel<<<dim3(ntiles, (uint32_t) nrows), kLanes, 0, s>>>(curve, nbins, ntiles, window, tiles);
}

void rvb_launch_decay_times_fit(const float * curve, uint64_t nrows, uint64_t nbins, const uint2 * window, const double * tiles, double sample_rate,
                                float * seconds, hipStream_t s)
{
    decay_times_fit_kernel<<<dim3(1, (uint32_t) nrows), 64, 0, s>>>(curve, nbins, rvb_decay_tiles(nbins), window, tiles, sample_rate, seconds);
}

void rvb_launch_decay_loss_sums(const float * curve, const float * target, const float * mask, uint64_t nrows, uint64_t nbins, bool normalised,
                                double * tiles, hipStream_t s)
{
    const uint32_t ntiles = rvb_decay_tiles(nbins);
    decay_loss_sums_kernel<<<dim3(ntiles, (uint32_t) nrows), kLanes, 0, s>>>(curve, target, mask, nbins, ntiles, (uint32_t) nrows, normalised ? 1 : 0, tiles);
}

void rvb_launch_decay_loss_carry(const float * curve, uint64_t nrows, uint64_t nbins, bool normalised, double * tiles, double * loss_rows, hipStream_t s)
{
    decay_loss_carry_kernel<<<dim3(1, (uint32_t) nrows), 64, 0, s>>>(curve, nbins, rvb_decay_tiles(nbins), (uint32_t) nrows, normalised ? 1 : 0, tiles, loss_rows);
}

void rvb_launch_decay_loss_scan(const float * hist, const float * curve, const float * target, const float * mask, uint64_t nrows, uint64_t nbins,
                                bool normalised, const double * tiles, float * weights, hipStream_t s)
{
    const uint32_t ntiles = rvb_decay_tiles(nbins);
    decay_loss_scan_kernel<<<dim3(ntiles, (uint32_t) nrows), kLanes, 0, s>>>(hist, curve, target, mask, nbins, ntiles, (uint32_t) nrows, normalised ? 1 : 0, tiles, weights);
}
