// histogram_kernels.hip — the fast mode of the fused impulse-response stage: attenuation, predelay and time bin of every impulse in one
// pass, added with float atomics into the accumulation image acc[bin][channel][band], then transposed into the histogram.
//
// HBM-bound, 64 B in per impulse.  16 lanes per impulse, so that the 8 band volumes sit one per lane and one wave-wide float-atomic instruction adds
// 4 impulses x (2 channels x 8 bands) = 4 x 64 contiguous bytes (memory-side atomics are paid per 64-byte request — MI355X_MICROARCH "Global float atomics").
#include "attenuation.h"

#define HIST_ROW 20     // LDS words per staged impulse: 16 record words + padding (b128-aligned, 4-way conflicts at most)
#define HIST_MAXCH 8
// HIST_WAVES waves per workgroup, each with a staging area of its own (no cross-wave traffic).  One-wave workgroups: when
// another impulse response's path_kernel holds 24 of a CU's 32 wave slots (IrPipeline), a four-wave workgroup finds room on a
// CU only now and then, single waves slip into the free slots.
#define HIST_WAVES 1
#define TR_BINS 64      // bins per tile of the transpose

namespace {

// Two phases per 64 impulses of a wave, through LDS:
//   1. impulse per lane: gain of every channel and the bin — computed ONCE per impulse
//      (the 16-lanes-per-impulse layout would recompute them in 16 lanes: ~30 wave instructions per
//      impulse, issue-bound; this form needs ~5);
//   2. 16 lanes per impulse (8 bands x 2 channels): one float-atomic wave instruction adds
//      4 impulses x 64 contiguous bytes.
__global__ __launch_bounds__(64 * HIST_WAVES) void histogram_fast_kernel(ModelDev m, const float4 * __restrict__ in, uint64_t n,
                                                             float predelay, float sample_rate, uint64_t nbins,
                                                             float * __restrict__ acc)
{
    __shared__ __attribute__((aligned(16))) float stage[HIST_WAVES][64 * HIST_ROW];      // the wave's 64 records
    __shared__ float gains[HIST_WAVES][64 * HIST_MAXCH];
    __shared__ uint32_t bins[HIST_WAVES][64 * 2];                                        // speakers: one bin; hrtf: one per ear
    const uint32_t wave = threadIdx.x >> 6, lane = threadIdx.x & 63u;
    float * st = stage[wave];
    float * gn = gains[wave];
    uint32_t * bn = bins[wave];
    const uint64_t nwaves = (uint64_t) gridDim.x * HIST_WAVES;
    const uint64_t ngroups = (n + 63) / 64;
    const uint32_t f = lane & 15u, band = f & 7u, chsel = f >> 3;
    for (uint64_t grp = (uint64_t) blockIdx.x * HIST_WAVES + wave; grp < ngroups; grp += nwaves) {
        const uint64_t first = grp * 64;
        // stage 64 records (4 KiB) with four fully coalesced 1-KiB wave loads
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const uint64_t chunk = first * 4 + (uint64_t) k * 64 + lane;        // 16-byte chunk index
            float4 v = make_float4(0, 0, 0, 0);
            if (chunk < n * 4) {
                const nt_float4_t t = __builtin_nontemporal_load(reinterpret_cast<const nt_float4_t *>(in) + chunk);
                v = make_float4(t.x, t.y, t.z, t.w);
            }
            const uint32_t imp = (uint32_t) ((k * 64 + lane) >> 2), part = lane & 3u;
            *reinterpret_cast<float4 *>(st + imp * HIST_ROW + part * 4) = v;
        }
        __builtin_amdgcn_s_waitcnt(0xC07F);     // lgkmcnt(0): the wave's own LDS writes (one wave per staging area)
        __builtin_amdgcn_wave_barrier();
        // phase 1: lane = impulse
        {
            const float4 v0 = *reinterpret_cast<const float4 *>(st + lane * HIST_ROW);
            const float4 v1 = *reinterpret_cast<const float4 *>(st + lane * HIST_ROW + 4);
            const float4 p4 = *reinterpret_cast<const float4 *>(st + lane * HIST_ROW + 8);
            const float time = st[lane * HIST_ROW + 12];
            const bool nonzero = ANY_VOLUME(v0, v1);
            const v3 pos = mk3(p4.x, p4.y, p4.z);
            uint32_t b0 = 0xFFFFFFFFu, b1 = 0xFFFFFFFFu;                       // 0xFFFFFFFF: contributes nothing
            if (nonzero && first + lane < n) {
                if (m.hrtf) {
                    const int64_t row = hrtf_row(m, pos);
                    // gains of an hrtf impulse are per band: keep the row, phase 2 reads the table
                    gn[lane * HIST_MAXCH] = __uint_as_float((uint32_t) row);
                    b0 = time_bin(hrtf_time(m, 0, pos, time), predelay, sample_rate);
                    b1 = time_bin(hrtf_time(m, 1, pos, time), predelay, sample_rate);
                } else {
                    for (uint32_t ch = 0; ch < m.nchannels; ++ch)
                        gn[lane * HIST_MAXCH + ch] = speaker_gain(m, ch, pos);
                    b0 = b1 = time_bin(time, predelay, sample_rate);
                }
            }
            bn[lane * 2] = b0;
            bn[lane * 2 + 1] = b1;
        }
        __builtin_amdgcn_s_waitcnt(0xC07F);
        __builtin_amdgcn_wave_barrier();
        // phase 2: 16 lanes per impulse, 4 impulses per wave instruction
        for (uint32_t j = 0; j < 16; ++j) {
            const uint32_t imp = j * 4 + (lane >> 4);
            const float vol = st[imp * HIST_ROW + band];
            for (uint32_t pair = 0; pair < m.nchannels; pair += 2) {
                const uint32_t ch = pair + chsel;
                if (ch >= m.nchannels)
                    continue;
                const uint64_t bin = bn[imp * 2 + (m.hrtf ? ch : 0)];
                if (bin >= nbins)
                    continue;                      // zero-volume impulse (or beyond the histogram)
                float gain;
                if (m.hrtf) gain = m.table[((uint64_t) ch * RVB_HRTF_ROWS + (uint64_t) __float_as_uint(gn[imp * HIST_MAXCH])) * 8 + band];
                else gain = gn[imp * HIST_MAXCH + ch];
                atomicAdd(acc + (bin * m.nchannels + ch) * 8 + band, vol * gain);
            }
        }
        __builtin_amdgcn_wave_barrier();          // staging area is reused by the next group
    }
}

// acc[bin][ch][band] -> out[ch][band][bin] (+=, so that several shards / image passes can add up).
// 64-bin tiles through LDS: the read is one contiguous span, the writes are 256-byte runs per (ch, band).
__global__ __launch_bounds__(256) void histogram_transpose_kernel(const float * __restrict__ acc, float * __restrict__ out,
                                                                  uint32_t nchannels, uint64_t nbins)
{
    __shared__ float tile[64][TR_BINS + 1];                  // [ch*8+band][bin], up to 8 channels
    const uint32_t cb = nchannels * 8;
    const uint64_t ntiles = (nbins + TR_BINS - 1) / TR_BINS;
    for (uint64_t t = blockIdx.x; t < ntiles; t += gridDim.x) {
        const uint64_t bin0 = t * TR_BINS;
        const uint32_t count = (uint32_t) min((uint64_t) TR_BINS, nbins - bin0) * cb;
        for (uint32_t i = threadIdx.x; i < count; i += 256)
            tile[i % cb][i / cb] = acc[bin0 * cb + i];
        __syncthreads();
        const uint32_t width = (uint32_t) min((uint64_t) TR_BINS, nbins - bin0);
        for (uint32_t i = threadIdx.x; i < cb * TR_BINS; i += 256) {
            const uint32_t row = i / TR_BINS, col = i % TR_BINS;
            if (col < width)
                out[(uint64_t) row * nbins + bin0 + col] += tile[row][col];
        }
        __syncthreads();
    }
}

// acc += x: one device's histogram added to another's (the peer-copy sum of csrc/multi.hip's fast mode)
__global__ __launch_bounds__(256) void add_kernel(float * __restrict__ acc, const float * __restrict__ x, uint64_t n)
{
    for (uint64_t i = (uint64_t) blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (uint64_t) gridDim.x * blockDim.x)
        acc[i] += x[i];
}

}  // namespace

void rvb_launch_histogram_fast(const AttenuationModel & m, const rvb_impulse * in, uint64_t n, float predelay,
                               float sample_rate, uint64_t nbins, float * acc, hipStream_t s)
{
    if (n == 0) return;
    hipLaunchKernelGGL(histogram_fast_kernel, dim3(stream_blocks(n, 64 * HIST_WAVES)), dim3(64 * HIST_WAVES), 0, s, make_model(m),
                       reinterpret_cast<const float4 *>(in), n, predelay, sample_rate, nbins, acc);
}

void rvb_launch_histogram_transpose(const float * acc, float * out, uint32_t nchannels, uint64_t nbins, hipStream_t s)
{
    hipLaunchKernelGGL(histogram_transpose_kernel, dim3(stream_blocks((nbins + TR_BINS - 1) / TR_BINS * 256, 256)), dim3(256), 0, s,
                       acc, out, nchannels, nbins);
}

void rvb_launch_add(float * acc, const float * x, uint64_t n, hipStream_t s)
{
    hipLaunchKernelGGL(add_kernel, dim3(4096), dim3(256), 0, s, acc, x, n);
}
