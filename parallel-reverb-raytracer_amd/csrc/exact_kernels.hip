// exact_kernels.hip — the exact mode of the fused impulse-response stage and flattenImpulses (rayverb/rayverb.cpp:48-77): a key per impulse
// (its time bin), the bin boundaries of the sorted list (the sort itself: rocprim_sort.hip / radix_sort.hip), and the folds that add a bin's
// impulses in impulse order: up to 8 speaker channels, the two HRTF ears, 9 to RVB_MAX_SPEAKERS channels, already attenuated impulses.
#include "attenuation.h"

#define SUM_UNROLL 4                // records per round of a fold: their index loads, then their record gathers, leave together
#define RVB_HRTF_SUM_THREADS 256    // workgroup of ordered_sum_hrtf_kernel
#define WIDE_BINS 32                // bins per workgroup of ordered_sum_wide_kernel = 64 lanes / 2
#define WIDE_MAX_WAVES 4            // its waves per workgroup: ceil(RVB_MAX_SPEAKERS / 16), and wide_channels_per_wave never asks for more

namespace {

// Key of an impulse = its bin; `sentinel` (= nbins, the first value past every bin) for an impulse that adds nothing.
// Keys therefore need key_bits_for(nbins) bits only (20 at workload C2 instead of 32: three radix passes instead of four).
__global__ __launch_bounds__(256) void bin_keys_kernel(ModelDev m, uint32_t ch, const rvb_impulse * __restrict__ in, uint64_t n,
                                                       uint64_t index_base, float predelay, float sample_rate, uint32_t sentinel,
                                                       uint32_t * __restrict__ keys, uint32_t * __restrict__ values)
{
    for (uint64_t i = (uint64_t) blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (uint64_t) gridDim.x * blockDim.x) {
        const float4 * r = reinterpret_cast<const float4 *>(in + i);
        const float4 v0 = r[0], v1 = r[1], p = r[2];
        const float time = r[3].x;
        const bool nonzero = ANY_VOLUME(v0, v1);
        // A zero-volume impulse attenuates to {0, 0} (quirk Q2): the reference adds its zeros to bin 0, which changes nothing
        // (x + 0 = x, and a sum that starts at +0 never becomes -0).  It gets the sentinel key — sorted last, matched by no
        // bin — instead of bin 0: the blocked third of all shadow rays would otherwise make ONE lane of ordered_sum_kernel walk
        // millions of entries (2.2 s at workload C2).
        uint32_t key = sentinel;
        if (nonzero) key = min(time_bin(attenuated_time(m, ch, mk3(p.x, p.y, p.z), time), predelay, sample_rate), sentinel);
        keys[index_base + i] = key;
        values[index_base + i] = (uint32_t) (index_base + i);
    }
}

// HRTF model: the two ears shift the arrival time differently (kernel.cpp:616-622), so each ear has its own bin per impulse.  Both
// keys come from ONE pass over the impulses, into ONE list of 2 n entries that one radix sort orders: ear e's entry of impulse j
// sits at e * n + j and carries key e * (nbins + 1) + bin (its sentinel: e * (nbins + 1) + nbins), so the sorted list is ear 0's
// bins, ear 0's silent impulses, ear 1's bins, ear 1's silent impulses — each run in impulse order (the sort is stable).
__global__ __launch_bounds__(256) void bin_keys_hrtf_kernel(ModelDev m, const rvb_impulse * __restrict__ in, uint64_t count, uint64_t index_base,
                                                            uint64_t n, float predelay, float sample_rate, uint32_t nbins,
                                                            uint32_t * __restrict__ keys, uint32_t * __restrict__ values)
{
    for (uint64_t i = (uint64_t) blockIdx.x * blockDim.x + threadIdx.x; i < count; i += (uint64_t) gridDim.x * blockDim.x) {
        const float4 * r = reinterpret_cast<const float4 *>(in + i);
        const float4 v0 = r[0], v1 = r[1], p = r[2];
        const float time = r[3].x;
        const bool nonzero = ANY_VOLUME(v0, v1);
        uint32_t k0 = nbins, k1 = nbins;                      // (a zero-volume impulse adds nothing: bin_keys_kernel)
        if (nonzero) {
            const v3 pos = mk3(p.x, p.y, p.z);
            k0 = min(time_bin(hrtf_time(m, 0, pos, time), predelay, sample_rate), nbins);
            k1 = min(time_bin(hrtf_time(m, 1, pos, time), predelay, sample_rate), nbins);
        }
        const uint64_t j = index_base + i;
        keys[j] = k0;
        keys[n + j] = nbins + 1u + k1;
        values[j] = (uint32_t) j;
        values[n + j] = (uint32_t) j;
    }
}

// ---- the live list: only the impulses that carry volume are sorted (a third of workload C2's shadow rays is blocked) ----
// Three plain launches, no workgroup waits for another:
//   live_keys_kernel      a raw key per impulse at the impulse's own position — its bin, the sentinel behind the histogram's end,
//                         LIVE_DEAD without volume — and per tile of RVB_LIVE_TILE consecutive impulses how many carry volume;
//   live_offsets_kernel   one workgroup: the tile counts become where each tile's live impulses start, and their total;
//   live_compact_kernel   (key, impulse number) of every live impulse at its tile's start + its rank within the tile, then sentinel
//                         entries from the total up to the list's length `listed`.
// The impulses are numbered as the fold gathers them: the diffuse ones, then the images.  Tile t is impulses [t, t + 1) * RVB_LIVE_TILE
// whatever the grid; one wave walks it in rounds of 64 consecutive impulses, so a rank is a prefix count of a ballot and the list keeps
// the impulses in their order — with the stable sort, what the fold's sums need.  `listed` comes from the trace's count and bounds the
// live impulses by contract; an entry that would land behind it is dropped and *overflow set, so that a broken count cannot write
// out of bounds (the host reports it: fetch_small).
#define LIVE_DEAD 0xFFFFFFFFu
#define LIVE_ROUNDS (RVB_LIVE_TILE / 64)
#define LIVE_WAVES 4                // tiles (waves) per workgroup of the key and the compaction kernel
static_assert(RVB_LIVE_TILE % 64 == 0, "a wave walks a tile in whole rounds");

struct LiveHeader { uint32_t total, pad_[3]; };          // in front of the tile words (SortBuffers::live)

__device__ __forceinline__ uint32_t lanes_below(const unsigned long long mask)
{
    return __builtin_amdgcn_mbcnt_hi((uint32_t) (mask >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t) mask, 0u));
}

// HRTF: both ears' raw keys from one pass, ear 1's at n + the impulse's number, as bin_keys_hrtf_kernel keys them.
template <bool HRTF>
__global__ __launch_bounds__(64 * LIVE_WAVES) void live_keys_kernel(ModelDev m, const rvb_impulse * __restrict__ diffuse, uint64_t ndiffuse,
                                                                    const rvb_impulse * __restrict__ images, uint64_t n, float predelay,
                                                                    float sample_rate, uint32_t nbins, uint32_t * __restrict__ raw,
                                                                    uint32_t * __restrict__ tile_counts)
{
    const uint32_t lane = threadIdx.x & 63u;
    const uint64_t wave = (uint64_t) __builtin_amdgcn_readfirstlane((int) (threadIdx.x >> 6));
    const uint64_t ntiles = (n + RVB_LIVE_TILE - 1) / RVB_LIVE_TILE;
    for (uint64_t tile = (uint64_t) blockIdx.x * LIVE_WAVES + wave; tile < ntiles; tile += (uint64_t) gridDim.x * LIVE_WAVES) {
        uint32_t live = 0;
#pragma unroll 4
        for (uint32_t r = 0; r < LIVE_ROUNDS; ++r) {
            const uint64_t j = tile * RVB_LIVE_TILE + r * 64u + lane;
            const uint64_t jj = j < n ? j : n - 1;            // (behind the end: the last impulse again, its verdict dropped)
            const float4 * rec = reinterpret_cast<const float4 *>(jj < ndiffuse ? diffuse + jj : images + (jj - ndiffuse));
            const float4 v0 = rec[0], v1 = rec[1], p = rec[2];
            const float time = rec[3].x;
            const bool nonzero = j < n && ANY_VOLUME(v0, v1);
            if (j < n) {
                const v3 pos = mk3(p.x, p.y, p.z);
                if (HRTF) {
                    raw[j] = nonzero ? min(time_bin(hrtf_time(m, 0, pos, time), predelay, sample_rate), nbins) : LIVE_DEAD;
                    raw[n + j] = nonzero ? nbins + 1u + min(time_bin(hrtf_time(m, 1, pos, time), predelay, sample_rate), nbins) : LIVE_DEAD;
                } else {
                    raw[j] = nonzero ? min(time_bin(time, predelay, sample_rate), nbins) : LIVE_DEAD;      // speaker channels keep the input time
                }
            }
            live += (uint32_t) __popcll(__ballot(nonzero));
        }
        if (lane == 0) tile_counts[tile] = live;
    }
}

// (Four waves, not sixteen: in the pipeline, beside the other contexts' path kernels, a workgroup of 1024 waited 0.7 ms for a CU with
// room for all of its waves at once.)
#define LIVE_OFFSET_THREADS 256
__global__ __launch_bounds__(LIVE_OFFSET_THREADS) void live_offsets_kernel(uint32_t * __restrict__ tiles, uint64_t ntiles, LiveHeader * __restrict__ head)
{
    __shared__ uint32_t wave_sums[LIVE_OFFSET_THREADS / 64];
    const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
    // a run of consecutive tiles per lane
    const uint64_t per = (ntiles + LIVE_OFFSET_THREADS - 1) / LIVE_OFFSET_THREADS;
    const uint64_t first = (uint64_t) threadIdx.x * per < ntiles ? (uint64_t) threadIdx.x * per : ntiles, last = first + per < ntiles ? first + per : ntiles;
    uint32_t sum = 0;
    for (uint64_t k = first; k < last; ++k) sum += tiles[k];
    uint32_t upto = sum;                                       // ... through this lane, within the wave
    for (int off = 1; off < 64; off <<= 1) {
        const uint32_t below = (uint32_t) __shfl_up((int) upto, off);
        if (lane >= (uint32_t) off) upto += below;
    }
    if (lane == 63u) wave_sums[wave] = upto;
    __syncthreads();
    uint32_t at = upto - sum;
    for (uint32_t w = 0; w < wave; ++w) at += wave_sums[w];
    for (uint64_t k = first; k < last; ++k) {
        const uint32_t count = tiles[k];
        tiles[k] = at;
        at += count;
    }
    if (threadIdx.x == LIVE_OFFSET_THREADS - 1u) head->total = at;          // (the last lane's run ends with the last tile)
}

template <bool HRTF>
__global__ __launch_bounds__(64 * LIVE_WAVES) void live_compact_kernel(const uint32_t * __restrict__ raw, uint64_t n,
                                                                       const uint32_t * __restrict__ tile_starts,
                                                                       const LiveHeader * __restrict__ head, uint64_t listed, uint32_t nbins,
                                                                       uint32_t * __restrict__ keys, uint32_t * __restrict__ values,
                                                                       uint32_t * overflow)
{
    const uint32_t lane = threadIdx.x & 63u;
    const uint64_t wave = (uint64_t) __builtin_amdgcn_readfirstlane((int) (threadIdx.x >> 6));
    const uint64_t ntiles = (n + RVB_LIVE_TILE - 1) / RVB_LIVE_TILE;
    for (uint64_t tile = (uint64_t) blockIdx.x * LIVE_WAVES + wave; tile < ntiles; tile += (uint64_t) gridDim.x * LIVE_WAVES) {
        uint64_t at = tile_starts[tile];
#pragma unroll 4
        for (uint32_t r = 0; r < LIVE_ROUNDS; ++r) {
            const uint64_t j = tile * RVB_LIVE_TILE + r * 64u + lane;
            const uint32_t key = j < n ? raw[j] : LIVE_DEAD;
            const bool live = key != LIVE_DEAD;
            const unsigned long long mask = __ballot(live);
            if (live) {
                const uint64_t to = at + lanes_below(mask);
                if (to < listed) {
                    keys[to] = key;
                    values[to] = (uint32_t) j;
                    if (HRTF) {
                        keys[listed + to] = raw[n + j];
                        values[listed + to] = (uint32_t) j;
                    }
                } else {
                    *overflow = 1u;
                }
            }
            at += (uint64_t) __popcll(mask);
        }
    }
    // the rest of the list: entries that match no bin (sorted last, never gathered)
    const uint64_t total = head->total < listed ? head->total : listed;
    for (uint64_t k = total + (uint64_t) blockIdx.x * blockDim.x + threadIdx.x; k < listed; k += (uint64_t) gridDim.x * blockDim.x) {
        keys[k] = nbins;
        values[k] = 0u;
        if (HRTF) {
            keys[listed + k] = 2u * nbins + 1u;
            values[listed + k] = 0u;
        }
    }
}

// Where each bin's run starts in the sorted key list: starts[key] = first position of that key (entries of absent keys keep
// the caller's 0xFFFFFFFF fill).  One coalesced pass over the keys replaces a 23-step binary search per bin — 19 M dependent
// random reads at workload C2, which made the summation kernel fetch 3 GB for 0.5 GB of impulses.
// shift > 0: the list is ordered on key >> shift only (sort_and_bin), and starts / ends are those of key >> shift, "coarse bins".
// Entries whose whole key is >= nbins count for nothing, and they may stand anywhere in the last coarse bin's run (a live impulse
// behind the histogram's end keeps its place among the others; the list's sentinel tail follows them all): the run reaches from its
// first entry below nbins to behind its last one, taken with atomicMin / atomicMax over every entry that has no such neighbour in
// its run (ends pre-filled with 0).  A coarse bin with no entry below nbins keeps starts = 0xFFFFFFFF.
__global__ __launch_bounds__(256) void bin_starts_kernel(const uint32_t * __restrict__ keys, uint64_t n, uint64_t nbins, uint32_t shift,
                                                         uint32_t * __restrict__ starts, uint32_t * __restrict__ ends)
{
    for (uint64_t k = (uint64_t) blockIdx.x * blockDim.x + threadIdx.x; k < n; k += (uint64_t) gridDim.x * blockDim.x) {
        const uint32_t key = keys[k];
        if (key >= nbins)
            continue;
        if (shift) {
            const uint32_t run = key >> shift;
            const uint32_t before = k == 0 ? 0xFFFFFFFFu : keys[k - 1], after = k + 1 == n ? 0xFFFFFFFFu : keys[k + 1];
            if (before >= nbins || (before >> shift) != run)
                atomicMin(starts + run, (uint32_t) k);
            if (after >= nbins || (after >> shift) != run)
                atomicMax(ends + run, (uint32_t) (k + 1));
            continue;
        }
        if (k == 0 || keys[k - 1] != key)
            starts[key] = (uint32_t) k;
        if (k + 1 == n || keys[k + 1] != key)     // (with both ends known the summation loop has no data-dependent exit: its gathers overlap)
            ends[key] = (uint32_t) (k + 1);
    }
}

// One lane per bin: add the bin's impulses in impulse order (the order of rayverb.cpp:67-74) ON TOP of what the histogram
// holds (the caller zeroes it; a second context that continues the fold with the next ray shard starts from the first one's
// sums, so the chain reproduces the serial order over all shards).  Speaker channels keep the input time (kernel.cpp:530-533)
// and share the bin, so ONE sorted list serves NCH channels of the speaker model (first_channel .. first_channel + NCH - 1);
// the two ears of the HRTF model have their own bins (NCH = 1, one list per ear).
// TWO lanes per bin — the even lane folds bands 0-3, the odd lane bands 4-7 (each reads its 16-byte half of the volume; both
// read the position) — so the gather of 8 M scattered 64-byte records has twice the loads in flight per bin.
// (Runs of neighbouring bins for the eight-apart workgroups of one XCD were measured and rejected: profiles/r04_ordered_sum_xcd_n1.txt.)
template <bool HRTF, int NCH>
__global__ __launch_bounds__(64) void ordered_sum_kernel(ModelDev m, uint32_t first_channel, const rvb_impulse * __restrict__ diffuse,
                                                         uint64_t ndiffuse, const rvb_impulse * __restrict__ images,
                                                         const uint32_t * __restrict__ values,
                                                         const uint32_t * __restrict__ starts, const uint32_t * __restrict__ ends,
                                                         uint64_t nbins, uint64_t bin_begin, uint64_t bin_end, float * __restrict__ hist)
{
    // (bins [bin_begin, bin_end) of this launch: the caller may fold the histogram bin range by bin range, each range leaving for
    // the host as soon as it is final — rvb_ir_accumulate_export)
    const uint64_t t = (uint64_t) blockIdx.x * blockDim.x + threadIdx.x;
    const uint64_t bin = bin_begin + (t >> 1);
    const uint32_t half = (uint32_t) t & 1u;
    if (bin >= bin_end)
        return;
    const uint64_t lo = starts[bin];
    if (lo == 0xFFFFFFFFull)
        return;                               // nothing lands in this bin: the histogram keeps what it holds
    float sum[NCH][4];
#pragma unroll
    for (int c = 0; c < NCH; ++c)
#pragma unroll
        for (int b = 0; b < 4; ++b)
            sum[c][b] = hist[hist_row(first_channel + c, half, b, nbins) + bin];
    const uint64_t hi = ends[bin];
    for (uint64_t k = lo; k < hi; k += SUM_UNROLL) {          // the adds stay in impulse order
        float4 v[SUM_UNROLL], p[SUM_UNROLL];
        gather_records<SUM_UNROLL>(values, k, lo, hi, diffuse, ndiffuse, images, half, v, p);
#pragma unroll
        for (int u = 0; u < SUM_UNROLL; ++u) {
            if (k + u >= hi) break;
            const float vol[4] = {v[u].x, v[u].y, v[u].z, v[u].w};
            const v3 pos = mk3(p[u].x, p[u].y, p[u].z);      // (keyed into a bin: the volume is non-zero)
            if (HRTF) {
                const float * tb = m.table + ((uint64_t) first_channel * RVB_HRTF_ROWS + (uint64_t) hrtf_row(m, pos)) * 8 + half * 4;
#pragma unroll
                for (int b = 0; b < 4; ++b) sum[0][b] += vol[b] * tb[b];
            } else {
#pragma unroll
                for (int c = 0; c < NCH; ++c) {
                    const float g = speaker_gain(m, first_channel + c, pos);
#pragma unroll
                    for (int b = 0; b < 4; ++b) sum[c][b] += vol[b] * g;
                }
            }
        }
    }
#pragma unroll
    for (int c = 0; c < NCH; ++c)
#pragma unroll
        for (int b = 0; b < 4; ++b)
            hist[hist_row(first_channel + c, half, b, nbins) + bin] = sum[c][b];
}

// The speaker fold over a list ordered by coarse bin only (sort_and_bin with RVB_COARSE_SHIFT: one radix pass less at workload C2).
// A wave owns one coarse bin, the run [starts, ends) of its RVB_COARSE_BINS = 32 bins; lane pair p owns bin 32 * coarse + p, the even
// lane bands 0-3 and the odd lane bands 4-7 as in ordered_sum_kernel.  The wave walks the run in rounds of COARSE_CHUNK = 64 entries:
//   * every lane holds one entry: its key and value come with one coalesced load each, its 64-byte record with the lane's own gather
//     (64 records in flight per wave; the next round's keys, values and records are requested before this round's are consumed);
//   * the lane evaluates the record's channel gains — once per record and channel, not once per lane of a pair — and leaves volume
//     and gains in LDS; an entry that no bin of this launch matches (a key at or past nbins or outside [bin_begin, bin_end)) is
//     neither gathered nor stored;
//   * behind a workgroup barrier (one wave: the LDS writes of the producer lanes are done before a consumer lane reads), each pair
//     takes the positions of the round's entries with its bin's key as a ballot mask and adds them lowest position first.
// Why the sums are bit for bit ordered_sum_kernel<false, NCH>'s: the list goes into a stable sort in impulse order, so within the
// run the entries of one bin stand in impulse order, and rounds and mask bits are taken in list order; the gain is speaker_gain of
// attenuation.h on the same record position and channel; the add is the same `sum[c][b] += vol[b] * g` (one multiply, one add, no
// contraction) on top of what the histogram holds; nothing else touches a value, and a bin without entries is not written.
// A second barrier ends the round: the next round's producers overwrite the LDS.
#define COARSE_CHUNK 64
static_assert(COARSE_CHUNK == 64 && RVB_COARSE_BINS * 2 == 64, "an entry per lane, a lane pair per bin");
template <int NCH>
__global__ __launch_bounds__(64)       // LDS per wave: 64 x (32 + 4 NCH) bytes — 2.5 KiB at two channels, 3 KiB at four
void ordered_sum_coarse_kernel(ModelDev m, uint32_t first_channel, const rvb_impulse * __restrict__ diffuse, uint64_t ndiffuse,
                               const rvb_impulse * __restrict__ images, const uint32_t * __restrict__ keys,
                               const uint32_t * __restrict__ values, const uint32_t * __restrict__ starts,
                               const uint32_t * __restrict__ ends, uint64_t nbins, uint64_t bin_begin, uint64_t bin_end,
                               float * __restrict__ hist)
{
    __shared__ float4 s_vol[COARSE_CHUNK][2];
    __shared__ float s_gain[COARSE_CHUNK][NCH];
    const uint32_t lane = threadIdx.x;
    const uint64_t coarse = (bin_begin >> RVB_COARSE_SHIFT) + blockIdx.x;
    const uint64_t lo = starts[coarse];
    if (lo == 0xFFFFFFFFull)
        return;                               // nothing lands in these bins: the histogram keeps what it holds (the whole wave leaves)
    const uint64_t hi = ends[coarse];
    const uint32_t half = lane & 1u, pair = lane >> 1;
    const uint32_t first_bin = (uint32_t) (coarse << RVB_COARSE_SHIFT);
    const uint64_t bin = (uint64_t) first_bin + pair;
    const bool mine = bin >= bin_begin && bin < bin_end;          // (bin_end <= nbins: fold_range)
    float sum[NCH][4];
#pragma unroll
    for (int c = 0; c < NCH; ++c)
#pragma unroll
        for (int b = 0; b < 4; ++b)
            sum[c][b] = mine ? hist[hist_row(first_channel + c, half, b, nbins) + bin] : 0.0f;
    bool touched = false;

    // the lane's entry of a round: its key (0xFFFFFFFF behind the run) and value, then its record where a bin of this launch takes it
    uint32_t key, value, next_key, next_value;
    float4 v0, v1, p;
#define COARSE_ENTRY(K, KEY, VALUE) do { const uint64_t at_ = (K) + lane; const bool in_ = at_ < hi; \
                                         KEY = in_ ? keys[at_] : 0xFFFFFFFFu; VALUE = in_ ? values[at_] : 0u; } while (0)
#define COARSE_TAKEN(KEY) ((KEY) >= bin_begin && (KEY) < bin_end)
#define COARSE_GATHER() do { if (COARSE_TAKEN(key)) { \
                                 const float4 * r_ = reinterpret_cast<const float4 *>(value < ndiffuse ? diffuse + value : images + (value - ndiffuse)); \
                                 v0 = r_[0]; v1 = r_[1]; p = r_[2]; } } while (0)
    v0 = v1 = p = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
    COARSE_ENTRY(lo, key, value);
    COARSE_GATHER();
    COARSE_ENTRY(lo + COARSE_CHUNK, next_key, next_value);
    for (uint64_t k = lo; k < hi; k += COARSE_CHUNK) {
        const bool taken = COARSE_TAKEN(key);
        const uint32_t slot = taken ? key - first_bin : 0xFFFFFFFFu;      // which pair's bin: 0 .. 31
        if (taken) {
            s_vol[lane][0] = v0;
            s_vol[lane][1] = v1;
            const v3 pos = mk3(p.x, p.y, p.z);                  // (keyed into a bin: the volume is non-zero)
#pragma unroll
            for (int c = 0; c < NCH; ++c)
                s_gain[lane][c] = speaker_gain(m, first_channel + c, pos);
        }
        key = next_key;
        value = next_value;
        COARSE_GATHER();
        COARSE_ENTRY(k + 2 * COARSE_CHUNK, next_key, next_value);
        __syncthreads();
        unsigned long long todo = 0;
#pragma unroll
        for (uint32_t q = 0; q < RVB_COARSE_BINS; ++q) {
            const unsigned long long holders = __ballot(slot == q);
            if (pair == q) todo = holders;
        }
        if (!mine) todo = 0;
        while (todo) {                                           // the adds stay in impulse order
            const uint32_t e = (uint32_t) __ffsll((long long) todo) - 1u;
            todo &= todo - 1;
            const float4 v = s_vol[e][half];
            const float vol[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
            for (int c = 0; c < NCH; ++c) {
                const float g = s_gain[e][c];
#pragma unroll
                for (int b = 0; b < 4; ++b) sum[c][b] += vol[b] * g;
            }
            touched = true;
        }
        __syncthreads();
    }
#undef COARSE_ENTRY
#undef COARSE_TAKEN
#undef COARSE_GATHER
    if (touched) {
#pragma unroll
        for (int c = 0; c < NCH; ++c)
#pragma unroll
            for (int b = 0; b < 4; ++b)
                hist[hist_row(first_channel + c, half, b, nbins) + bin] = sum[c][b];
    }
}

// The HRTF model's ordered sum, both ears in ONE launch over the combined list of bin_keys_hrtf_kernel: two lanes per (bin, ear) —
// the even lane folds bands 0-3 and evaluates the azimuth, the odd lane bands 4-7 and the elevation (hrtf_row_quad: one atan2 per
// lane and impulse instead of two, the binary32 one unless the integer part of an angle is in doubt).
__global__ __launch_bounds__(RVB_HRTF_SUM_THREADS) void ordered_sum_hrtf_kernel(ModelDev m, const rvb_impulse * __restrict__ diffuse, uint64_t ndiffuse,
                                                              const rvb_impulse * __restrict__ images, const uint32_t * __restrict__ values,
                                                              const uint32_t * __restrict__ starts, const uint32_t * __restrict__ ends,
                                                              uint64_t nbins, uint64_t bin_begin, uint64_t bin_end, float * __restrict__ hist)
{
    const uint64_t t = (uint64_t) blockIdx.x * blockDim.x + threadIdx.x;
    // (bin, ear) in bin-major order: a workgroup folds BOTH ears of a run of neighbouring bins.  The two ears' times differ by at
    // most 0.29 ms (13 bins at 44.1 kHz), so the impulses of ear 1's bin b are those of ear 0's bins b-13 .. b+13: gathered by the
    // same workgroup, or its neighbour, at about the same time, the second gather of a record finds it in cache (with all of ear 0's
    // bins first and ear 1's after them every record was fetched from HBM twice).
    const uint64_t slot = 2 * bin_begin + (t >> 1);          // bins [bin_begin, bin_end) of this launch
    const uint32_t half = (uint32_t) t & 1u;
    if (slot >= 2 * bin_end)
        return;
    const uint32_t ear = (uint32_t) slot & 1u;
    const uint64_t bin = slot >> 1;
    const uint64_t key = (uint64_t) ear * (nbins + 1) + bin;
    const uint64_t lo = starts[key];
    if (lo == 0xFFFFFFFFull)
        return;                               // nothing lands in this bin: the histogram keeps what it holds (both lanes of the pair leave)
    float sum[4];                             // (the row index written out: through hist_row the code of this kernel changes)
#pragma unroll
    for (int b = 0; b < 4; ++b)
        sum[b] = hist[((uint64_t) ear * 8 + half * 4 + b) * nbins + bin];
    const uint64_t hi = ends[key];
    const float * table = m.table + (uint64_t) ear * RVB_HRTF_ROWS * 8 + half * 4;
    for (uint64_t k = lo; k < hi; k += SUM_UNROLL) {
        float4 v[SUM_UNROLL], p[SUM_UNROLL];
        gather_records<SUM_UNROLL>(values, k, lo, hi, diffuse, ndiffuse, images, half, v, p);
#pragma unroll
        for (int u = 0; u < SUM_UNROLL; ++u) {
            if (k + u >= hi) break;           // (the two lanes of a bin agree: the DPP exchange below always finds its partner)
            const float4 tb = *reinterpret_cast<const float4 *>(table + (uint64_t) hrtf_row_quad(m, mk3(p[u].x, p[u].y, p[u].z), half) * 8);
            sum[0] += v[u].x * tb.x;
            sum[1] += v[u].y * tb.y;
            sum[2] += v[u].z * tb.z;
            sum[3] += v[u].w * tb.w;
        }
    }
#pragma unroll
    for (int b = 0; b < 4; ++b)
        hist[((uint64_t) ear * 8 + half * 4 + b) * nbins + bin] = sum[b];
}

// The fold for speaker layouts of more than 8 channels (up to RVB_MAX_SPEAKERS).  ordered_sum_kernel carries its speakers as kernel
// arguments (ModelDev) and folds at most four channels per launch, so a wider layout would gather every scattered 64-byte record once
// per four channels.  Here the speaker table sits in device memory (AttenuationModel::speaker_table: normalised direction +
// coefficient, 16 bytes per channel) and ONE launch folds all channels of a bin range:
//   * a workgroup owns WIDE_BINS = 32 consecutive bins, two lanes per bin as in ordered_sum_kernel, so every [channel][band] row is
//     written in 128-byte runs;
//   * the workgroup's waves take NCH consecutive channels each and walk the SAME bins' lists at the same time: the first wave to ask
//     for a record brings it in from HBM, the others find it in the CU's L1 or the XCD's L2;
//   * what does not depend on the channel is evaluated once per record: the two normalisations of (pos - mic), with the operations
//     of speaker_gain on the same operands, and the non-zero test (made when the record was keyed: only live records are listed);
//   * a wave's table entries are wave-uniform and read through the scalar cache; the NCH x 4 sums per lane stay in registers.
// The sums are the left-to-right float sums in impulse order on top of what the histogram holds: bit for bit what
// ordered_sum_kernel<false, N> leaves in the same rows.
template <int NCH>
__global__ __launch_bounds__(64 * WIDE_MAX_WAVES) void ordered_sum_wide_kernel(v3 mic, const float4 * __restrict__ speakers, uint32_t nchannels,
                                                                               const rvb_impulse * __restrict__ diffuse, uint64_t ndiffuse,
                                                                               const rvb_impulse * __restrict__ images,
                                                                               const uint32_t * __restrict__ values,
                                                                               const uint32_t * __restrict__ starts, const uint32_t * __restrict__ ends,
                                                                               uint64_t nbins, uint64_t bin_begin, uint64_t bin_end, float * __restrict__ hist)
{
    // channels [c0, c0 + NCH) of this wave; those at or past nchannels (the last wave's tail) are computed on a copy of the last
    // speaker and never loaded or stored
    const uint32_t c0 = (uint32_t) __builtin_amdgcn_readfirstlane((int) (threadIdx.x >> 6)) * NCH;
    const uint32_t lane = threadIdx.x & 63u;
    const uint32_t half = lane & 1u;
    const uint64_t bin = bin_begin + (uint64_t) blockIdx.x * WIDE_BINS + (lane >> 1);
    if (bin >= bin_end)
        return;
    const uint64_t lo = starts[bin];
    if (lo == 0xFFFFFFFFull)
        return;                               // nothing lands in this bin: the histogram keeps what it holds
    const uint64_t hi = ends[bin];
    float4 spk[NCH];
    float sum[NCH][4];
#pragma unroll
    for (int c = 0; c < NCH; ++c) {
        const uint32_t ch = c0 + c < nchannels ? c0 + c : nchannels - 1;
        spk[c] = speakers[ch];
#pragma unroll
        for (int b = 0; b < 4; ++b)
            sum[c][b] = c0 + c < nchannels ? hist[hist_row(c0 + c, half, b, nbins) + bin] : 0.0f;
    }
    for (uint64_t k = lo; k < hi; k += SUM_UNROLL) {
        float4 v[SUM_UNROLL], p[SUM_UNROLL];
        gather_records<SUM_UNROLL>(values, k, lo, hi, diffuse, ndiffuse, images, half, v, p);
#pragma unroll
        for (int u = 0; u < SUM_UNROLL; ++u) {
            if (k + u >= hi) break;
            const float vol[4] = {v[u].x, v[u].y, v[u].z, v[u].w};
            // reference kernel.cpp:528 getDirection, then :511 normalises the unit vector again — once per record, not per channel
            const v3 direction = normalize3(mk3(p[u].x, p[u].y, p[u].z) - mic);
            const v3 unit = normalize3(direction);
#pragma unroll
            for (int c = 0; c < NCH; ++c) {
                const float g = (1 - spk[c].w) + spk[c].w * dot3(unit, mk3(spk[c].x, spk[c].y, spk[c].z));
#pragma unroll
                for (int b = 0; b < 4; ++b) sum[c][b] += vol[b] * g;
            }
        }
    }
#pragma unroll
    for (int c = 0; c < NCH; ++c) {
        if (c0 + c < nchannels) {
#pragma unroll
            for (int b = 0; b < 4; ++b)
                hist[hist_row(c0 + c, half, b, nbins) + bin] = sum[c][b];
        }
    }
}

// Channels per wave: 12 where that needs no more waves than 16 would (9-12, 17-24, 33-36 channels: fewer idle channel slots in the
// last wave, 2-6 % faster at workload C2), else 16.  A fifth wave costs far more than idle slots do: 56 channels as 5 x 12 took 2.34 ms,
// as 4 x 16 1.70 ms (profiles/speaker_arrays_n1.txt).
uint32_t wide_channels_per_wave(uint32_t nchannels)
{
    return (nchannels + 11) / 12 <= (nchannels + 15) / 16 ? 12u : 16u;
}

__global__ __launch_bounds__(256) void flat_keys_kernel(const rvb_attenuated_impulse * __restrict__ in, uint64_t n, float sample_rate,
                                                        uint32_t * __restrict__ keys, uint32_t * __restrict__ values,
                                                        uint32_t * max_time_bits)
{
    float tmax = 0.0f;
    for (uint64_t i = (uint64_t) blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (uint64_t) gridDim.x * blockDim.x) {
        const float4 * r = reinterpret_cast<const float4 *>(in + i);
        const float4 v0 = r[0], v1 = r[1];
        const float t = r[2].x;
        tmax = fmaxf(tmax, t);                 // MAX_SAMPLE counts every impulse (rayverb.cpp:54-57)
        // an all-zero volume adds nothing to its bin (x + 0 = x): keyed past every bin, so that the many {0, 0} entries of an
        // attenuated array (quirk Q2) do not pile up on the one lane that owns bin 0
        const bool nonzero = ANY_VOLUME(v0, v1);
        keys[i] = nonzero ? (uint32_t) roundf(t * sample_rate) : 0xFFFFFFFFu;
        values[i] = (uint32_t) i;
    }
    for (int off = 32; off > 0; off >>= 1)
        tmax = fmaxf(tmax, __shfl_xor(tmax, off));
    if ((threadIdx.x & 63u) == 0 && __float_as_uint(tmax) > *(const volatile uint32_t *) max_time_bits)
        atomicMax(max_time_bits, __float_as_uint(tmax));     // only a wave that can still raise the maximum pays for the atomic
}

__global__ __launch_bounds__(64) void flat_ordered_sum_kernel(const rvb_attenuated_impulse * __restrict__ in,
                                                              const uint32_t * __restrict__ keys, const uint32_t * __restrict__ values,
                                                              const uint32_t * __restrict__ starts,
                                                              uint64_t n, uint64_t nbins, float * __restrict__ out)
{
    const uint64_t bin = (uint64_t) blockIdx.x * blockDim.x + threadIdx.x;
    if (bin >= nbins)
        return;
    const uint64_t lo = starts[bin] == 0xFFFFFFFFu ? n : starts[bin];
    float sum[8] = {0, 0, 0, 0, 0, 0, 0, 0};
    for (uint64_t k = lo; k < n && keys[k] == (uint32_t) bin; ++k) {
        const float4 * r = reinterpret_cast<const float4 *>(in + values[k]);
        const float4 v0 = r[0], v1 = r[1];
        sum[0] += v0.x; sum[1] += v0.y; sum[2] += v0.z; sum[3] += v0.w;
        sum[4] += v1.x; sum[5] += v1.y; sum[6] += v1.z; sum[7] += v1.w;
    }
    for (int b = 0; b < 8; ++b)
        out[(uint64_t) b * nbins + bin] = sum[b];
}

// The bins [bin_begin, bin_end) a fold is asked for, cut to the histogram's; false: none left, nothing to launch.
bool fold_range(uint64_t nbins, uint64_t bin_begin, uint64_t & bin_end)
{
    bin_end = std::min(bin_end, nbins);
    return bin_begin < bin_end;
}

}  // namespace

void rvb_launch_bin_keys(const AttenuationModel & m, uint32_t channel, const rvb_impulse * in, uint64_t n, uint64_t index_base,
                         float predelay, float sample_rate, uint32_t sentinel, uint32_t * keys, uint32_t * values, hipStream_t s)
{
    if (n == 0) return;
    hipLaunchKernelGGL(bin_keys_kernel, dim3(stream_blocks(n, 256)), dim3(256), 0, s, make_model(m), channel, in, n,
                       index_base, predelay, sample_rate, sentinel, keys, values);
}

void rvb_launch_bin_keys_hrtf(const AttenuationModel & m, const rvb_impulse * in, uint64_t count, uint64_t index_base, uint64_t n,
                              float predelay, float sample_rate, uint32_t nbins, uint32_t * keys, uint32_t * values, hipStream_t s)
{
    if (count == 0) return;
    hipLaunchKernelGGL(bin_keys_hrtf_kernel, dim3(stream_blocks(count, 256)), dim3(256), 0, s, make_model(m), in, count, index_base, n,
                       predelay, sample_rate, nbins, keys, values);
}

void rvb_launch_bin_starts(const uint32_t * sorted_keys, uint64_t n, uint64_t nbins, uint32_t * starts, uint32_t * ends, hipStream_t s, int shift)
{
    if (n == 0) return;
    hipLaunchKernelGGL(bin_starts_kernel, dim3(stream_blocks(n, 256)), dim3(256), 0, s, sorted_keys, n, nbins, (uint32_t) shift, starts, ends);
}

size_t rvb_live_scratch_bytes(uint64_t n)
{
    return sizeof(LiveHeader) + (size_t) ((n + RVB_LIVE_TILE - 1) / RVB_LIVE_TILE) * sizeof(uint32_t);
}

void rvb_launch_live_list(const AttenuationModel & m, const rvb_impulse * diffuse, uint64_t ndiffuse, const rvb_impulse * images, uint64_t n,
                          float predelay, float sample_rate, uint32_t nbins, uint64_t listed, uint32_t * raw, void * scratch,
                          uint32_t * keys, uint32_t * values, uint32_t * overflow, hipStream_t s)
{
    if (n == 0) return;
    LiveHeader * head = static_cast<LiveHeader *>(scratch);
    uint32_t * tiles = reinterpret_cast<uint32_t *>(head + 1);
    const uint64_t ntiles = (n + RVB_LIVE_TILE - 1) / RVB_LIVE_TILE;
    const dim3 grid(stream_blocks(ntiles, LIVE_WAVES)), block(64 * LIVE_WAVES);
    const ModelDev md = make_model(m);
    if (m.hrtf) {
        hipLaunchKernelGGL(live_keys_kernel<true>, grid, block, 0, s, md, diffuse, ndiffuse, images, n, predelay, sample_rate, nbins, raw, tiles);
        hipLaunchKernelGGL(live_offsets_kernel, dim3(1), dim3(LIVE_OFFSET_THREADS), 0, s, tiles, ntiles, head);
        hipLaunchKernelGGL(live_compact_kernel<true>, grid, block, 0, s, raw, n, tiles, head, listed, nbins, keys, values, overflow);
    } else {
        hipLaunchKernelGGL(live_keys_kernel<false>, grid, block, 0, s, md, diffuse, ndiffuse, images, n, predelay, sample_rate, nbins, raw, tiles);
        hipLaunchKernelGGL(live_offsets_kernel, dim3(1), dim3(LIVE_OFFSET_THREADS), 0, s, tiles, ntiles, head);
        hipLaunchKernelGGL(live_compact_kernel<false>, grid, block, 0, s, raw, n, tiles, head, listed, nbins, keys, values, overflow);
    }
}

void rvb_launch_ordered_sum(const AttenuationModel & m, uint32_t first_channel, uint32_t nchannels, const rvb_impulse * diffuse,
                            uint64_t ndiffuse, const rvb_impulse * images,
                            const uint32_t * sorted_values, const uint32_t * starts, const uint32_t * ends, uint64_t n,
                            uint64_t nbins, float * hist, hipStream_t s, uint64_t bin_begin, uint64_t bin_end, const uint32_t * coarse_keys)
{
    if (!fold_range(nbins, bin_begin, bin_end) || n == 0) return;
    const bool coarse = coarse_keys != nullptr && !m.hrtf;
    // two lanes per bin; by coarse bin: a wave for each one that [bin_begin, bin_end) cuts
    const dim3 grid(coarse ? (unsigned) (((bin_end - 1) >> RVB_COARSE_SHIFT) - (bin_begin >> RVB_COARSE_SHIFT) + 1)
                           : (unsigned) ((2 * (bin_end - bin_begin) + 63) / 64)), block(64);
    const ModelDev md = make_model(m);
#define RVB_SUM(HRTF, NCH) do { if (coarse) hipLaunchKernelGGL((ordered_sum_coarse_kernel<NCH>), grid, block, 0, s, md, first_channel, diffuse, ndiffuse, \
                                                               images, coarse_keys, sorted_values, starts, ends, nbins, bin_begin, bin_end, hist); \
                                else hipLaunchKernelGGL((ordered_sum_kernel<HRTF, NCH>), grid, block, 0, s, md, first_channel, diffuse, ndiffuse, \
                                                        images, sorted_values, starts, ends, nbins, bin_begin, bin_end, hist); } while (0)
    if (m.hrtf) { RVB_SUM(true, 1); return; }
    switch (nchannels) {                       // speaker channels of one sorted list
    case 1: RVB_SUM(false, 1); break;
    case 2: RVB_SUM(false, 2); break;
    case 3: RVB_SUM(false, 3); break;
    case 4: RVB_SUM(false, 4); break;
    default:                                   // more than four: in groups (64 accumulators per lane would spill)
        for (uint32_t c = 0; c < nchannels; c += 4) {
            const uint32_t k = nchannels - c < 4 ? nchannels - c : 4;
            rvb_launch_ordered_sum(m, first_channel + c, k, diffuse, ndiffuse, images, sorted_values, starts, ends, n, nbins, hist, s, bin_begin, bin_end,
                                   coarse_keys);
        }
    }
#undef RVB_SUM
}

void rvb_launch_ordered_sum_hrtf(const AttenuationModel & m, const rvb_impulse * diffuse, uint64_t ndiffuse, const rvb_impulse * images,
                                 const uint32_t * sorted_values, const uint32_t * starts, const uint32_t * ends, uint64_t nbins, float * hist,
                                 hipStream_t s, uint64_t bin_begin, uint64_t bin_end)
{
    if (!fold_range(nbins, bin_begin, bin_end)) return;
    const dim3 grid((unsigned) ((4 * (bin_end - bin_begin) + RVB_HRTF_SUM_THREADS - 1) / RVB_HRTF_SUM_THREADS));      // two lanes per (bin, ear)
    hipLaunchKernelGGL(ordered_sum_hrtf_kernel, grid, dim3(RVB_HRTF_SUM_THREADS), 0, s, make_model(m), diffuse, ndiffuse,
                       images, sorted_values, starts, ends, nbins, bin_begin, bin_end, hist);
}

void rvb_make_speaker_table(const rvb_speaker * speakers, uint64_t nspeakers, float4 * table)
{
    for (uint64_t i = 0; i < nspeakers; ++i)
        table[i] = speaker_device_form(speakers[i]);
}

void rvb_launch_ordered_sum_wide(const AttenuationModel & m, const rvb_impulse * diffuse, uint64_t ndiffuse, const rvb_impulse * images,
                                 const uint32_t * sorted_values, const uint32_t * starts, const uint32_t * ends, uint64_t n,
                                 uint64_t nbins, float * hist, hipStream_t s, uint64_t bin_begin, uint64_t bin_end)
{
    if (!fold_range(nbins, bin_begin, bin_end) || n == 0 || m.nchannels == 0 || !m.speaker_table) return;
    const uint32_t per_wave = wide_channels_per_wave(m.nchannels);
    const uint32_t waves = (m.nchannels + per_wave - 1) / per_wave;        // <= WIDE_MAX_WAVES for nchannels <= RVB_MAX_SPEAKERS
    const dim3 grid((unsigned) ((bin_end - bin_begin + WIDE_BINS - 1) / WIDE_BINS)), block(64 * waves);
    const v3 mic = mk3(m.mic[0], m.mic[1], m.mic[2]);
    if (per_wave == 12)
        hipLaunchKernelGGL(ordered_sum_wide_kernel<12>, grid, block, 0, s, mic, m.speaker_table, m.nchannels, diffuse, ndiffuse, images,
                           sorted_values, starts, ends, nbins, bin_begin, bin_end, hist);
    else
        hipLaunchKernelGGL(ordered_sum_wide_kernel<16>, grid, block, 0, s, mic, m.speaker_table, m.nchannels, diffuse, ndiffuse, images,
                           sorted_values, starts, ends, nbins, bin_begin, bin_end, hist);
}

void rvb_launch_flat_keys(const rvb_attenuated_impulse * in, uint64_t n, float sample_rate, uint32_t * keys, uint32_t * values,
                          uint32_t * max_time_bits, hipStream_t s)
{
    if (n == 0) return;
    hipLaunchKernelGGL(flat_keys_kernel, dim3(stream_blocks(n, 256)), dim3(256), 0, s, in, n, sample_rate, keys, values, max_time_bits);
}

void rvb_launch_flat_ordered_sum(const rvb_attenuated_impulse * in, const uint32_t * sorted_keys, const uint32_t * sorted_values,
                                 const uint32_t * starts, uint64_t n, uint64_t nbins, float * out, hipStream_t s)
{
    if (nbins == 0) return;
    hipLaunchKernelGGL(flat_ordered_sum_kernel, dim3((unsigned) ((nbins + 63) / 64)), dim3(64), 0, s, in, sorted_keys,
                       sorted_values, starts, n, nbins, out);
}
