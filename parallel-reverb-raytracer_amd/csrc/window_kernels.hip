// window_kernels.hip — the echo finder's kernels (include/rvb_capi_window.h): the score pass over the records, the exact radix select
// over the 4-byte keys it leaves (the arithmetic is csrc/window_select.h, shared with the host and replayed by tests/cpp/window_select.cpp),
// the gather and the sort of the at most RVB_WINDOW_MAX_PATHS winners, and the walk back along the rays of the listed paths.
//
//   window_score_kernel       a workgroup of 256 lanes takes tiles of RVB_WINDOW_TILE records, four lanes per record and one per 16-byte
//                             chunk (a wave's load is 1 KiB in a row): the two volume chunks and the time chunk of each, the key out.
//                             Counts the window and digit 0 of the keys in LDS, then adds what it counted to the state and to table 0.
//   window_histogram_kernel   digit 1, 2 of the keys that agree with the threshold so far; digit 0, 1, 2 of ~record of the ties at the
//                             threshold key (these three return at once unless the record number has to decide).  16 bytes of keys per load.
//   window_walk_kernel        one workgroup: lane t adds up its 8 (4) buckets, the lane in whose buckets the places run out walks them
//                             (window_select::walk) and moves the state on.
//   window_gather_kernel      every key whose composite is at or above the threshold takes a slot of the list.  The slots are handed out
//                             by an integer atomic, so the list's order is arbitrary; its content is not.
//   window_sort_kernel        one workgroup of 1024 lanes: the list in LDS, a bitonic sort by descending composite, entry e out.
//   window_paths_kernel       one wave per listed path, lanes over bounces.
// Integer atomics only, and only for counts.  A kernel boundary is the only synchronisation between workgroups.
#include "kernels.h"
#include "window_select.h"

#include <cstddef>

namespace {

namespace ws = window_select;

constexpr uint32_t kLanes = 256;
constexpr uint32_t kTile = RVB_WINDOW_TILE;
constexpr uint32_t kChunkLoads = kTile * 4 / kLanes;    // 16-byte chunks of a tile per lane of the score pass
constexpr uint32_t kKeyChunk = kLanes * 4 * 4;          // keys per workgroup step of the key passes: four 16-byte loads per lane
constexpr uint32_t kMaxGroups = 2048;                   // workgroups of a streaming launch: each adds its counts to the tables once
static_assert(kTile % kLanes == 0 && kTile % 64 == 0 && kChunkLoads % 2 == 0, "a tile is whole waves, its chunks two rounds of loads");
static_assert(RVB_WINDOW_MAX_PATHS == 1024, "window_sort_kernel sorts one entry per lane of a 1024-lane workgroup");

// the scratch block (rvb_window_scratch_bytes): [State 32 B][gathered 4 B][pad to 64][tables 6 x 2048 words][list 1024 x 8 B]
// [entries 1024 x 16 B][keys: a word per record, padded to whole 16-byte loads]
constexpr size_t kGatheredAt = sizeof(ws::State);
constexpr size_t kTablesAt = 64;
constexpr size_t kTablesBytes = (size_t) 2 * ws::kPasses * ws::kMaxBuckets * sizeof(uint32_t);
constexpr size_t kListAt = kTablesAt + kTablesBytes;
constexpr size_t kEntriesAt = kListAt + (size_t) RVB_WINDOW_MAX_PATHS * sizeof(uint64_t);
constexpr size_t kKeysAt = kEntriesAt + (size_t) RVB_WINDOW_MAX_PATHS * sizeof(rvb_window_entry);
static_assert(sizeof(ws::State) == 32 && kGatheredAt + 4 <= kTablesAt && kKeysAt % 16 == 0, "scratch layout");

struct Scratch {
    ws::State * state;
    uint32_t * gathered;
    uint32_t * tables;          // [6][2048]
    uint64_t * list;
    rvb_window_entry * entries;
    uint32_t * keys;
    __host__ __device__ explicit Scratch(void * p)
    {
        char * c = static_cast<char *>(p);
        state = reinterpret_cast<ws::State *>(c);
        gathered = reinterpret_cast<uint32_t *>(c + kGatheredAt);
        tables = reinterpret_cast<uint32_t *>(c + kTablesAt);
        list = reinterpret_cast<uint64_t *>(c + kListAt);
        entries = reinterpret_cast<rvb_window_entry *>(c + kEntriesAt);
        keys = reinterpret_cast<uint32_t *>(c + kKeysAt);
    }
    __host__ __device__ uint32_t * table(uint32_t pass) const { return tables + (size_t) pass * ws::kMaxBuckets; }
};

// the score of include/rvb_capi_window.h: one binary32 operation per operator, in this order (the unit is compiled with -ffp-contract=off)
// four bands of it on top of `score`
__device__ __forceinline__ float window_score4(float score, const float (&v)[4], const float (&w)[4])
{
#pragma unroll
    for (int b = 0; b < 4; ++b) {
        const float x = w[b] * v[b];
        score = score + x * x;
    }
    return score;
}

// what a workgroup counted in LDS added to a table of the scratch: one atomic per bucket that is not empty
__device__ __forceinline__ void flush_table(const uint32_t * counts, uint32_t buckets, uint32_t * table)
{
    for (uint32_t b = threadIdx.x; b < buckets; b += kLanes) {
        const uint32_t c = counts[b];
        if (c) atomicAdd(table + b, c);
    }
}

__global__ __launch_bounds__(kLanes) void window_score_kernel(const rvb_impulse * __restrict__ in, uint64_t n, float t_begin, float t_end,
                                                              WindowWeights weights, void * scratch)
{
    __shared__ uint32_t counts[ws::kMaxBuckets];
    __shared__ uint32_t inside;
    const Scratch s(scratch);
    for (uint32_t b = threadIdx.x; b < ws::kMaxBuckets; b += kLanes) counts[b] = 0;
    if (threadIdx.x == 0) inside = 0;
    __syncthreads();
    // Four lanes per record, one per 16-byte chunk: a wave's load is 16 whole records, 1 KiB in a row.  Lane 0 of a record adds up bands
    // 0..3, lane 1 goes on from there with bands 4..7 (the sum keeps its order), lane 3 holds the time; the position chunk is not read.
    const uint64_t ntiles = (n + kTile - 1) / kTile;
    const uint32_t part = threadIdx.x & 3u, quad = (threadIdx.x & 63u) & ~3u;
    float w[4];
#pragma unroll
    for (int b = 0; b < 4; ++b) w[b] = part == 1 ? weights.w[4 + b] : weights.w[b];
    uint32_t mine = 0;
    for (uint64_t tile = blockIdx.x; tile < ntiles; tile += gridDim.x) {
        const float4 * chunks = reinterpret_cast<const float4 *>(in + tile * kTile);
        for (uint32_t half = 0; half < 2; ++half) {
            float4 chunk[kChunkLoads / 2];
#pragma unroll
            for (uint32_t i = 0; i < kChunkLoads / 2; ++i) {
                const uint32_t c = (half * (kChunkLoads / 2) + i) * kLanes + threadIdx.x;          // chunk of the tile
                chunk[i] = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
                if (part != 2 && tile * kTile + c / 4 < n) chunk[i] = chunks[c];
            }
#pragma unroll
            for (uint32_t i = 0; i < kChunkLoads / 2; ++i) {
                const uint32_t c = (half * (kChunkLoads / 2) + i) * kLanes + threadIdx.x;
                const uint64_t r = tile * kTile + c / 4;
                const float v[4] = {chunk[i].x, chunk[i].y, chunk[i].z, chunk[i].w};
                const float before = __shfl(part == 0 ? window_score4(0.0f, v, w) : 0.0f, quad, 64);     // bands 0..3, from lane 0 of the record
                const float score = window_score4(before, v, w);                                       // lane 1: ... and bands 4..7
                const float time = __shfl(chunk[i].x, quad + 3, 64);
                if (part == 1 && r < n) {
                    const bool in_window = t_begin <= time && time < t_end && score > 0.0f;
                    const uint32_t key = in_window ? __float_as_uint(score) : 0u;
                    s.keys[r] = key;
                    if (in_window) {
                        ++mine;
                        atomicAdd(&counts[ws::digit_of(key, 0)], 1u);
                    }
                }
            }
        }
    }
    if (mine) atomicAdd(&inside, mine);
    __syncthreads();
    flush_table(counts, ws::digit_buckets(0), s.table(0));
    if (threadIdx.x == 0 && inside) atomicAdd(&s.state->in_window, inside);
}

// pass 1, 2: a digit of the key; 3, 4, 5: digit 0, 1, 2 of ~record among the ties
__global__ __launch_bounds__(kLanes) void window_histogram_kernel(uint32_t pass, uint64_t n, void * scratch)
{
    __shared__ uint32_t counts[ws::kMaxBuckets];
    const Scratch s(scratch);
    const ws::State st = *s.state;
    const bool by_record = pass >= ws::kPasses;
    const uint32_t digit = by_record ? pass - ws::kPasses : pass;
    if (st.want == 0 || (by_record && !ws::record_passes_needed(st))) return;
    for (uint32_t b = threadIdx.x; b < ws::kMaxBuckets; b += kLanes) counts[b] = 0;
    __syncthreads();
    const uint4 * keys4 = reinterpret_cast<const uint4 *>(s.keys);          // (the key array ends on a whole 16 bytes)
    for (uint64_t base = (uint64_t) blockIdx.x * kKeyChunk; base < n; base += (uint64_t) gridDim.x * kKeyChunk) {
#pragma unroll
        for (uint32_t i = 0; i < 4; ++i) {
            const uint64_t r = base + ((uint64_t) i * kLanes + threadIdx.x) * 4;
            if (r >= n) continue;
            const uint4 k4 = keys4[r / 4];
            const uint32_t k[4] = {k4.x, k4.y, k4.z, k4.w};
#pragma unroll
            for (uint32_t j = 0; j < 4; ++j) {
                if (r + j >= n) continue;
                const uint32_t record = (uint32_t) (r + j);
                if (by_record) {
                    if (ws::counts_in_record_pass(st, k[j], record, digit)) atomicAdd(&counts[ws::digit_of(~record, digit)], 1u);
                } else if (ws::counts_in_key_pass(st, k[j], digit)) {
                    atomicAdd(&counts[ws::digit_of(k[j], digit)], 1u);
                }
            }
        }
    }
    __syncthreads();
    flush_table(counts, ws::digit_buckets(digit), s.table(pass));
}

__global__ __launch_bounds__(kLanes) void window_walk_kernel(uint32_t pass, uint64_t max_entries, void * scratch)
{
    __shared__ uint32_t sums[kLanes];
    const Scratch s(scratch);
    ws::State st = *s.state;
    const bool by_record = pass >= ws::kPasses;
    const uint32_t digit = by_record ? pass - ws::kPasses : pass;
    if (pass == 0) ws::begin(st, st.in_window, max_entries);
    if (st.want == 0 || (by_record && !ws::record_passes_needed(st))) {
        __syncthreads();                                                      // (every lane has read the state)
        if (pass == 0 && threadIdx.x == 0) *s.state = st;
        return;
    }
    const uint32_t left = by_record ? ws::record_left(st) : ws::key_left(st);
    const uint32_t per = ws::digit_buckets(digit) / kLanes;                  // 8 or 4 buckets per lane
    const uint32_t * table = s.table(pass) + threadIdx.x * per;
    uint32_t local[ws::kMaxBuckets / kLanes];
    uint32_t sum = 0;
    for (uint32_t i = 0; i < per; ++i) { local[i] = table[i]; sum += local[i]; }
    sums[threadIdx.x] = sum;
    __syncthreads();
    uint32_t before = 0;                                                      // the buckets above this lane's
    for (uint32_t t = threadIdx.x + 1; t < kLanes; ++t) before += sums[t];
    if (before < left && left <= before + sum) {                              // (one lane: the counted keys are at least `left`)
        ws::Walk w = ws::walk(local, per, left - before);
        w.bucket += threadIdx.x * per;
        w.before += before;
        if (by_record) ws::record_walked(st, w, digit);
        else ws::key_walked(st, w, digit);
        *s.state = st;
    }
}

__global__ __launch_bounds__(kLanes) void window_gather_kernel(uint64_t n, void * scratch)
{
    const Scratch s(scratch);
    const ws::State st = *s.state;
    if (st.want == 0) return;
    const uint4 * keys4 = reinterpret_cast<const uint4 *>(s.keys);
    for (uint64_t base = (uint64_t) blockIdx.x * kKeyChunk; base < n; base += (uint64_t) gridDim.x * kKeyChunk) {
#pragma unroll
        for (uint32_t i = 0; i < 4; ++i) {
            const uint64_t r = base + ((uint64_t) i * kLanes + threadIdx.x) * 4;
            if (r >= n) continue;
            const uint4 k4 = keys4[r / 4];
            const uint32_t k[4] = {k4.x, k4.y, k4.z, k4.w};
#pragma unroll
            for (uint32_t j = 0; j < 4; ++j) {
                if (r + j >= n || !ws::listed(st, k[j], (uint32_t) (r + j))) continue;
                const uint32_t slot = atomicAdd(s.gathered, 1u);
                if (slot < RVB_WINDOW_MAX_PATHS) s.list[slot] = ws::composite(k[j], (uint32_t) (r + j));     // (exactly `want` are listed)
            }
        }
    }
}

__global__ __launch_bounds__(RVB_WINDOW_MAX_PATHS) void window_sort_kernel(const rvb_impulse * __restrict__ in, void * scratch,
                                                                           rvb_window_entry * __restrict__ entries)
{
    __shared__ uint64_t c[RVB_WINDOW_MAX_PATHS];
    const Scratch s(scratch);
    const uint32_t want = min(s.state->want, (uint32_t) RVB_WINDOW_MAX_PATHS);
    const uint32_t t = threadIdx.x;
    c[t] = t < want ? s.list[t] : 0ull;                                       // (0 is below every listed composite)
    __syncthreads();
    for (uint32_t k = 2; k <= RVB_WINDOW_MAX_PATHS; k <<= 1) {
        for (uint32_t j = k >> 1; j > 0; j >>= 1) {
            const uint32_t o = t ^ j;
            if (o > t) {
                const uint64_t a = c[t], b = c[o];
                const bool descending = (t & k) == 0;
                if (descending ? a < b : a > b) { c[t] = b; c[o] = a; }
            }
            __syncthreads();
        }
    }
    if (t < want) {
        const uint32_t record = ws::record_of(c[t]);
        rvb_window_entry e;
        e.record = record;
        e.score = __uint_as_float(ws::key_of(c[t]));
        e.time = in[record].time;
        entries[t] = e;
    }
}

__global__ __launch_bounds__(64) void window_paths_kernel(const rvb_impulse * __restrict__ in, const uint2 * __restrict__ listen, uint32_t nreflections,
                                                          uint64_t max_hits, const void * scratch, rvb_window_path * __restrict__ paths,
                                                          rvb_window_hit * __restrict__ hits)
{
    const Scratch s(const_cast<void *>(scratch));
    const uint32_t e = blockIdx.x;
    if (e >= s.state->want) return;
    const rvb_window_entry entry = s.entries[e];
    const uint64_t ray = entry.record / nreflections;
    const uint32_t bounce = (uint32_t) (entry.record % nreflections);
    if (threadIdx.x == 0) {
        const float4 * chunks = reinterpret_cast<const float4 *>(in + entry.record);
        const float4 lo = chunks[0], hi = chunks[1];
        rvb_window_path p;
        p.ray = ray;
        p.bounce = bounce;
        p.nhits = bounce + 1;
        p.score = entry.score;
        p.time = entry.time;
        p.pad_[0] = p.pad_[1] = 0.0f;
        p.volume[0] = lo.x; p.volume[1] = lo.y; p.volume[2] = lo.z; p.volume[3] = lo.w;
        p.volume[4] = hi.x; p.volume[5] = hi.y; p.volume[6] = hi.z; p.volume[7] = hi.w;
        paths[e] = p;
    }
    if (!hits) return;
    const uint64_t stored = min((uint64_t) bounce + 1, max_hits);
    const uint64_t first = ray * nreflections;                                // record (ray, 0) of the pair
    for (uint64_t j = threadIdx.x; j < stored; j += 64) {
        const float4 position = reinterpret_cast<const float4 *>(in + first + j)[2];
        uint4 h;
        h.x = __float_as_uint(position.x);
        h.y = __float_as_uint(position.y);
        h.z = __float_as_uint(position.z);
        h.w = listen[first + j].y;                                            // ListenRecord of kept_tiles.h: {threshold, triangle}
        reinterpret_cast<uint4 *>(hits)[(uint64_t) e * max_hits + j] = h;
    }
}

uint32_t groups_for(uint64_t n, uint32_t per_group)
{
    const uint64_t g = (n + per_group - 1) / per_group;
    return (uint32_t) (g < kMaxGroups ? (g ? g : 1) : kMaxGroups);
}

} // namespace

static_assert(sizeof(rvb_window_entry) == 16 && sizeof(rvb_window_path) == 64 && sizeof(rvb_window_hit) == 16, "include/rvb_capi_window.h");
static_assert(offsetof(rvb_impulse, position) == 32 && offsetof(rvb_impulse, time) == 48, "the chunks of a record");

size_t rvb_window_scratch_bytes(uint64_t n) { return kKeysAt + (size_t) ((n + 3) & ~3ull) * sizeof(uint32_t); }
rvb_window_entry * rvb_window_scratch_entries(void * scratch) { return Scratch(scratch).entries; }
const void * rvb_window_scratch_state(const void * scratch) { return scratch; }

hipError_t rvb_launch_window_begin(void * scratch, hipStream_t s) { return hipMemsetAsync(scratch, 0, kListAt, s); }

void rvb_launch_window_score(const rvb_impulse * in, uint64_t n, float t_begin, float t_end, const WindowWeights & weights, void * scratch, hipStream_t s)
{
    hipLaunchKernelGGL(window_score_kernel, dim3(groups_for(n, kTile)), dim3(kLanes), 0, s, in, n, t_begin, t_end, weights, scratch);
}

void rvb_launch_window_pass(uint32_t pass, uint64_t n, uint64_t max_entries, void * scratch, hipStream_t s)
{
    if (pass != 0) hipLaunchKernelGGL(window_histogram_kernel, dim3(groups_for(n, kKeyChunk)), dim3(kLanes), 0, s, pass, n, scratch);
    hipLaunchKernelGGL(window_walk_kernel, dim3(1), dim3(kLanes), 0, s, pass, max_entries, scratch);
}

void rvb_launch_window_gather(uint64_t n, void * scratch, hipStream_t s)
{
    hipLaunchKernelGGL(window_gather_kernel, dim3(groups_for(n, kKeyChunk)), dim3(kLanes), 0, s, n, scratch);
}

void rvb_launch_window_sort(const rvb_impulse * in, void * scratch, rvb_window_entry * entries, hipStream_t s)
{
    hipLaunchKernelGGL(window_sort_kernel, dim3(1), dim3(RVB_WINDOW_MAX_PATHS), 0, s, in, scratch, entries);
}

void rvb_launch_window_paths(const rvb_impulse * in, const uint2 * listen, uint32_t nreflections, uint64_t max_paths, uint64_t max_hits,
                             const void * scratch, rvb_window_path * paths, rvb_window_hit * hits, hipStream_t s)
{
    hipLaunchKernelGGL(window_paths_kernel, dim3((unsigned) max_paths), dim3(64), 0, s, in, listen, nreflections, max_hits, scratch, paths, hits);
}
