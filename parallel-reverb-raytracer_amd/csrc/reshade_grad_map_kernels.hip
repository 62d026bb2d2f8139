// reshade_grad_map_kernels.hip — the fold of rvb_reshade_grad_map (include/rvb_capi.h): material gradients per TRIANGLE from a kept trace.
// The call is three steps.  The terms pass is reshade_grad_kernel itself with another place for a term (reshade_grad_kernels.hip,
// rvb_launch_reshade_grad_map_terms): per record of the pair a row of 16 binary32 terms, and the list (triangle of the record, number of
// the record).  The library's stable sort brings the list into triangle order, every triangle's run in ascending record number (sort.hip,
// sort_and_bin, which also leaves where each run starts and ends).  The fold, here, adds the rows of every run, column by column:
//   reshade_grad_map_fold_kernel      the sorted list cut into tiles of RVB_GRAD_MAP_TILE entries, a workgroup of 256 lanes per tile, the
//                                     tile into 16 segments of 64 entries.  Lane (segment, column) walks its segment in entry order and
//                                     adds terms[value][column] in binary64, run by run: 16 lanes read one 64-byte row.  A run that lies
//                                     inside the segment is complete and is rounded and stored; a run that crosses a segment edge leaves
//                                     a PIECE in LDS.  Then 16 lanes, one per column, walk the segments in order and add the pieces of a
//                                     run one after the other: a run inside the tile is stored, a run that crosses a tile edge leaves the
//                                     tile's partial — slot 0 for the run that holds the tile's first entry, slot 1 for another one that
//                                     holds its last.
//   reshade_grad_map_combine_kernel   lane (triangle, column): 0.0 for a triangle without a run, the partials of a run of several tiles
//                                     added in tile order, rounded once; a run inside one tile has been stored already.
// THE ORDER of a triangle's additions is fixed by the positions of its records in the sorted list alone — inside a segment one after the
// other, a run's segments one after the other, its tiles one after the other —, never by which workgroup ran first: no atomics, no
// flags, identical bytes from call to call.  The work of a lane is bounded by a segment and that of a workgroup by a tile however the
// records spread over the triangles; only the combine walks a long run's tiles, one 8-byte partial per 1024 records.  Nothing here is
// sized by the triangle count but the result itself.
#include "kernels.h"

namespace {

constexpr uint32_t kTile = RVB_GRAD_MAP_TILE;
constexpr uint32_t kLanes = 256;
constexpr uint32_t kColumns = 16;                           // floats of a term row, of a row of the map
constexpr uint32_t kSegments = kLanes / kColumns;
constexpr uint32_t kSegment = kTile / kSegments;            // entries per segment
constexpr uint32_t kAhead = 8;                              // row gathers of a lane in flight together
constexpr uint32_t kNoKey = 0xFFFFFFFFu;                    // what lies before the list and behind it
static_assert(kSegment * kSegments == kTile && kSegment % kAhead == 0, "a tile is 16 segments of whole groups of gathers");

__global__ __launch_bounds__(kLanes) void reshade_grad_map_fold_kernel(const uint32_t * __restrict__ keys, const uint32_t * __restrict__ values, const uint64_t n,
                                                                       const uint32_t ntriangles, const float * __restrict__ terms,
                                                                       double * __restrict__ partials, float * __restrict__ map)
{
    __shared__ uint32_t key_halo[kTile + 2];                // the tile's keys between the key before it and the key behind it
    __shared__ uint32_t val[kTile];
    __shared__ double piece[kSegments][2][kColumns];        // per segment: of the run that holds its first entry, of another that holds its last
    const uint64_t base = (uint64_t) blockIdx.x * kTile;
    const uint32_t count = (uint32_t) min((uint64_t) kTile, n - base);
    for (uint32_t i = threadIdx.x; i < kTile + 2; i += kLanes) {
        const uint64_t e = base + i;                        // (entry e - 1)
        key_halo[i] = e >= 1 && e - 1 < n ? keys[e - 1] : kNoKey;
    }
    for (uint32_t i = threadIdx.x; i < kTile; i += kLanes) val[i] = base + i < n ? values[base + i] : 0u;
    __syncthreads();
    const uint32_t * key = key_halo + 1;                    // key[-1] .. key[count]
    const uint32_t seg = threadIdx.x / kColumns, col = threadIdx.x % kColumns;
    const uint32_t a = seg * kSegment, b = min(a + kSegment, count);
    if (a < b) {
        const bool from_left = key[(int) a - 1] == key[a], to_right = key[b] == key[b - 1];
        double sum = 0.0;
        uint32_t cur = key[a];
        bool first = true;                                  // the run that holds the segment's first entry
        for (uint32_t e0 = a; e0 < b; e0 += kAhead) {
            float x[kAhead];
#pragma unroll
            for (uint32_t u = 0; u < kAhead; ++u) {
                const uint32_t e = e0 + u;
                x[u] = 0.0f;                                // (the run of slots without a record has no rows)
                if (e < b && key[e] < ntriangles && val[e] < n) x[u] = terms[(uint64_t) val[e] * kColumns + col];
            }
#pragma unroll
            for (uint32_t u = 0; u < kAhead; ++u) {
                const uint32_t e = e0 + u;
                if (e >= b) break;
                if (key[e] != cur) {                        // `cur` ends inside the segment
                    if (first && from_left) piece[seg][0][col] = sum;
                    else if (cur < ntriangles) map[(uint64_t) cur * kColumns + col] = (float) sum;
                    first = false;
                    cur = key[e];
                    sum = 0.0;
                }
                sum += (double) x[u];
            }
        }
        if (first ? from_left || to_right : to_right) piece[seg][first ? 0 : 1][col] = sum;
        else if (cur < ntriangles) map[(uint64_t) cur * kColumns + col] = (float) sum;
    }
    __syncthreads();
    if (threadIdx.x >= kColumns) return;
    // the pieces of a run one after the other, segment by segment
    double acc = 0.0;
    bool open = false, from_before = false, has_first = false;      // a run is open; it came from the tile before; it holds the tile's first entry
    for (uint32_t s = 0; s * kSegment < count; ++s) {
        const uint32_t sa = s * kSegment, sb = min(sa + kSegment, count);
        const bool from_left = key[(int) sa - 1] == key[sa], to_right = key[sb] == key[sb - 1], single = key[sa] == key[sb - 1];
        if (from_left || (single && to_right)) {
            const double p = piece[s][0][col];
            if (!open) {                                    // (from_left without an open run: the tile's first segment)
                acc = p;
                open = true;
                from_before = from_left;
                has_first = s == 0;
            } else {
                acc = acc + p;
            }
            if (!(single && to_right)) {                    // the run ends in this segment
                const uint32_t k = key[sa];
                if (from_before) partials[((uint64_t) blockIdx.x * 2u) * kColumns + col] = acc;
                else if (k < ntriangles) map[(uint64_t) k * kColumns + col] = (float) acc;
                open = false;
            }
        }
        if (!single && to_right) {
            acc = piece[s][1][col];
            open = true;
            from_before = false;
            has_first = false;
        }
    }
    if (open) partials[((uint64_t) blockIdx.x * 2u + (has_first ? 0u : 1u)) * kColumns + col] = acc;
}

__global__ __launch_bounds__(kLanes) void reshade_grad_map_combine_kernel(const uint32_t * __restrict__ starts, const uint32_t * __restrict__ ends,
                                                                          const uint32_t ntriangles, const double * __restrict__ partials,
                                                                          float * __restrict__ map)
{
    const uint64_t g = (uint64_t) blockIdx.x * kLanes + threadIdx.x;
    const uint32_t t = (uint32_t) (g / kColumns), col = (uint32_t) (g % kColumns);
    if (t >= ntriangles) return;
    const uint32_t s = starts[t];
    if (s == kNoKey) {                                      // no record on this triangle
        map[g] = 0.0f;
        return;
    }
    const uint32_t t0 = s / kTile, t1 = (ends[t] - 1u) / kTile;
    if (t0 == t1) return;                                   // (stored by the fold)
    // the first tile's partial is its slot 1 unless the run starts with the tile; every later tile's is its slot 0
    double acc = partials[((uint64_t) t0 * 2u + (s % kTile ? 1u : 0u)) * kColumns + col];
    for (uint32_t tile0 = t0 + 1u; tile0 <= t1; tile0 += kAhead) {
        double p[kAhead];
#pragma unroll
        for (uint32_t u = 0; u < kAhead; ++u) p[u] = tile0 + u <= t1 ? partials[((uint64_t) (tile0 + u) * 2u) * kColumns + col] : 0.0;
#pragma unroll
        for (uint32_t u = 0; u < kAhead; ++u)
            if (tile0 + u <= t1) acc = acc + p[u];
    }
    map[g] = (float) acc;
}

}  // namespace

void rvb_launch_reshade_grad_map_fold(const uint32_t * sorted_keys, const uint32_t * sorted_values, uint64_t n, uint32_t ntriangles, const float * terms,
                                      double * partials, float * map, hipStream_t s)
{
    if (n == 0) return;
    hipLaunchKernelGGL(reshade_grad_map_fold_kernel, dim3((unsigned) rvb_grad_map_tiles(n)), dim3(kLanes), 0, s, sorted_keys, sorted_values, n, ntriangles, terms,
                       partials, map);
}

void rvb_launch_reshade_grad_map_combine(const uint32_t * starts, const uint32_t * ends, uint32_t ntriangles, const double * partials, float * map, hipStream_t s)
{
    if (ntriangles == 0) return;
    const uint64_t lanes = (uint64_t) ntriangles * kColumns;
    hipLaunchKernelGGL(reshade_grad_map_combine_kernel, dim3((unsigned) ((lanes + kLanes - 1) / kLanes)), dim3(kLanes), 0, s, starts, ends, ntriangles, partials, map);
}
