/* rvb_capi_window.h — the echo finder: the strongest diffuse paths behind a time window of a finished trace, found on the device.  An
 * extension of rvb_capi.h (which it includes and whose types, codes and conventions it uses), exported by the same librvb_hip.so;
 * rvb_capi.h itself is unchanged by it.  No reference counterpart.  python: capi.Context.window_select / window_paths, echoes.py.
 *
 * WHY.  Re-shading, a new microphone, the gradients and the decay calls answer "what if" and "which wall".  The first question asked of
 * a finished impulse response is another one: what is this peak — through which sequence of walls did the sound of this window travel?
 * Every record holds its hit point, its arrival time and its eight band volumes, and the listener record of a kept trace names the
 * triangle of every (ray, bounce).  The query is a deterministic top-K over the records and, for the winners, the walk back along the
 * ray; without it the caller copies every record to the host and sorts there.
 */
#ifndef RVB_CAPI_WINDOW_H
#define RVB_CAPI_WINDOW_H

#include "rvb_capi.h"

#ifdef __cplusplus
extern "C" {
#endif

struct rvb_ctx;                   /* the context of rvb_capi.h: every call here works on one */

#define RVB_WINDOW_TILE      1024   /* records per workgroup tile of the score pass; tests choose their edge shapes from it */
#define RVB_WINDOW_MAX_PATHS 1024   /* most entries one call lists */
typedef struct { uint64_t record; float score; float time; } rvb_window_entry;                  /* 16 B */
typedef struct { uint64_t ray; uint32_t bounce; uint32_t nhits; float score; float time;
                 float pad_[2]; float volume[8]; } rvb_window_path;                             /* 64 B */
typedef struct { float position[3]; uint32_t triangle; } rvb_window_hit;                        /* 16 B */

/* ---- the selection on any device array of impulses (csrc/window.hip, csrc/window_kernels.hip, csrc/window_select.h) -----------------
 * THE SCORE of a record, one IEEE binary32 operation per operator in the order written, never a fused multiply-add:
 *     x_b = weights[b] * volume[b];   score = ((((0 + x_0 * x_0) + x_1 * x_1) + ...) + x_7 * x_7).      weights == NULL: eight ones.
 * IN THE WINDOW: t_begin <= time, time < t_end (both binary32 comparisons) and score > 0 — a zero score and a NaN score are outside,
 * +inf is inside.  *in_window receives the number of such records.
 * THE LIST: the min(*in_window, max_entries) records in the window with the highest score, by descending score, equal scores by
 * ascending record number; entry e is {record, score, time} of the e-th.  *count receives its length; entries from *count on are not
 * written.  count and in_window may be NULL.  The result is fixed by this text alone: two calls return identical bytes.
 * MECHANISM.  "window_score_kernel" (the names are those of rvb_last_timings): one streaming pass over the records, which leaves a
 * 4-byte key per record — the score's bit pattern, which orders positive floats as unsigned integers; 0 outside the window —, counts the
 * window and the first digit of the keys.  "window_select_keys": an exact radix select on the composite (key << 32) | ~record, digits of
 * 11, 11 and 10 bits of the key: window_histogram_kernel counts a digit per workgroup in LDS and adds to a small table (integer atomics:
 * the sums do not depend on order), window_walk_kernel finds the threshold's digit.  "window_select_records": the same three digits over
 * the record number, which run only where the ties at the threshold score exceed the places left (the launches stay, their workgroups
 * return at once otherwise).  Every pass reads the keys, never the records.  "window_gather_kernel" collects the at most 1024 composites
 * at or above the threshold; "window_sort_kernel", one workgroup, sorts them in LDS and writes the entries.  No float atomics, no
 * hand-off between workgroups inside a launch.
 * CALLING.  Uses of the context its device, stream, timings and a scratch block of its own (4 bytes per record, grown on demand): no
 * scene and no trace is needed or read, the sort buffers, the accumulation scratch, the IR configuration and a prepared exact list stay.
 * Synchronous: the counts come back.  d_impulses is read on the context's stream.
 * REFUSALS, each with a text that names its condition; a failed call writes nothing.  RVB_ERR_INVALID, before any device is touched:
 * NULL ctx; NULL d_impulses with nimpulses > 0; NULL d_entries; max_entries 0 or above RVB_WINDOW_MAX_PATHS; a t_begin, t_end or weight
 * that is not finite; t_end < t_begin.  RVB_ERR_CAPACITY: 2^32 records or more (record numbers are 32-bit in the selection key).
 * nimpulses == 0 and an empty window (t_end == t_begin) are legal and list nothing. */
int rvb_window_select(rvb_ctx * ctx, const void * d_impulses, uint64_t nimpulses, float t_begin, float t_end,
                      const float weights[8], uint64_t max_entries, void * d_entries, uint64_t * count, uint64_t * in_window);

/* ---- the strongest paths of the selected pair ----------------------------------------------------------------------------------------
 * The same selection over the diffuse records of the selected pair (rvb_ir_select_pair) AS THEY STAND NOW: after a trace, after
 * rvb_reshade, after rvb_relisten, with a source directivity applied.  Entry e, record number n inside the pair, becomes d_paths[e]:
 *     ray = n / nreflections (the index into the array given to rvb_set_directions), bounce = n % nreflections, nhits = bounce + 1,
 *     score and time of the entry, the record's eight volumes unchanged.
 * d_hits, if not NULL, is [max_paths][max_hits] rvb_window_hit: row e receives the first min(nhits, max_hits) hits of the path —
 * position: the position of record (ray, j), bit for bit (the trace writes the intersection point whether or not bounce j sees the
 * microphone); triangle: the listener record's triangle of (ray, j), the caller's index as rvb_reshade_grad_map reads it.  A listed
 * record carries volume, so its ray had not escaped at or before `bounce`: every stored hit is a real hit.  Slots of a row beyond the
 * stored hits, and rows (of d_paths too) from *count on, are not written.
 * d_hits needs a trace kept with RVB_KEEP_LISTENER; d_hits == NULL works on any trace.
 * "window_paths_kernel" follows the kernels above: one wave per listed path, lanes over bounces, a 16-byte position chunk and a 4-byte
 * triangle read and one 16-byte hit stored per lane.
 * STATE.  Synchronous.  Changes no byte of the records, the direct slot, the candidates or the time range; the IR configuration and a
 * prepared exact list stay (rvb_ir_exact_fold still works afterwards); the sort buffers and the accumulation scratch are not touched.
 * REFUSALS as above (max_paths for max_entries, d_paths for d_entries; no d_impulses), and RVB_ERR_INVALID for max_hits == 0 with d_hits
 * given and for d_hits overlapping d_paths; RVB_ERR_CAPACITY for nrays * nreflections >= 2^32 in the pair.  RVB_ERR_STATE: nothing
 * traced, or the scene or the directions changed since; d_hits given and the last trace not kept with RVB_KEEP_LISTENER.
 * OUT OF SCOPE in this version: image sources and the direct sound — their reflection points are not the ray's hit points and would have
 * to be constructed —; rvb_multi_* and rvb_pipeline_* do not offer the calls, like the rest of the kept-trace family.
 * MEASURED on one MI355X, 100 k rays x 128 in the 75 k-triangle cathedral, 12.8 M records of which 8.27 M carry volume, max_hits 128
 * (profiles/window_paths_n1.txt, tools/window_bench.py; medians of 21 repetitions in one process, [min .. max]).  The whole call:
 *     50 ms from the first arrival (57 017 records in the window)    0.314 ms [0.309 .. 0.328] at max_paths 64, 0.326 ms at 1024
 *     [q25, q75) of the live times (4 136 099 in the window)         0.322 ms [0.313 .. 0.328] at 64, 0.330 ms at 1024
 *     the whole response (8 272 199 in the window)                   0.314 ms [0.309 .. 0.326] at 64, 0.330 ms [0.323 .. 0.348] at 1024
 * Its kernels at [q25, q75), 1024 paths: window_score_kernel 0.168 ms, window_select_keys 0.044, window_gather_kernel 0.018,
 *     window_sort_kernel 0.018, window_select_records 0.014 (no ties: the three launches return at once), window_paths_kernel 0.007.
 *     The call is bound by the score pass: 4.9 TB/s of record bytes beside the floor of 819 MB at 6.6 TB/s = 0.124 ms; the size of the
 *     window does not move it.  The kernels add up to 0.26 ms, the rest is the wait and the 32-byte copy of the counts.  No counter run
 *     was made.
 * The same query without these calls, in the same run: torch.topk(1024) over a score tensor made with torch (from a copy of the records
 *     in a torch tensor: torch did not take the library's device pointer as a view) 1.454 ms [1.434 .. 1.461]; rvb_get_diffuse plus
 *     numpy 1 130 ms, of which 16.3 ms are the copy of the records.  The device's list equals the host's, in order.
 * Against a build of the parent commit in processes that take turns (2 turns of 21): rvb_trace with keeping on 4.848 against 4.845 ms
 *     (the parent's own spread 0.118 ms), rvb_reshade 0.619 against 0.621 ms (0.043), rvb_relisten 1.925 against 1.925 ms (0.074):
 *     inside the spread, their device code is unchanged. */
int rvb_window_paths(rvb_ctx * ctx, float t_begin, float t_end, const float weights[8], uint64_t max_paths, uint64_t max_hits,
                     void * d_paths, void * d_hits, uint64_t * count, uint64_t * in_window);

#ifdef __cplusplus
}
#endif

#endif
