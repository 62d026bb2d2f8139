/* rvb_capi_images.h — the image sources of a kept trace on the device: the merged image list without the host, and the image-source
 * part of the material gradient.  An extension of rvb_capi.h (which it includes and whose types, codes and conventions it uses),
 * exported by the same librvb_hip.so; rvb_capi.h itself is unchanged by it.  No reference counterpart.
 *
 * WHY.  The fitting chain (rvb_keep_paths, rvb_reshade, rvb_ir_accumulate, rvb_decay_params_loss, rvb_reshade_grad) sees the diffuse
 * records only, while clarity, definition and early decay time are decided by the direct sound and the first specular reflections.
 * Two things were missing: a forward path for an RVB_IR_ALL histogram that stays on the device across re-shades, and the gradient of
 * the image part.  Both are here; python: capi.Context.ir_configure_speakers_merged / reshade_grad_images, fitting.py which=IR_ALL.
 */
#ifndef RVB_CAPI_IMAGES_H
#define RVB_CAPI_IMAGES_H

#include "rvb_capi.h"

#ifdef __cplusplus
extern "C" {
#endif

struct rvb_ctx;                   /* the context of rvb_capi.h: every call here works on one */

/* ---- the merged image list on the device (csrc/images.hip, csrc/image_grad_kernels.hip) --------------------------------------------
 * rvb_reshade rewrites the candidates' volumes in device memory, but an RVB_IR_ALL histogram then still needs the candidates on the
 * host, rvb_merge_images there and rvb_ir_configure_speakers with the merged array: once per material set and per line-search trial.
 * Which candidate wins each key of the merge depends on geometry and microphone only, never on materials.
 *
 * CONTRACT.  The context is left exactly as rvb_ir_configure_speakers / rvb_ir_configure_hrtf would leave it with images = what
 * rvb_merge_images makes of the selected pair's candidates (rvb_get_image_candidates), the pair's direct impulse (rvb_get_direct) and
 * remove_direct: the same impulses in the same (std::map key) order.  Every later rvb_ir_time_range*, rvb_ir_accumulate*,
 * rvb_ir_exact_* and rvb_ir_download returns the same bytes.  *nimages (may be NULL) receives the length of the list.  All refusals and
 * voiding rules of those two calls apply with the same codes — nothing traced, which outside 1..3, the speaker count, table == NULL
 * without an earlier table; rvb_reshade, rvb_relisten, rvb_ir_select_pair and a new trace void the configuration —, and so does the
 * synchronisation before the image buffer grows.
 * MECHANISM.  The winner list has one entry per output impulse: the device position of the candidate it is copied from, or a mark for
 * the pair's direct slot.  The host makes it with the merge rule of rvb_merge_images itself (one shared function) from ONE download of
 * the candidates in device order, once per (trace or relisten, pair, remove_direct); it is cached in the context and uploaded once.
 * "image_gather_kernel" (rvb_last_timings; one lane per image, whole 16-byte chunks) then copies the impulses into the context's image
 * list in stream order.  Everything that voids a trace voids the cache: a trace, rvb_relisten, rvb_set_scene, rvb_share_scene,
 * rvb_set_directions*.  rvb_reshade, the source setters and rvb_ir_select_pair do NOT (the list of another pair replaces it when that
 * pair is configured): after a re-shade the call costs the gather alone, no download and no host merge.  The list needs no kept trace.
 * The host copy of the list that rvb_ir_time_range scans under the speaker model is fetched from the device by its first reader. */
int rvb_ir_configure_speakers_merged(rvb_ctx * ctx, const float mic[3], const rvb_speaker * speakers, uint64_t nspeakers,
                                     int which, int remove_direct, uint64_t * nimages);
int rvb_ir_configure_hrtf_merged(rvb_ctx * ctx, const float mic[3], const float * table, const float facing[3], const float up[3],
                                 int which, int remove_direct, uint64_t * nimages);

/* ---- the image-source part of the material gradient (csrc/image_grad_kernels.hip) --------------------------------------------------
 * THE QUANTITY.  L_img = sum over the images i of the current configuration, the channels c and the bands b of
 *     w[c][b][bin_i] * speaker_gain_c(i) * volume_b(i),
 * skipping images whose bin time_bin(time_i, predelay, sample_rate) is >= nbins: what rvb_ir_accumulate with RVB_IR_FAST adds for the
 * image part.  w has the histogram's layout [nchannels][8][nbins] (device memory) and is read in place.  L of an RVB_IR_ALL
 * configuration is a sum over impulses, so the caller ADDS this call's result to rvb_reshade_grad's (taken under an RVB_IR_DIFFUSE
 * configuration with the same w); which == RVB_IR_IMAGES and RVB_IR_ALL return the same bytes here.  The result is taken at the table,
 * the air and the source directivity that the records reflect now.
 * Image i comes from candidate (ray, slot s): its chain is the surfaces s_0 .. s_{s-2} of the ray's first bounces, D_i its kept
 * INIT_DIST, gamma_b(i) its source gain (v = mic - position; 1 without directivity), and
 *     alpha_{i,b} = (air_attenuation(D_i, air_b) * 1.0f) * gamma_b(i) * sum_c w[c][b][bin_i] gain_c(i).  Then
 *     grad_surfaces[s].specular[b] = sum_i sum_{k: s_k = s} (-1) * alpha_{i,b} * prod_{j != k} (-specular[s_j][b])
 *     grad_air[b]                  = sum_i (prod_j -specular[s_j][b]) * alpha_{i,b} * D_i * ln((float) M_E)
 *   - prefix and suffix products, never a division: a coefficient that is 0 still gets its derivative;
 *   - the direct slot has an empty chain: it adds to grad_air and nowhere else; a hidden direct path (negative kept distance) adds nothing;
 *   - grad_surfaces[s].diffuse[b] is exactly +0.0 everywhere (images never read a diffuse coefficient), and a surface on no live
 *     image's chain gets exactly 0 in all 16 entries;
 *   - terms in binary32 with the trace's own functions in the re-shade's order; sums in binary64 in an order fixed by (position in the
 *     merged list, chain position) and the launch shape, no atomics, rounded to float once: two calls return identical bytes.
 * SCOPE of this version.  RVB_ERR_INVALID, before any device is touched: NULL ctx, d_weights or grad_surfaces; nbins 0 or >= 2^32; a
 * predelay or sample rate that is not finite.  RVB_ERR_STATE, with a text that names the condition: nothing traced (or the scene or the
 * directions changed since); the last trace made without rvb_keep_paths; no IR configuration (a re-shade and a relisten void it:
 * configure again); a configuration made by rvb_ir_configure_speakers or rvb_ir_configure_hrtf, "the caller's list has lost its
 * chains"; the HRTF model; which == RVB_IR_DIFFUSE; more than 8 channels.  The per-triangle map (rvb_reshade_grad_map), rvb_multi_* and
 * rvb_pipeline_* are out of scope: none of them offers the merged list or this gradient.
 * CALLING.  Synchronous: waits for the context's stream and fills the host arrays (grad_surfaces: the scene's nsurfaces entries;
 * grad_air may be NULL).  Changes no byte of the records, the candidates, the direct slot, the time range, the sort buffers or the
 * accumulation scratch; the configuration stays and so does a prepared exact list.  A failed call writes nothing.  rvb_last_timings:
 * "reshade_grad_images_kernel" (one lane per image, at most eight chain steps, a term row per image), "reshade_grad_images_reduce_kernel"
 * (a workgroup per surface, the fixed-order fold).
 * MEASURED on one MI355X, 100 k rays, stereo speakers, 44.1 kHz (profiles/early_fit_n1.txt, tools/early_fit_bench.py; medians of 21
 * repetitions in one process, [min .. max]).  One RVB_IR_ALL forward evaluation, rvb_reshade + configure + rvb_ir_accumulate with
 * RVB_IR_EXACT, to rvb_synchronize:
 *     the constructed room of tests/image_edges.py, 100 k x 12, 158 293 candidates -> 725 images, 12 520 bins: through the host merge
 *     28.24 ms [27.78 .. 29.10], of which its configure step (candidates down, sort, map, upload) 27.80 ms; through the merged call
 *     27.36 ms on the first call, which makes the list, and 0.597 ms [0.581 .. 0.644] on later calls (configure step 0.067 ms): 47 x.
 *     the 75 k-triangle cathedral, 100 k x 128, 24 candidates -> 14 images, 846 741 bins: 1.501 ms [1.490 .. 1.536] through the host
 *     merge, 1.517 ms first call, 1.427 ms [1.411 .. 1.446] later calls (configure step 0.642 -> 0.014 ms): 1.05 x, 0.074 ms against a
 *     spread of 0.046 ms — a room of large smooth walls has few image sources, and the evaluation is the re-shade and the exact
 *     binning of 12.8 M diffuse records.
 * The gradient: rvb_reshade_grad_images 0.116 ms in the room (reshade_grad_images_kernel 0.030 ms, reshade_grad_images_reduce_kernel
 *     0.016 ms; the rest is the synchronisation and the copy of the result) beside rvb_reshade_grad 0.269 ms; 0.075 ms in the cathedral
 *     (0.025 + 0.007 ms) beside 1.608 ms.  Latency-bound, as expected of a few hundred rows.
 * Against a build of the parent commit in processes that take turns (3 turns, 63 samples each, cathedral): rvb_trace with keeping on
 *     4.800 against 4.797 ms (the parent's own spread 0.172 ms), rvb_reshade 0.626 against 0.627 ms (0.049), rvb_reshade_grad 1.593
 *     against 1.595 ms (0.042): inside the spread, their device code is unchanged.
 * Accuracy: over every case of tests/test_gpu_reshade_grad_images.py the largest |gpu - reference| is 0.038 of the derived bar
 *     4 (9 + 16) 2^-24 A. */
int rvb_reshade_grad_images(rvb_ctx * ctx, float predelay, float sample_rate, uint64_t nbins, const void * d_weights,
                            rvb_surface * grad_surfaces, float grad_air[8]);

#ifdef __cplusplus
}
#endif
#endif
