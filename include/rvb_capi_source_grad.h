/* rvb_capi_source_grad.h — source-end gradients of a weighted impulse response from a kept trace: how a loss changes when the source is
 * turned or its directivity changes.  An extension of rvb_capi.h (which it includes and whose types, codes and conventions it uses),
 * exported by the same librvb_hip.so; rvb_capi.h itself is unchanged by it.  No reference counterpart.
 *
 * WHY.  The kept-trace family (rvb_reshade, rvb_reshade_grad, rvb_reshade_grad_map, rvb_reshade_grad_images of rvb_capi_images.h, with the
 * losses of rvb_decay_*, rvb_decay_params_loss and rvb_mtf_adjoint of rvb_capi_speech.h) answers "what if the walls were different".
 * A PA designer asks the other question: where to aim the loudspeaker, and with which pattern, to raise the speech transmission index
 * over the seats.  rvb_reshade applies a newly set directivity to a kept trace without retracing, but a search over directions then costs
 * a re-shade, a binning and an analysis per trial, with no gradient.  H is linear in the source gain of every ray, so everything the
 * gradient needs is in the context already.  python: capi.Context.source_grad / source_grad_images, directivity.balloon_gradient,
 * fitting.source_gradient, aim_loss_and_grad, fit_aim, sti_source_balloon.
 */
#ifndef RVB_CAPI_SOURCE_GRAD_H
#define RVB_CAPI_SOURCE_GRAD_H

#include "rvb_capi.h"

#ifdef __cplusplus
extern "C" {
#endif

struct rvb_ctx;                   /* the context of rvb_capi.h: every call here works on one */

/* dL/dshape[b] of the polar pattern's eight shapes and dL/ddirection[j] of its direction.  direction is the derivative with respect to the
 * unit vector n of the pattern TAKEN AS A FREE 3-VECTOR: the caller who keeps n a unit vector projects it onto the tangent plane,
 * t = direction - dot(direction, n) n.  direction[3] = 0. */
typedef struct { float shape[8]; float direction[4]; } rvb_source_pattern_grad;

/* ---- the gradients (csrc/source_grad.hip, csrc/source_grad_kernels.hip) ------------------------------------------------------------
 * THE QUANTITY.  L = sum w * H, exactly the L of rvb_reshade_grad (rvb_source_grad: the diffuse records) and of rvb_reshade_grad_images
 * (rvb_source_grad_images: the merged image list): the same H, the same weights [nchannels][8][nbins] in device memory, the same
 * selected pair, the table and the air that the records reflect now.  H is taken as the polynomial that rvb_reshade's ARITHMETIC writes
 * down: the source gain g_b(r) of ray r is a factor of every diffuse record of that ray, gamma_b(i) a factor of image i.
 *   d_ray_grad[r][b] = dL/dg_b(r) = sum over the bounces k of ray r, in bounce order, of the binary32 term
 *       t_k = (P_k * ((air_attenuation(dist_k, air_b) * DIFF(k)) * u_k)) * diffuse[s_k][b],   u_k = sum_c w[c][b][bin_k] * gain_c(k),
 *     P_k = prod_{j<=k} -specular[s_j][b]; u_k is formed as rvb_reshade_grad forms it, 0 for an invisible record and for a bin >= nbins:
 *     rvb_reshade_grad's P_k a_k with the pattern factor left out, times the diffuse coefficient.  The call never divides by a gain and
 *     never reads a record's stored (already scaled) volume: a ray at a null of the pattern still has its derivative.  The terms are added
 *     in binary64 and rounded to float once.  Every entry is written; a ray that escapes before its first hit, or has no live record,
 *     gets exactly 0.
 *   d_image_grad[i][b] = dL/dgamma_b(i) = (prod_j -specular[s_j][b]) * (air_attenuation(D_i, air_b) * 1.0f) * sum_c w[c][b][bin_i] gain_c(i),
 *     in the order of rvb_reshade_grad_images' products, i the position in the merged list.  A hidden direct path and an image past the
 *     histogram get exactly 0.  d_image_depart[i] = normalize3(normalize3(mic - position_i)), w = 0: the departure unit vector the gain uses.
 *   pattern_grad, for the polar pattern (n, shape) that the records reflect now for the selected pair: with v the ray's own direction
 *     (images: mic - position, as the pattern's CONTRACT says), u = normalize3(normalize3(v)) and d = dot3(u, n) in binary32 exactly as
 *     the gain takes them, and Lambda_b the binary64 sum above BEFORE its rounding,
 *       shape[b]     = sum over rays (images) of Lambda_b * (d - 1)
 *       direction[j] = sum over rays (images) of (sum_b shape_b * Lambda_b) * u_j
 *     with products and sums in binary64: one partial per tile of 256 rays (images) from a fixed tree, the tiles combined in a fixed
 *     order, no atomics, rounded to float once.
 *   d_ray_rows[r], d_image_rows[i]: the table row in 0 .. 64800 that the source table selects for the ray or image under the orientation
 *     the records reflect now (64800: the zero row behind the table).  There is no fold by row on the device — a [64800][8] result is no
 *     smaller than [nrays][8] —: directivity.balloon_gradient adds the rows up.
 * Two calls return identical bytes.
 * REFUSALS, each with a text that names its condition, each before any device is touched; a failed call writes nothing.  Those of
 * rvb_reshade_grad (rvb_source_grad) and of rvb_reshade_grad_images (rvb_source_grad_images) with the same codes — RVB_ERR_INVALID: NULL
 * ctx or d_weights, nbins 0 or >= 2^32, a predelay or sample rate that is not finite; RVB_ERR_STATE: nothing traced, no kept trace, no IR
 * configuration, the HRTF model, more than 8 channels, which != RVB_IR_DIFFUSE (rvb_source_grad), which == RVB_IR_DIFFUSE or a
 * configuration that was not made by rvb_ir_configure_speakers_merged (rvb_source_grad_images); RVB_ERR_CAPACITY: more than 2048
 * reflections (rvb_source_grad), 2^27 surfaces —, and in addition RVB_ERR_INVALID for a device output that overlaps d_weights,
 * RVB_ERR_STATE for a rows output when the records reflect no source table and for pattern_grad when they reflect no polar pattern.
 * Every output may be NULL; a call with none checks and computes nothing it has to store.
 * CALLING.  Synchronous, like rvb_reshade_grad.  The calls change no byte of the records, the candidates, the direct slot, the time range,
 * the IR configuration or a prepared exact list; rvb_source_grad_images also leaves the sort buffers and the accumulation scratch as they
 * were, rvb_source_grad uses the accumulation scratch for the transposed weights as rvb_reshade_grad does.  They work after rvb_reshade,
 * after rvb_relisten and for pair p of rvb_trace_pairs (rvb_ir_select_pair).  Their scratch lives with the kept buffers: rvb_keep_paths(ctx, 0)
 * frees it.  rvb_last_timings: "reshade_grad_weights_kernel", "source_grad_rays_kernel" (the forward sweep of rvb_reshade_grad's kernel:
 * eight rays per wave, one lane per (ray, band), tiles of 16 bounces; no table in LDS, no backward sweep), "source_grad_images_kernel" (one
 * lane per image), "source_grad_pattern_kernel", "source_grad_pattern_fold_kernel".
 * OUT OF SCOPE: the HRTF model, more than 8 channels, rvb_multi_* and rvb_pipeline_*, a fold per table cell on the device, and derivatives
 * with respect to the source POSITION — the paths depend on it, so it needs a retrace.
 * d_image_depart is written as whole 16-byte vectors: it must be 16-byte aligned (any device allocation is).
 * MEASURED on one MI355X, 100 k rays x 128 in the 75 k-triangle cathedral, stereo speakers, 44.1 kHz, 846 741 bins, 14 images, a polar
 * pattern on the source (profiles/source_grad_n1.txt, tools/source_grad_bench.py; medians of 21 repetitions in one process, [min .. max]):
 *     rvb_source_grad with d_ray_grad and pattern_grad 0.871 ms [0.865 .. 0.887]: source_grad_rays_kernel 0.754 ms [0.751 .. 0.765],
 *     reshade_grad_weights_kernel 0.034 ms, source_grad_pattern_kernel 0.008 ms, source_grad_pattern_fold_kernel 0.006 ms; with d_ray_grad
 *     alone 0.819 ms.  Beside it in the same run rvb_reshade_grad 1.578 ms [1.567 .. 1.592], reshade_grad_kernel 1.480 ms: the new sweep
 *     takes 0.51 of it.  Its floor — 12.8 M records x (16 B side record + 32 B of the record) + 54 MB of weights = 669 MB once at 6.6 TB/s —
 *     is 0.101 ms: the kernel stands 7.45 x above it.  What bounds it was not measured; the weight gathers and the serial chain of a
 *     lane are the suspects, as for the sweep it is cut from.  rvb_source_grad_images, everything asked for: 0.105 ms [0.103 .. 0.151]
 *     (source_grad_images_kernel 0.024 ms; the rest is the synchronisation and the copy of the result).
 *     One aim-gradient evaluation of the STI loss (fitting.aim_loss_and_grad, RVB_IR_ALL) 3.718 ms [3.668 .. 3.849] against 2.241 ms
 *     [2.203 .. 2.299] for one loss evaluation: central differences cost 8.96 ms for the direction alone (2.4 x) and 44.8 ms for direction
 *     and eight shapes (12.1 x).
 * Against a build of the parent commit in processes that take turns (3 turns, 63 samples each): rvb_trace with keeping on 4.822 against
 *     4.811 ms (the parent's own spread 0.137 ms), rvb_reshade 0.627 against 0.625 ms (0.043), rvb_reshade_grad 1.587 against 1.585 ms
 *     (0.053): inside the spread, their device code is unchanged.
 * Accuracy: over every case of tests/test_gpu_source_grad.py the largest |gpu - reference| is 0.057 of the derived bar
 *     4 (nreflections + 16) 2^-24 A (0.003 of it for the pattern gradients).
 * Not measured: hardware counters (no counter run was made), other tile sizes or launch shapes, other ray counts, more than one GPU. */
int rvb_source_grad(rvb_ctx * ctx, float predelay, float sample_rate, uint64_t nbins, const void * d_weights,
                    void * d_ray_grad   /* device float [nrays][8], may be NULL */,
                    void * d_ray_rows   /* device uint32 [nrays], may be NULL; RVB_ERR_STATE unless the records reflect a source table */,
                    rvb_source_pattern_grad * pattern_grad /* host, may be NULL; RVB_ERR_STATE unless the records reflect a polar pattern */);

int rvb_source_grad_images(rvb_ctx * ctx, float predelay, float sample_rate, uint64_t nbins, const void * d_weights,
                           void * d_image_grad   /* device float [nimages][8], merged-list order, may be NULL */,
                           void * d_image_depart /* device float [nimages][4]: the departure unit vector the gain uses, may be NULL */,
                           void * d_image_rows   /* device uint32 [nimages], may be NULL; table only */,
                           rvb_source_pattern_grad * pattern_grad /* host, may be NULL; pattern only */);

#ifdef __cplusplus
}
#endif
#endif
