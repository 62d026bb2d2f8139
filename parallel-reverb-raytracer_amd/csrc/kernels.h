// kernels.h — launch interface between the C-ABI (trace.hip, source.hip, kept.hip, sort.hip, ir.hip, multi.hip) and the HIP kernels.
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/rvb_capi.h"
#include "../../include/rvb_capi_live.h"
#include "../../include/rvb_capi_window.h"
#include "bvh.h"

struct SceneDev {                       // device pointers of the current scene
    const BvhNode * nodes = nullptr;
    const BvhTri * tris = nullptr;
    const TriShade * shade = nullptr;
    const TriCorners * corners = nullptr;
    const rvb_surface * surfaces = nullptr;
    uint32_t ntris = 0;                  // entries of tris[]
    float cull_abs = 0.0f;              // slack added to the running closest distance when culling
    float cull_rel = 0.0f;
    unsigned long long * stamps = nullptr;   // diagnostic builds only (RVB_STAMPS)
};

// entry of the image-source work list: ray within the launch and bounce; index 0xFFFFFFFF = the direct path of pair `ray`
struct ImageItem { uint32_t ray, index; };
struct TraceArgs {
    SceneDev scene;
    const float4 * directions;          // [nrays]
    rvb_impulse * impulses;             // [nrays * nreflections]
    uint32_t * early;                   // [nrays * 9] triangle hit at bounce 0..8, 0xFFFFFFFF = none
    rvb_image_candidate * candidates;   // [nrays * 9] capacity
    uint32_t * candidate_count;
    ImageItem * image_items;     // [nrays * 9 + npairs] (ray, bounce) pairs whose image ray crosses every image triangle (image_plan_kernel)
    uint32_t * image_item_count;
    uint32_t * image_state;             // [capacity of image_items] per listed pair: queries done (low half), queries failed (high half)
    rvb_impulse * direct;               // slot 0
    unsigned long long * executed;      // bounces executed
    uint32_t * sort_keys;               // [nrays * nreflections] leaf position of the triangle hit, 0xFFFFFFFF = no record (or null)
    uint16_t * sort_keys16;             // the same as 16-bit keys (leaf position >> key_shift, 0xFFFF = no record), written in 64-byte runs through LDS
                                        // (path kernels; needs nreflections % 32 == 0); exactly one of sort_keys / sort_keys16 is set, or neither
    uint32_t key_shift;
    uint32_t * sort_order;              // [nrays * nreflections] record indices grouped by bucket
    uint32_t * time_range;              // [2] float bits: min non-zero / max time of non-zero diffuse impulses; behind the pairs' ranges a count
                                        // per pair of the diffuse impulses that carry volume (rvb_launch_shadow only: live_sum_kernel)
    uint64_t nrays;
    uint32_t nreflections;
    uint32_t stack_entries;             // LDS traversal stack entries per lane (BuiltScene::stack_need)
    uint32_t lds_surfaces;              // surfaces staged in LDS behind the stack by the quad kernels (rvb_lds_surfaces), 0 = none
    uint32_t path_lanes;                // lanes per ray in the path kernel: 4 (path_kernel) or 2 (path_pair_kernel), rvb_path_lanes_for
    // Several (source, microphone) pairs in ONE launch (rvb_trace_pairs): ray r belongs to pair r / rays_per_pair and uses
    // direction r % rays_per_pair; its records, early ids, candidates follow the global ray number.  npairs == 1: mic / source below.
    uint32_t npairs;
    uint32_t rays_per_pair;
    const float4 * pair_mics;           // device [npairs] (xyz, w unused); direct[] and time_range[] then hold one entry per pair
    const float4 * pair_sources;
    uint64_t ray_offset;
    float mic[3];
    float source[3];
    float air[8];
    float * image_dist;                 // rvb_keep_paths only, else null: [nrays * 9 + npairs] INIT_DIST of candidates[i] at i, then of the direct path of every
                                        // pair (negative: hidden) — what rvb_reshade cannot recover from an image impulse
    // [RVB_LIVE_STRIPES][npairs] partial counts of the diffuse impulses that carry volume, all zero between launches: the shadow kernel's
    // waves add to the stripe of their workgroup (one address for all 65 536 of them: shadow_pair_kernel 1.25 -> 5.84 ms at workload C2),
    // and live_sum_kernel behind it adds the stripes up, zeroes them and leaves the counts behind the time ranges
    uint32_t * live_stripes;
};
#define RVB_LIVE_STRIPES 1024

// ---- the trace: trace_kernels.hip (path stage), image_kernels.hip, shadow_kernels.hip; their shared device code: traversal.h ----
// Phase A (trace_kernels.hip): one lane per ray, the sequential closest-hit / reflect chain (kernel.cpp:359-375,
// :459-461, :478, :492-501).  Leaves a work record per bounce in impulses[].
void rvb_launch_path(const TraceArgs & a, hipStream_t s);
// How many surfaces the quad kernels stage in LDS for this scene (all of them, or 0 when they would cost occupancy).
uint32_t rvb_lds_surfaces(uint32_t stack_entries, uint64_t nsurfaces);
// lanes per ray for a launch of `nrays` rays when the caller keeps `concurrent` such traces in flight on the device
uint32_t rvb_path_lanes_for(uint64_t nrays, uint32_t concurrent);
// the two-lane path kernel for up to RVB_MAX_GROUP traces (contexts) in ONE launch: their waves are dispatched and scheduled together
#define RVB_MAX_GROUP 4
void rvb_launch_path_group(const TraceArgs * traces, uint32_t count, hipStream_t s);
uint32_t rvb_shadow_lanes();        // lanes per record in the shadow kernel: 2 (shadow_pair_kernel) unless RVB_SHADOW_LANES=4
// Phase C (image_kernels.hip): image-source validation (kernel.cpp:379-457) + slot 0: a plan kernel (one lane per ray) and a check kernel (four lanes per listed pair).
void rvb_launch_images(const TraceArgs & a, hipStream_t s);
// Phase B (shadow_kernels.hip): one lane per (ray, bounce): diffuse shadow ray to the microphone and the final
// Impulse (kernel.cpp:463-490).  Overwrites the work records.
void rvb_launch_shadow(const TraceArgs & a, hipStream_t s);
// Directional sources (source_kernels.hip): volume_b *= (1 - shape_b) + shape_b * dot3(normalize3(normalize3(v)), direction) on the final
// records of a trace — the diffuse impulses (v = the ray's direction), the image-source candidates and the direct slot(s) (v = mic -
// position) — and the time range of the scaled diffuse records into a.time_range, which the caller has reset (0xFFFFFFFF / 0 per pair).
// patterns: device [npatterns] in their device form, npatterns 1 (every pair) or a.npairs.  Behind rvb_launch_shadow, on a stream that
// has waited for rvb_launch_images.
struct SourcePatternDev { float direction[4]; float shape[8]; };        // rvb_source_pattern with the direction normalised (w = 0)
SourcePatternDev rvb_source_pattern_device_form(const rvb_source_pattern & p);                      // host (source_state.hip)
void rvb_launch_source_pattern(const TraceArgs & a, const SourcePatternDev * patterns, uint32_t npatterns, hipStream_t s);
// The tabulated directivity (rvb_set_source_table of include/rvb_capi.h) at the same place: volume_b *= table[row(v)][b] with the row of
// csrc/attenuation.h (hrtf_row with pos - mic replaced by v) in the source's basis.  rvb_launch_source_table_rays: one row selection per
// (pair, ray) from a.directions into ray_gains[a.npairs][a.rays_per_pair][8] — it reads no record, so rvb_relisten reuses what it left.
// rvb_launch_source_table: the streaming pass over the records with those gains and the time range into a.time_range (reset by the
// caller), then the candidates and the direct slot(s), row by row from the table.
#define RVB_HRTF_ROWS (360 * 180 + 1)   // rows per ear of the device's HRTF table: one per (azimuth, elevation) degree, then the zero row behind quirk Q5
struct SourceTableDev {
    const float * table;                // device [RVB_HRTF_ROWS][8]: the caller's rows, then the zero row
    const float4 * bases;               // device [norientations][3]: bx, by, bz of rvb_source_table_basis
    uint32_t basis_stride;              // float4s between the bases of two pairs: 0 (one orientation for every pair) or 3
    float * ray_gains;                  // device [a.npairs][a.rays_per_pair][8]
};
// host (source_state.hip): the basis of kernel.cpp:538-549 for (facing, up) as twelve floats (bx, by, bz; w = 0), with the device's operations; false where
// normalize3(cross3(up, facing)) is zero or a value is not finite
bool rvb_source_table_basis(const rvb_source_orientation & o, float basis[12]);
void rvb_launch_source_table_rays(const TraceArgs & a, const SourceTableDev & t, hipStream_t s);
void rvb_launch_source_table(const TraceArgs & a, const SourceTableDev & t, hipStream_t s);
// Re-shading a finished trace (reshade_kernels.hip; rvb_keep_paths / rvb_reshade of include/rvb_capi.h).
// path_keep_kernel, between the path and the shadow stage: what the shadow stage destroys of every work record, as a 16-byte side record
// kept[nrays * nreflections] (SideRecord of kept_tiles.h: newDist, DIFF, the surface or "the ray had escaped").  Only reads the records.
// listen != null (RVB_KEEP_LISTENER): also listen[nrays * nreflections], own-plane threshold and triangle (ListenRecord of kept_tiles.h).
void rvb_launch_path_keep(const TraceArgs & a, float4 * kept, uint2 * listen, hipStream_t s);
// How many surfaces the re-shade pass stages in LDS (all of them, or 0: read through L2).
uint32_t rvb_reshade_lds_surfaces(uint64_t nsurfaces);
// reshade_kernel: the final volumes of every diffuse record again — the specular chain along the ray from 1, then the shadow stage's
// product — with a.scene.surfaces, a.air and a.lds_surfaces those of the RE-SHADE, everything else the finished trace's TraceArgs; and
// the time range into a.time_range, which the caller has reset.  reshade_images_kernel: the candidates [0, *candidate_count) and the
// direct slot(s), from a.early, a.image_dist and the same table.  (The wave's tiles in LDS: KeptTileLds of kept_tiles.h, from which the
// launchers of reshade_kernel and relisten_records_kernel take their workgroups and byte counts.)
void rvb_launch_reshade(const TraceArgs & a, const float4 * kept, hipStream_t s);
void rvb_launch_reshade_images(const TraceArgs & a, hipStream_t s);
// A new microphone on a finished trace (relisten_kernels.hip; RVB_KEEP_LISTENER / rvb_relisten of include/rvb_capi.h).
// relisten_records_kernel: every slot of a.impulses as the work record the path stage left (trace_kernels.hip, "Work record") — the chain
// volumes under a.scene.surfaces (a.lds_surfaces as rvb_reshade_lds_surfaces gives it), the position the record holds, DIFF and newDist of
// `kept` (SideRecord), threshold and triangle of `listen` (ListenRecord), the ray's pair tag; 64 zero bytes behind an escape.  rvb_launch_images, rvb_launch_shadow and
// rvb_launch_source_pattern then run as behind a path kernel.
void rvb_launch_relisten_records(const TraceArgs & a, const float4 * kept, const uint2 * listen, hipStream_t s);
// Material gradients of a weighted histogram from the kept trace (reshade_grad_kernels.hip; rvb_reshade_grad of include/rvb_capi.h).
// The launch works on ONE pair's rays, [first_ray, first_ray + nrays) of the kept launch, with the speaker model `model` (<= 8 channels)
// and the weights already in the accumulation image's layout [bin][channel][band] (rvb_launch_reshade_grad_weights makes it from the
// histogram's layout [channel][8][nbins]).  Every workgroup keeps a binary64 table of nsurfaces * 16 + 8 sums — a surface's row in
// rvb_surface's order, then the eight air derivatives — and leaves it in partials[block]; the reduce kernel adds the `blocks` tables in a
// fixed order and rounds once: out[nsurfaces * 16 + 8] floats.  Bit-identical from run to run.
struct AttenuationModel;
struct ReshadeGradArgs {
    const float * weights;              // device [nbins][nchannels][8]
    uint64_t nbins;
    float predelay, sample_rate;
    uint64_t first_ray;                 // of the pair within the kept launch
    uint32_t nrays;                     // rays of the pair
    float mic[3];                       // the pair's microphone in the trace
    bool has_pattern;                   // a source pattern scales the pair's records
    SourcePatternDev pattern;
    const float * ray_gains;            // device [nrays][8], the pair's rows of SourceTableDev::ray_gains: a source table scales the pair's records; null: none
    uint64_t nsurfaces;
};
#define RVB_RESHADE_GRAD_MAX_REFLECTIONS 2048     // a ray's chain checkpoints (one per tile of bounces and lane) live in LDS
uint32_t rvb_reshade_grad_blocks(uint64_t nrays, uint64_t nsurfaces);      // workgroups (= partial tables) of the launch
void rvb_launch_reshade_grad_weights(const float * weights, float * transposed, uint32_t nchannels, uint64_t nbins, hipStream_t s);
void rvb_launch_reshade_grad(const TraceArgs & a, const float4 * kept, const AttenuationModel & model, const ReshadeGradArgs & g,
                             double * partials, uint32_t blocks, hipStream_t s);
void rvb_launch_reshade_grad_reduce(const double * partials, uint32_t blocks, uint64_t nsurfaces, float * out, hipStream_t s);
// The same gradient per TRIANGLE (rvb_reshade_grad_map of include/rvb_capi.h).  The terms pass (reshade_grad_kernels.hip: reshade_grad_kernel
// with another place for a term) leaves, by the record's number i within the pair, terms[i][16] — specular 0..7, diffuse 8..15; no row
// for a slot without a record —, keys[i] = the record's triangle from `listen` (ntriangles for such a slot) and values[i] = i.  After a
// stable sort by key the fold (reshade_grad_map_kernels.hip) adds the rows of every run in binary64 in entry order: tiles of
// RVB_GRAD_MAP_TILE entries, `partials` [rvb_grad_map_tiles(n)][2][16] doubles for the runs that cross a tile edge, which the combine
// adds in tile order; it also writes the zeros of a triangle without a run (starts / ends: rvb_launch_bin_starts).  Together they write
// every entry of map[ntriangles][16] exactly once.
inline uint64_t rvb_grad_map_tiles(uint64_t n) { return (n + RVB_GRAD_MAP_TILE - 1) / RVB_GRAD_MAP_TILE; }
void rvb_launch_reshade_grad_map_terms(const TraceArgs & a, const float4 * kept, const uint2 * listen, const AttenuationModel & model, const ReshadeGradArgs & g,
                                       uint32_t ntriangles, float * terms, uint32_t * keys, uint32_t * values, hipStream_t s);
void rvb_launch_reshade_grad_map_fold(const uint32_t * sorted_keys, const uint32_t * sorted_values, uint64_t n, uint32_t ntriangles, const float * terms,
                                      double * partials, float * map, hipStream_t s);
void rvb_launch_reshade_grad_map_combine(const uint32_t * starts, const uint32_t * ends, uint32_t ntriangles, const double * partials, float * map, hipStream_t s);
// The merged image list on the device and the image-source part of the material gradient (image_grad_kernels.hip;
// include/rvb_capi_images.h).  winners[i]: the position in a.candidates of the candidate that output impulse i is copied from, or
// RVB_IMAGE_WINNER_DIRECT for `direct`, the selected pair's direct slot.
#define RVB_IMAGE_WINNER_DIRECT 0xFFFFFFFFu
#define RVB_IMAGE_GRAD_STEPS 8u          // a candidate's chain: the bounces 0 .. slot - 2, slot <= RVB_NUM_IMAGE_SOURCE - 1
#define RVB_IMAGE_GRAD_ROW 80u           // words of a term row: the chain's surfaces [8] (0xFFFFFFFF: no step), the steps' terms [8][8], the air terms [8]
void rvb_launch_image_gather(const rvb_image_candidate * candidates, const rvb_impulse * direct, const uint32_t * winners, uint64_t n,
                             rvb_impulse * images, hipStream_t s);
// rvb_reshade_grad_images.  `a`: the kept trace's arguments under the table and air that the records reflect now; `direct_dist`: the
// place of the pair's direct slot in a.image_dist; weights: device [nchannels][8][nbins], read in place; pattern / table: the source
// directivity that the records reflect (at most one; table_basis: the pair's three float4).  The terms kernel leaves `rows`
// [n][RVB_IMAGE_GRAD_ROW]; the reduce kernel adds them per surface and band in binary64 — thread t of the surface's workgroup the images
// t, t + 256, ... in list order and chain order, then a fixed tree — and writes out[nsurfaces * 16 + 8] floats, the diffuse entries +0.
struct ImageGradArgs {
    const uint32_t * winners;
    const rvb_impulse * images;         // the gathered list: position and time of image i
    uint64_t n;
    uint64_t direct_dist;
    const float * weights;
    uint64_t nbins;
    float predelay, sample_rate;
    float mic[3];                       // the pair's microphone in the trace
    bool has_pattern;
    SourcePatternDev pattern;
    const float * table;                // null: no source table
    const float4 * table_basis;
};
void rvb_launch_reshade_grad_images(const TraceArgs & a, const AttenuationModel & model, const ImageGradArgs & g, uint32_t * rows, hipStream_t s);
void rvb_launch_reshade_grad_images_reduce(const uint32_t * rows, uint64_t n, uint64_t nsurfaces, float * out, hipStream_t s);
// Source-end gradients from the kept trace (source_grad_kernels.hip; include/rvb_capi_source_grad.h): L = sum w * H of rvb_reshade_grad
// (rays: `g` as that launch takes it, the weights transposed) and of rvb_reshade_grad_images (images: `g` as that launch takes it, the
// weights read in place), differentiated with respect to the source gain of every ray or image.  What a launch leaves per item (each may
// be null): grad[n][8] the sums rounded once, lambda[n][8] the binary64 sums before the rounding (the pattern kernel's input), rows[n] the
// row of the source table for the item's departure vector under table_basis (three float4; read with rows only).  The images kernel also
// leaves departures[n] = mic - position (w = 0) and, where asked, units[n] = normalize3(normalize3(departure)).
// The pattern pair: a partial of eleven binary64 sums (shape[8], direction[3]) per tile of RVB_SOURCE_GRAD_TILE items in `partials`, then
// out[12] floats, rvb_source_pattern_grad's layout.  Bit-identical from run to run.
struct SourceGradOut {
    float * grad;
    double * lambda;
    uint32_t * rows;
    const float4 * table_basis;
};
#define RVB_SOURCE_GRAD_TILE 256
inline uint64_t rvb_source_grad_tiles(uint64_t n) { return (n + RVB_SOURCE_GRAD_TILE - 1) / RVB_SOURCE_GRAD_TILE; }
void rvb_launch_source_grad_rays(const TraceArgs & a, const float4 * kept, const AttenuationModel & model, const ReshadeGradArgs & g, const SourceGradOut & o,
                                 hipStream_t s);
void rvb_launch_source_grad_images(const TraceArgs & a, const AttenuationModel & model, const ImageGradArgs & g, const SourceGradOut & o, float4 * departures,
                                   float4 * units, hipStream_t s);
void rvb_launch_source_grad_pattern(const float4 * vectors, const double * lambda, uint64_t n, const SourcePatternDev & pattern, double * partials, hipStream_t s);
void rvb_launch_source_grad_pattern_fold(const double * partials, uint64_t n, float * out, hipStream_t s);
// Decay curves (decay_kernels.hip; rvb_decay_curve / rvb_decay_times / rvb_decay_loss of include/rvb_capi.h) on nrows rows of nbins floats.
// Every phase is a launch of its own — a value per tile of RVB_DECAY_TILE bins, one wave per row over the row's tiles, the tile again on
// top of its carry —; `tiles` is [nrows][rvb_decay_tiles(nbins)] doubles (three such planes for the loss: m d^2, 2 m d, g), `first`
// [2][nrows][tiles] bin numbers, `window` [nrows] {k0, k1}.
inline uint32_t rvb_decay_tiles(uint64_t nbins) { return (uint32_t) ((nbins + RVB_DECAY_TILE - 1) / RVB_DECAY_TILE); }
void rvb_launch_decay_curve_sums(const float * hist, uint64_t nrows, uint64_t nbins, double * tiles, hipStream_t s);
void rvb_launch_decay_curve_carry(uint64_t nrows, uint64_t nbins, double * tiles, hipStream_t s);
void rvb_launch_decay_curve_scan(const float * hist, uint64_t nrows, uint64_t nbins, const double * tiles, float * curve, hipStream_t s);
// ratio_* = 10^(db / 10): the window is found by comparing E with E[0] * ratio
void rvb_launch_decay_times_find(const float * curve, uint64_t nrows, uint64_t nbins, double ratio_begin, double ratio_end, uint32_t * first, hipStream_t s);
void rvb_launch_decay_times_window(const uint32_t * first, uint64_t nrows, uint64_t nbins, uint2 * window, hipStream_t s);
void rvb_launch_decay_times_sums(const float * curve, uint64_t nrows, uint64_t nbins, const uint2 * window, double * tiles, hipStream_t s);
void rvb_launch_decay_times_fit(const float * curve, uint64_t nrows, uint64_t nbins, const uint2 * window, const double * tiles, double sample_rate,
                                float * seconds, hipStream_t s);
void rvb_launch_decay_loss_sums(const float * curve, const float * target, const float * mask, uint64_t nrows, uint64_t nbins, bool normalised,
                                double * tiles, hipStream_t s);
void rvb_launch_decay_loss_carry(const float * curve, uint64_t nrows, uint64_t nbins, bool normalised, double * tiles, double * loss_rows, hipStream_t s);
void rvb_launch_decay_loss_scan(const float * hist, const float * curve, const float * target, const float * mask, uint64_t nrows, uint64_t nbins,
                                bool normalised, const double * tiles, float * weights, hipStream_t s);
// Room acoustic parameters of a curve and their adjoint (decay_params_kernels.hip; rvb_decay_params / rvb_decay_params_loss), in the
// tile shape of the decay kernels.  `first` is [5][nrows][tiles] bin numbers — the first bin at or below 0 dB, below -10 dB, at or below
// -5 dB, below -25 dB, below -35 dB —, `window` [nrows][5] the same per row, `tiles` four planes of [nrows][tiles] doubles: sum xc level
// of the EDT, T20 and T30 windows and sum E over the bins behind bin 0 (the adjoint reuses plane 0 for sum g).
struct DecayParamsRatios { double r[5]; };                // 10^(db / 10) for 0, -10, -5, -25, -35 dB
// What decay_params_fit_kernel leaves per row for the adjoint, with c_p = 2 weight (q - target), 0 for a parameter that does not count:
// every term of g[k] = dL/dE[k] but for E[k] itself, so that the adjoint kernels evaluate g from E on the fly.
struct DecayParamsRow {
    double time_coef[3];      // EDT, T20, T30: c_p (60 / (s^2 fs)) C10 / Sxx; g[k] += time_coef xc_k / E[k] inside [k0, k1)
    double centre[3];         // (n - 1) / 2: xc_k = (k - k0) - centre
    double c_zero[2], c_at[2];// C50, C80: g[0] += c C10 / early; g[ke] -= c C10 (1 / early + 1 / late)
    double d_zero, d_at;      // D50: g[0] += c E[k50] / E[0]^2; g[k50] -= c / E[0]
    double ts_zero, ts_each;  // Ts: g[0] -= c Ts / E[0]; g[k] += c / (fs E[0]) for every k >= 1
    uint32_t k0[3], k1[3];    // the windows; k0 == k1 == 0 where the time does not count
    uint32_t ke[2];           // bin of 50 ms and of 80 ms; 0xFFFFFFFF: behind the row's end
    uint32_t counts;          // any parameter of the row counts
};
void rvb_launch_decay_params_find(const float * curve, uint64_t nrows, uint64_t nbins, const DecayParamsRatios & ratios, uint32_t * first, hipStream_t s);
void rvb_launch_decay_params_window(const uint32_t * first, uint64_t nrows, uint64_t nbins, uint32_t * window, hipStream_t s);
void rvb_launch_decay_params_sums(const float * curve, uint64_t nrows, uint64_t nbins, const uint32_t * window, double * tiles, hipStream_t s);
// ke50 / ke80: 0xFFFFFFFF where the bin lies behind the row's end; targets / param_weights: device [nrows][7], or both null (no loss)
void rvb_launch_decay_params_fit(const float * curve, uint64_t nrows, uint64_t nbins, const uint32_t * window, const double * tiles, double sample_rate,
                                 uint32_t ke50, uint32_t ke80, const float * targets, const float * param_weights, float * params,
                                 DecayParamsRow * rows, double * loss_rows, hipStream_t s);
void rvb_launch_decay_params_adjoint_sums(const float * curve, uint64_t nrows, uint64_t nbins, const DecayParamsRow * rows, double * tiles, hipStream_t s);
void rvb_launch_decay_params_adjoint_carry(uint64_t nrows, uint64_t nbins, double * tiles, hipStream_t s);
void rvb_launch_decay_params_adjoint_scan(const float * hist, const float * curve, uint64_t nrows, uint64_t nbins, const DecayParamsRow * rows,
                                          const double * tiles, float * weights, hipStream_t s);
// Grouping of the work records by the leaf position of the triangle they start from (rocprim_sort.hip):
// order[] lists the records bucket by bucket and the shadow kernel walks that list.
size_t rvb_group_records_temp_bytes(uint64_t n);
hipError_t rvb_group_records(void * temp, size_t temp_bytes, const uint32_t * keys, uint32_t * keys_scratch, uint32_t * order,
                             uint64_t n, uint32_t first_record, int begin_bit, int end_bit, hipStream_t s);
hipError_t rvb_group_records16(void * temp, size_t temp_bytes, const uint16_t * keys, uint16_t * keys_scratch, uint32_t * order,
                               uint64_t n, uint32_t first_record, int begin_bit, int end_bit, hipStream_t s);

// ---- the stages behind the trace: attenuate_kernels.hip (materialised attenuation, time range, predelay), histogram_kernels.hip
// (fast mode), exact_kernels.hip (exact mode, flatten), rocprim_sort.hip (the sort); their shared device code: attenuation.h ----
// (RVB_HRTF_ROWS, above: the rows of one ear of the device's HRTF table)
struct AttenuationModel {
    int hrtf = 0;                       // 0: speakers, 1: hrtf
    uint32_t nchannels = 0;             // speakers: <= RVB_MAX_SPEAKERS; hrtf: 2
    float mic[3] = {0, 0, 0};
    rvb_speaker speakers[8] = {};       // as the caller gave them; make_model passes their device form (speaker_device_form, attenuation.h)
    // more than 8 speakers (ordered_sum_wide_kernel): the table in device memory, one 16-byte entry per channel — the same device form,
    // made by rvb_make_speaker_table.  speakers[] then holds the first eight only (the kernels that take them never run for a wide layout).
    const float4 * speaker_table = nullptr;
    const float * hrtf_table = nullptr; // device [2][RVB_HRTF_ROWS][8]
    float facing[3] = {0, 0, 0}, up[3] = {0, 0, 0};
};

// kernel attenuate / hrtf for one channel, materialised (kernel.cpp:515-535, :586-625)
void rvb_launch_attenuate(const AttenuationModel & m, uint32_t channel, const rvb_impulse * in, uint64_t n,
                          rvb_attenuated_impulse * out, hipStream_t s);
// min non-zero / max attenuated time over all channels -> range[0], range[1] (uint bits of floats;
// caller initialises to 0xFFFFFFFF / 0)
void rvb_launch_time_range(const AttenuationModel & m, const rvb_impulse * in, uint64_t n, uint32_t * range, hipStream_t s);
// fused attenuate + predelay + bin with float atomics into the image acc[nbins][nchannels][8]
void rvb_launch_histogram_fast(const AttenuationModel & m, const rvb_impulse * in, uint64_t n, float predelay,
                               float sample_rate, uint64_t nbins, float * acc, hipStream_t s);
// acc[bin][channel][band] -> hist[channel][band][bin] (added to what is there)
void rvb_launch_histogram_transpose(const float * acc, float * hist, uint32_t nchannels, uint64_t nbins, hipStream_t s);
// acc[i] += x[i], i < n: a whole histogram of another device added to this one's (csrc/multi.hip, the fast mode without RCCL)
void rvb_launch_add(float * acc, const float * x, uint64_t n, hipStream_t s);
// exact mode helpers: per-impulse bin keys (`sentinel` = nbins marks impulses that add nothing), then the ordered per-bin
// summation of `nchannels` channels that share the sorted list, added to what hist [all channels][8][nbins] holds
void rvb_launch_bin_keys(const AttenuationModel & m, uint32_t channel, const rvb_impulse * in, uint64_t n, uint64_t index_base,
                         float predelay, float sample_rate, uint32_t sentinel, uint32_t * keys, uint32_t * values, hipStream_t s);
void rvb_launch_ordered_sum(const AttenuationModel & m, uint32_t first_channel, uint32_t nchannels, const rvb_impulse * diffuse,
                            uint64_t ndiffuse, const rvb_impulse * images,
                            const uint32_t * sorted_values, const uint32_t * starts, const uint32_t * ends, uint64_t n,
                            uint64_t nbins, float * hist, hipStream_t s, uint64_t bin_begin = 0, uint64_t bin_end = ~0ull,   // bins [bin_begin, bin_end) only
                            const uint32_t * coarse_keys = nullptr);
// coarse_keys: the list is ordered by coarse bin only (sort_and_bin with coarse_shift = RVB_COARSE_SHIFT: runs of RVB_COARSE_BINS
// neighbouring bins, every bin's entries in impulse order within its run) — its whole keys, and starts / ends are per coarse bin.
// The same sums then come from ordered_sum_coarse_kernel, a wave per coarse bin.
#define RVB_COARSE_SHIFT 5
#define RVB_COARSE_BINS (1u << RVB_COARSE_SHIFT)
// The same fold for more than 8 speaker channels (ordered_sum_wide_kernel): ALL m.nchannels channels of bins [bin_begin, bin_end) in one
// launch, the speaker table read from m.speaker_table, every record gathered from HBM once.
void rvb_make_speaker_table(const rvb_speaker * speakers, uint64_t nspeakers, float4 * table);      // host: the entries of speaker_table
void rvb_launch_ordered_sum_wide(const AttenuationModel & m, const rvb_impulse * diffuse, uint64_t ndiffuse, const rvb_impulse * images,
                                 const uint32_t * sorted_values, const uint32_t * starts, const uint32_t * ends, uint64_t n,
                                 uint64_t nbins, float * hist, hipStream_t s, uint64_t bin_begin = 0, uint64_t bin_end = ~0ull);
// HRTF model, both ears at once: ONE list of 2 n (key, value) entries — ear e's entry of impulse j at e * n + j, key e * (nbins + 1) + bin
// (sentinel e * (nbins + 1) + nbins) — and the ordered sum of both ears over its sorted form (starts / ends indexed by that key)
void rvb_launch_bin_keys_hrtf(const AttenuationModel & m, const rvb_impulse * in, uint64_t count, uint64_t index_base, uint64_t n,
                              float predelay, float sample_rate, uint32_t nbins, uint32_t * keys, uint32_t * values, hipStream_t s);
void rvb_launch_ordered_sum_hrtf(const AttenuationModel & m, const rvb_impulse * diffuse, uint64_t ndiffuse, const rvb_impulse * images,
                                 const uint32_t * sorted_values, const uint32_t * starts, const uint32_t * ends, uint64_t nbins, float * hist,
                                 hipStream_t s, uint64_t bin_begin = 0, uint64_t bin_end = ~0ull);
// The live list of exact mode, in place of rvb_launch_bin_keys* and their identity values: only the impulses that carry volume are
// listed (numbered as the fold gathers them: diffuse, then images), in their order, and sentinel entries fill the list up to `listed`
// entries — per ear for the HRTF model, ear 1's half from `listed` on.  `listed` bounds the live impulses by contract (the trace's
// count + every image); what would land behind it is dropped and *overflow (any memory the device can write) set.  raw: n words (2 n:
// HRTF) for the raw keys; scratch: rvb_live_scratch_bytes(n) — the total of live impulses in its first word once the launches have
// run, then a word per tile of RVB_LIVE_TILE impulses.  Three launches, none waits for another's workgroups.
size_t rvb_live_scratch_bytes(uint64_t n);
void rvb_launch_live_list(const AttenuationModel & m, const rvb_impulse * diffuse, uint64_t ndiffuse, const rvb_impulse * images, uint64_t n,
                          float predelay, float sample_rate, uint32_t nbins, uint64_t listed, uint32_t * raw, void * scratch,
                          uint32_t * keys, uint32_t * values, uint32_t * overflow, hipStream_t s);
// starts[key] / ends[key] = first position of `key` in the sorted list / one past its last (starts[] pre-filled with 0xFFFFFFFF by
// the caller, nbins entries each; ends[] is only read where starts[] was written).  With shift > 0 the list is ordered on
// key >> shift only and the boundaries are those of key >> shift, (nbins + 2^shift - 1) >> shift entries each: from the first to
// behind the last entry of the run whose whole key is below nbins (ends[] pre-filled with 0 by the caller).
void rvb_launch_bin_starts(const uint32_t * sorted_keys, uint64_t n, uint64_t nbins, uint32_t * starts, uint32_t * ends, hipStream_t s, int shift = 0);
// flattenImpulses of already attenuated impulses (rayverb.cpp:48-77): keys + ordered sum
void rvb_launch_flat_keys(const rvb_attenuated_impulse * in, uint64_t n, float sample_rate, uint32_t * keys, uint32_t * values,
                          uint32_t * max_time_bits, hipStream_t s);
void rvb_launch_flat_ordered_sum(const rvb_attenuated_impulse * in, const uint32_t * sorted_keys, const uint32_t * sorted_values,
                                 const uint32_t * starts, uint64_t n, uint64_t nbins, float * out, hipStream_t s);
void rvb_launch_fix_predelay(rvb_attenuated_impulse * a, uint64_t n, float seconds, hipStream_t s);
// csrc/radix_sort.hip: stable LSD radix sort whose kernels fit beside resident path waves (single-wave workgroups, <= 32 VGPRs)
size_t rvb_radix_sort_temp_bytes(uint64_t n);
hipError_t rvb_radix_sort_pairs(void * temp, size_t temp_bytes, const uint32_t * keys, const uint32_t * values, uint32_t value_base,
                                uint32_t * keys_a, uint32_t * values_a, uint32_t * keys_b, uint32_t * values_b, uint64_t n,
                                int begin_bit, int end_bit, bool want_keys, const uint32_t ** keys_sorted, const uint32_t ** values_sorted,
                                hipStream_t s);
// stable sort of (key, value) pairs on key bits [begin_bit, key_bits) (rocPRIM's device radix sort, rocprim_sort.hip); the keys come
// out whole; temp storage managed by the caller
size_t rvb_sort_temp_bytes(uint64_t n);
void rvb_sort_pairs(void * temp, size_t temp_bytes, const uint32_t * keys_in, uint32_t * keys_out,
                    const uint32_t * values_in, uint32_t * values_out, uint64_t n, int begin_bit, int key_bits, hipStream_t s);
// The echo finder (window_kernels.hip; include/rvb_capi_window.h; the select's arithmetic: window_select.h).  `scratch` is one block of
// rvb_window_scratch_bytes(n) bytes: the select's state and the gather's counter, the digit tables of the six passes, the gathered
// composites, the entries of rvb_window_paths, then a key per record.  rvb_launch_window_begin zeroes its head (a memset node);
// the others are one kernel each but rvb_launch_window_pass, which is window_histogram_kernel for digit `pass` (0..2: of the key — 0 is
// counted by the score kernel, so only its walk runs —, 3..5: of ~record) and window_walk_kernel behind it.  The sort kernel writes entries
// [0, want) and nothing else; the paths kernel reads them from the scratch.  listen: the pair's listener records, null with hits == null.
struct WindowWeights { float w[8]; };
size_t rvb_window_scratch_bytes(uint64_t n);
rvb_window_entry * rvb_window_scratch_entries(void * scratch);
const void * rvb_window_scratch_state(const void * scratch);             // window_select::State
hipError_t rvb_launch_window_begin(void * scratch, hipStream_t s);
void rvb_launch_window_score(const rvb_impulse * in, uint64_t n, float t_begin, float t_end, const WindowWeights & weights, void * scratch, hipStream_t s);
void rvb_launch_window_pass(uint32_t pass, uint64_t n, uint64_t max_entries, void * scratch, hipStream_t s);
void rvb_launch_window_gather(uint64_t n, void * scratch, hipStream_t s);
void rvb_launch_window_sort(const rvb_impulse * in, void * scratch, rvb_window_entry * entries, hipStream_t s);
void rvb_launch_window_paths(const rvb_impulse * in, const uint2 * listen, uint32_t nreflections, uint64_t max_paths, uint64_t max_hits,
                             const void * scratch, rvb_window_path * paths, rvb_window_hit * hits, hipStream_t s);
