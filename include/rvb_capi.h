/* rvb_capi.h — C-ABI of the MI355X-native acoustic ray tracer (librvb_hip.so).
 *
 * This is the drop-in boundary for the reference's per-ray hot path.  The reference has no
 * FFI of its own for this path: its callers (cmd/main.cpp:241-298 and the gtest fixtures)
 * use the C++ classes of rayverb/rayverb.h directly, which in turn drive three OpenCL
 * kernels.  Each entry point below names the reference interface it replaces; the C++ mirror
 * of those classes (include/rayverb/rayverb.h, built on nothing but this header) is what a
 * maintainer links instead of the OpenCL-backed library — see INTEGRATION.md.
 *
 * Conventions
 *   - every function returns RVB_OK (0) or an RVB_ERR_* code; rvb_last_error() gives the text
 *     (the reference throws cl::Error / std::runtime_error instead, rayverb.cpp:151-192);
 *   - all pointers are caller-owned; "host" pointers are ordinary memory, "device" pointers are
 *     HBM addresses on the context's GPU (e.g. torch.Tensor.data_ptr());
 *   - PODs are layout-identical to reference rayverb/clstructs.h (sizes in SURVEY.md §8(a));
 *     this header demands no particular alignment of host buffers;
 *   - a context is bound to one GPU and one HIP stream and is not thread-safe (the reference's
 *     objects are not either: one in-order queue per KernelLoader, rayverb.cpp:191);
 *   - there is no CPU fallback: without a usable gfx950 device rvb_create() fails.
 */
#ifndef RVB_CAPI_H
#define RVB_CAPI_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define RVB_NUM_IMAGE_SOURCE 10   /* reference rayverb/clstructs.h:4 */
#define RVB_NUM_BANDS 8           /* VolumeType = cl_float8, reference rayverb/clstructs.h:13 */

enum {
    RVB_OK = 0,
    RVB_ERR_INVALID = 1,     /* bad argument */
    RVB_ERR_NO_DEVICE = 2,   /* no usable gfx950 GPU / HIP runtime failure at start-up */
    RVB_ERR_HIP = 3,         /* a HIP call failed */
    RVB_ERR_STATE = 4,       /* call order (e.g. trace before set_scene) */
    RVB_ERR_CAPACITY = 5     /* caller buffer too small / scene exceeds a built-in limit */
};

/* reference rayverb/clstructs.h:17-24 (Triangle), :27-32 (Surface), :36-42 (Impulse),
 * :44-49 (AttenuatedImpulse), :53-58 (Speaker); cl_float3 is a 16-byte float4. */
typedef struct { uint64_t surface, v0, v1, v2; } rvb_triangle;                          /* 32 B */
typedef struct { float s[4]; } rvb_float3;                                              /* 16 B */
typedef struct { float specular[8]; float diffuse[8]; } rvb_surface;                    /* 64 B */
typedef struct { float volume[8]; float position[4]; float time; float pad_[3]; } rvb_impulse;     /* 64 B */
typedef struct { float volume[8]; float time; float pad_[7]; } rvb_attenuated_impulse;  /* 64 B */
typedef struct { float direction[4]; float coefficient; float pad_[3]; } rvb_speaker;   /* 32 B */

/* One valid image-source contribution of one ray (what the reference keeps per work-item in
 * image_source[i*10+slot] / image_source_index[i*10+slot], kernel.cpp:258-264), compacted. */
typedef struct {
    uint64_t ray;            /* global ray index (ray_offset of the trace call added) */
    uint32_t slot;           /* 1..9 (slot 0, the direct path, is reported separately) */
    uint32_t index;          /* triangle index + 1 (kernel.cpp:453) */
    rvb_impulse impulse;
} rvb_image_candidate;       /* 80 B */

typedef struct rvb_ctx rvb_ctx;

/* ---- life cycle: replaces ContextProvider / KernelLoader (rayverb.cpp:151-192) ------------- */
int rvb_create(rvb_ctx ** out, int device, unsigned flags);
void rvb_destroy(rvb_ctx * ctx);
const char * rvb_last_error(const rvb_ctx * ctx);       /* ctx may be NULL after a failed rvb_create */
int rvb_synchronize(rvb_ctx * ctx);                     /* wait for the context's stream */
/* Work submitted to the context after this call starts only after `hip_event` (a hipEvent_t recorded on another stream,
 * e.g. the one a caller-owned buffer was zeroed on) has completed.  No host synchronisation. */
int rvb_wait_for_event(rvb_ctx * ctx, void * hip_event);
/* Records `hip_event` (a hipEvent_t of the caller's) behind the work submitted to the context so far: the counterpart of rvb_wait_for_event
 * for a caller that hands a buffer the context has written to a stream of its own (e.g. a histogram block to the next device). */
int rvb_record_event(rvb_ctx * ctx, void * hip_event);
/* Name ("gfx950"), compute-unit count and HBM bytes of the bound device; its HIP device index. */
int rvb_device_info(rvb_ctx * ctx, char * arch, uint64_t arch_capacity, int * compute_units, uint64_t * hbm_bytes);
int rvb_device_index(rvb_ctx * ctx, int * device);

/* ---- scene: replaces the geometry half of Raytracer::Raytracer (rayverb.cpp:242-293) --------
 * Copies triangles / vertices / surfaces, builds the BVH on the host and uploads everything.
 * Triangle and surface indices are validated (the reference never calls its own
 * SceneData::valid(), rayverb.cpp:463-502; out-of-range indices are rejected here). */
int rvb_set_scene(rvb_ctx * ctx,
                  const rvb_triangle * triangles, uint64_t ntriangles,
                  const rvb_float3 * vertices, uint64_t nvertices,
                  const rvb_surface * surfaces, uint64_t nsurfaces);
/* Gives `ctx` the scene `from` holds — the SAME device buffers, no second build, no second copy: the contexts of one GPU that trace
 * side by side in one room (rvb_pipeline_*, rvb_trace_group; the reference builds one Raytracer per scene, rayverb.cpp:242-293) then
 * keep one hierarchy in HBM and in the L2s instead of one each.  The buffers live as long as any context holds them; a later
 * rvb_set_scene on either context gives THAT context a scene of its own and leaves the other's untouched.
 * RVB_ERR_STATE: `from` has no scene; RVB_ERR_INVALID: the contexts are on different devices. */
int rvb_share_scene(rvb_ctx * ctx, rvb_ctx * from);
/* BVH statistics of the current scene (nodes, leaf triangles kept, tree depth). */
int rvb_scene_info(rvb_ctx * ctx, uint64_t * nodes, uint64_t * kept_triangles, uint32_t * depth);

/* ---- ray directions: replaces the per-group cl::copy of rayverb.cpp:593-598 ---------------- */
/* Directions are unit vectors (reference getRandomDirections, helpers.cpp:63-81); RVB_ERR_INVALID for a direction that is not
 * finite or whose length is outside [0.5, 2] (the range the pruning margins of the acceleration structure are derived for).
 * The device variant borrows the caller's buffer and does not inspect it: the same contract is the caller's to keep.
 * rvb_set_scene, rvb_share_scene and rvb_set_directions* void the last trace and everything made from it: until the next trace the
 * fetches (rvb_get_*, rvb_diffuse_device), rvb_ir_select_pair and rvb_ir_configure_* return RVB_ERR_STATE, an IR configuration and a
 * prepared exact list are void (rvb_ir_time_range*, rvb_ir_accumulate*, rvb_ir_exact_*, rvb_ir_download: RVB_ERR_STATE), and a kept trace
 * is no longer usable (rvb_reshade, rvb_relisten). */
int rvb_set_directions(rvb_ctx * ctx, const rvb_float3 * directions, uint64_t nrays);          /* host */
int rvb_set_directions_device(rvb_ctx * ctx, const void * d_directions, uint64_t nrays);        /* device, borrowed */
/* A hint, never a change of results: how many traces of this size the caller keeps in flight on the device at a time (several
 * contexts whose streams run side by side; default 1).  The path kernel spends two lanes per ray instead of four when the rays in
 * flight fill the chip without the extra waves (csrc/trace_kernels.hip — the path stage —, rvb_path_lanes_for).  No reference counterpart: the
 * reference runs one 4096-ray group at a time (rayverb.cpp:586-591). */
int rvb_set_concurrent_traces(rvb_ctx * ctx, uint32_t traces);
/* Measurement / test hook, never a change of results: the path kernel of this context's traces with `lanes` lanes per ray — 4 (path_kernel),
 * 2 (path_pair_kernel), 1 (path_lane_kernel) — whatever the launch size; 0 (default) lets every launch choose (rvb_path_lanes_for).  The three
 * kernels write the same bytes (tests/test_gpu_parity.py runs every trace case with each). */
int rvb_set_path_lanes(rvb_ctx * ctx, uint32_t lanes);

/* ---- trace: replaces Raytracer::raytrace (rayverb.cpp:538-685) + kernel raytrace
 * (kernel.cpp:304-503).  Traces exactly nrays rays (all at once, no 4096-ray groups) for
 * nreflections bounces; results stay in HBM.  Asynchronous on the context's stream.
 * ray_offset is added to ray numbers reported by rvb_get_image_candidates (multi-GPU shards). */
int rvb_trace(rvb_ctx * ctx, const float mic[3], const float source[3],
              uint64_t nreflections, const float air_coefficient[8], uint64_t ray_offset);

/* Several (source, microphone) pairs of one scene in ONE launch — what a caller of the reference does with one
 * Raytracer::raytrace (rayverb.cpp:538-685) per pair, e.g. the 64 pairs of a hall.  Every pair is traced with the context's
 * nrays directions; ray r of pair p is global ray p * nrays + r: rvb_get_diffuse / rvb_diffuse_device return
 * [npairs][nrays][nreflections] impulses and rvb_get_image_candidates reports global ray numbers (pair = ray / nrays).
 * mics / sources are [npairs][3].  More rays per launch fill the GPU better (path tracing costs 3.8 ms per 100 k rays at
 * 100 k, 2.9 ms at 400 k); results are bit-identical to tracing the pairs one by one. */
int rvb_trace_pairs(rvb_ctx * ctx, const float * mics, const float * sources, uint64_t npairs,
                    uint64_t nreflections, const float air_coefficient[8], uint64_t ray_offset);

/* rvb_trace on several contexts of one device at once (at most 4): same results as calling rvb_trace(ctxs[i], mics + 3 i, sources + 3 i,
 * nreflections, air_coefficient, ray_offsets ? ray_offsets[i] : 0) one after the other, but the path kernels of the group are ONE launch
 * when the rays of the group fill the chip (their waves are then scheduled together instead of one launch after the other's).  Every
 * context keeps its own rays, buffers and stream; what follows the path kernel runs per context as in rvb_trace.  No reference
 * counterpart (the reference traces one 4096-ray group at a time, rayverb.cpp:586-591). */
int rvb_trace_group(rvb_ctx ** ctxs, uint64_t count, const float * mics, const float * sources, uint64_t nreflections,
                    const float air_coefficient[8], const uint64_t * ray_offsets);
/* ---- directional sources: a per-band polar pattern at the SOURCE end (csrc/source_kernels.hip) ------------------------------------
 * The twin of rvb_speaker at the other end of the path; no reference counterpart (the reference's source radiates equally in every
 * direction and band).  `direction` is the way the source faces (any non-zero length; direction[3] is ignored), shape[b] the shape of
 * band b as for a speaker: 0 omni, 0.5 cardioid, 1 figure-of-eight.
 *
 * CONTRACT.  For an impulse with departure vector v the gain of band b is
 *     g_b = (1 - shape_b) + shape_b * dot3(normalize3(normalize3(v)), normalize3(direction))
 * — the expression of kernel `attenuate` (kernel.cpp:505-513, speaker_gain in csrc/attenuation.h), double normalisation included, one
 * IEEE binary32 operation per operator in the order written; normalize3(direction) is taken once on the host with the device's operations.
 *   - diffuse impulses:               v = the ray's own direction (the entry of rvb_set_directions the record's ray was traced with);
 *   - image-source impulses, direct:  v = mic - position, component by component in binary32.  The trace stores
 *                                     position = mic + (source - mic_reflection), so mic - position is the direction in which the image
 *                                     ray leaves the real source, up to the rounding of that one addition; taking v from the record
 *                                     alone makes the gain a pure function of (record, microphone, ray direction).
 * The stored impulse becomes volume_b = volume_b * g_b: ONE multiply per band after everything the trace computes without a pattern,
 * applied to every diffuse Impulse the shadow pass wrote, to every image-source candidate and to the direct slot, each exactly once.
 * Nothing else changes: rvb_get_diffuse, rvb_get_direct, rvb_get_image_candidates, the materialised attenuators, RVB_IR_FAST and
 * RVB_IR_EXACT, the wide speaker fold and the HRTF model all see the scaled records.  An impulse whose eight scaled volumes are all
 * zero (a null of the pattern, or underflow) is a zero-volume impulse from then on (quirk Q2): the diffuse time range of the trace —
 * what rvb_ir_time_range returns for the speaker model, per pair after rvb_trace_pairs — is that of the SCALED records.
 *
 * npatterns == 0 (or patterns == NULL): off — the default; no extra launch, every byte and every kernel as without this call.
 * npatterns == 1: that pattern for every pair of the traces that follow (rvb_trace, rvb_trace_pairs, rvb_trace_group: every context
 * has its own).  npatterns == n: pattern p for pair p of rvb_trace_pairs, which fails with RVB_ERR_INVALID unless n is 1 or its npairs;
 * rvb_trace and rvb_trace_group take n == 1 only.  The patterns are copied.  RVB_ERR_INVALID for a non-finite value or a zero-length
 * direction.  Cost: one streaming pass over the records behind the shadow kernel ("source_pattern_kernel" in rvb_last_timings). */
typedef struct { float direction[4]; float shape[8]; } rvb_source_pattern;               /* 48 B */
int rvb_set_source_pattern(rvb_ctx * ctx, const rvb_source_pattern * patterns, uint64_t npatterns);

/* ---- tabulated source directivity: a per-band gain table at the SOURCE end (csrc/source_kernels.hip) -------------------------------
 * The twin of the HRTF table at the other end of the path, for a loudspeaker balloon: measured gain per octave band over azimuth and
 * elevation.  No reference counterpart for the stage; the row selection is the reference's own.
 *
 * LAYOUT.  `table` has the layout of ONE ear of the HRTF table (rvb_ir_configure_hrtf): row a * 180 + e, a = 0 .. 359, e = 0 .. 179, eight
 * band gains per row; [360*180*8] floats, copied.  On the device it is followed by one zero row, row 64800.
 *
 * CONTRACT.  For an impulse with departure vector v the selected row is
 *     row_of(to_listener(basis(facing, up), normalize3(v)))
 * — exactly the expression of the reference's kernel `hrtf` (kernel.cpp:538-584, hrtf_row in csrc/attenuation.h) with pos - mic replaced
 * by v: x = normalize3(cross3(up, facing)), y = cross3(facing, x), z = facing; a = (long) (degrees(atan2(t.x, t.z)) + 180) % 360,
 * e = 90 - (long) degrees(atan2(t.y, sqrt(t.x^2 + t.z^2))), the quirk by which e == 180 runs into the next azimuth row included, and with
 * the margin scheme of angle_deg, so that the integer parts are those of the correctly rounded binary32 atan2.  facing and up are taken
 * as given, as rvb_ir_configure_hrtf takes them (facing[3], up[3] ignored); the basis is computed once on the host with the device's
 * operations.  The departure vector is that of a pattern:
 *   - diffuse impulses:               v = the ray's own direction;
 *   - image-source impulses, direct:  v = mic - position, component by component in binary32.
 * The stored impulse becomes volume_b = volume_b * table[row][b]: ONE binary32 multiply per band, applied to every diffuse record, every
 * image-source candidate and every direct slot exactly once.  An impulse whose eight scaled volumes are all zero is a zero-volume
 * impulse from then on, and the per-pair diffuse time range is that of the SCALED records.  An index outside 0 .. 64800 reads the zero
 * row: finite inputs cannot produce one, but no address outside the table is ever formed.
 *
 * norientations == 1: that orientation for every pair.  norientations == n: orientation p for pair p of rvb_trace_pairs; as with
 * patterns the trace (or re-shade) fails with RVB_ERR_INVALID unless n is 1 or its npairs.  The table itself is one per context.
 *
 * ONE DIRECTIVITY SLOT.  A source has one directivity at a time: a call with a table turns any pattern off; table == NULL (orientations
 * and count are then ignored) turns the table off; ANY call of rvb_set_source_pattern turns the table off, the one with npatterns == 0
 * included, which still means "nothing at the source end".  With the table off there is no extra launch and no extra allocation: every
 * byte and every kernel as without this call.
 *
 * RVB_ERR_INVALID, before any device is touched: a NULL ctx; a table with orientations NULL or count 0; a value in table, facing or up
 * that is not finite; an orientation whose normalize3(cross3(up, facing)) is zero or not finite.
 *
 * UPLOAD.  Lazily, in stream order, by the next trace or re-shade, through a staging block as the patterns are.  A table set after a kept
 * trace is therefore NOT what rvb_relisten uses: relisten uses what the records reflect now — pattern, table or nothing, as the kept
 * trace or the last rvb_reshade left them — and reuses the per-ray gains, which do not depend on the microphone; rvb_reshade applies
 * what is set now; rvb_reshade_grad takes a ray's gain as a factor of every term of that ray, where a pattern's gain enters.
 * KERNELS.  The diffuse gain depends on (pair, ray) only, never on the bounce: "source_table_rays_kernel" selects one row per (pair, ray)
 * and leaves its 32 bytes in a buffer of the context (32 bytes per (pair, ray)); "source_table_kernel" is the streaming pass over the
 * records, shaped like "source_pattern_kernel", followed by the candidates and direct slots, one lane and one row selection each.
 * SCOPE.  Contexts only, through rvb_trace, rvb_trace_pairs, rvb_trace_group, rvb_reshade, rvb_relisten and rvb_reshade_grad; not
 * offered through rvb_multi_* and rvb_pipeline_* in this version.  One table per context; no interpolation between rows (the reference's
 * table semantics are nearest-cell by truncation; resample on the host).
 * MEASURED on one MI355X at 100 k rays x 128 in the 75 k-triangle cathedral (profiles/source_table_n1.txt, tools/source_table_bench.py;
 * medians, all in one run):
 *     rvb_trace with the directivity off 4.53 ms (the commit before this feature: 4.51 ms, its repetitions spread over 0.15 ms); with a
 *     polar pattern 4.99 ms, source_pattern_kernel 0.465 ms; with a table 4.95 ms — source_table_rays_kernel 0.007 ms for the 100 k row
 *     selections, source_table_kernel 0.417 ms (3.9 TB/s of 128 bytes per record; the pattern pass 3.5 TB/s): not slower than the polar
 *     pass, the difference of 0.05 ms is inside that kernel's own spread. */
typedef struct { float facing[4]; float up[4]; } rvb_source_orientation;     /* [3] ignored */
int rvb_set_source_table(rvb_ctx * ctx, const float * table /* [360*180*8] */,
                         const rvb_source_orientation * orientations, uint64_t norientations);

/* ---- re-shading a finished trace: new surfaces and a new air coefficient without retracing (csrc/reshade_kernels.hip) -------------
 * Everything a trace spends its time on — the closest-hit / reflect chain, the shadow rays, the image-source validation, every
 * position, distance and arrival time — depends on geometry, microphone, source and directions only.  Surfaces and air enter in three
 * places of the reference (kernel.cpp:461, :480-485, :260).  A caller that sweeps materials in a fixed room (reference chain
 * cmd/main.cpp:241-298 once per material set) traces ONCE with keeping on and then calls rvb_reshade per material set: one streaming
 * pass over the records instead of rvb_set_scene + rvb_trace.  No reference counterpart for the calls themselves.
 *
 * rvb_keep_paths(ctx, 1): from now on the traces of this context (rvb_trace, rvb_trace_pairs, rvb_trace_group) keep what rvb_reshade
 * needs: per (ray, bounce) a 16-byte side record {newDist, DIFF, surface, spare} written by one more streaming kernel between the path
 * and the shadow stage ("path_keep_kernel" in rvb_last_timings), and one float per image-source candidate and direct slot (INIT_DIST,
 * which cannot be recovered from an impulse's time or position).  Keeping never changes what a trace returns.  Memory: 16 bytes per
 * (ray, bounce) — 205 MB beside the 819 MB of records at 100 k rays x 128 —, allocated by the first trace made with keeping on.
 * rvb_keep_paths(ctx, 0), the default: no extra launch, no extra allocation, every byte and every kernel as without this call; the side
 * buffers of an earlier keep are freed (after waiting for the context's stream) and rvb_reshade fails until the next kept trace.
 * `keep` is a set of bits: RVB_KEEP_MATERIALS (1) is the above, exactly; with RVB_KEEP_LISTENER (2) set a trace keeps everything that 1
 * keeps and in addition what rvb_relisten (below) needs: see there.
 *
 * rvb_reshade(ctx, surfaces, nsurfaces, air_coefficient), after a trace made with keeping on: the context is left in the state that
 * rvb_trace / rvb_trace_pairs would have left with the same microphones, sources, directions, nreflections and ray_offset on a scene
 * whose surface table is `surfaces` and with `air_coefficient`:
 *   - every byte of the diffuse records (volume, position, time, padding), of the direct slot(s) and of the image-source candidates,
 *     and the per-pair diffuse time range that rvb_ir_time_range reports for the speaker model, equal that trace's;
 *     rvb_executed_bounces is unchanged;
 *   - surfaces == NULL: the scene's own table (only the air changes); otherwise nsurfaces must equal the scene's (RVB_ERR_INVALID).
 *     Values are taken as rvb_set_scene takes them (the triangles' surface indices were validated there; coefficients are not inspected);
 *   - the scene stays as it is (it may be shared, rvb_share_scene): the next rvb_trace uses the scene's own surfaces.  The table is copied
 *     into a buffer of the context; the caller's array is free on return;
 *   - repeatable in any order: every call starts from the kept numbers, never from the volumes the records hold.  Re-shading with A,
 *     then B, then the scene's own surfaces and the trace's own air returns the original trace bit for bit;
 *   - with a source pattern set (rvb_set_source_pattern) the re-shaded records are scaled and the time range taken again, as a trace does;
 *   - like a trace it voids the IR configuration and a prepared exact list (rvb_ir_configure_* again; rvb_ir_select_pair is back at 0);
 *   - asynchronous on the context's stream; timed as "reshade_kernel" and "reshade_images_kernel" in rvb_last_timings.
 * ARITHMETIC, one IEEE binary32 operation per operator in the order written, with the trace's own functions: for ray r, bounce k
 *     vol_b(k) = -vol_b(k-1) * specular[surface(k)][b], vol_b(-1) = 1                                    (kernel.cpp:461)
 *     dist     = visible ? newDist(k) + length3(mic - position(k)) : 0                                  (kernel.cpp:471)
 *     volume_b = visible ? ((vol_b(k) * (air_attenuation(dist, air_b) * 1.0f)) * diffuse[surface(k)][b]) * DIFF(k) : 0
 * where `visible` is what the shadow stage found (the record's time is non-zero exactly then); an image-source candidate in slot s gets
 * vol_b(s-2) * (air_attenuation(INIT_DIST, air_b) * 1.0f) with the chain over the ray's first s - 1 triangles, the direct slot
 * 1 * (air_attenuation(INIT_DIST, air_b) * 1.0f) (kernel.cpp:260).
 * RVB_ERR_STATE: nothing traced, the last trace was made without keeping, or rvb_set_scene / rvb_share_scene / rvb_set_directions* came
 * since.  RVB_ERR_HIP with the runtime's text when a buffer cannot be allocated (rvb_trace for the side buffers).  A failed call
 * leaves the results as they were.  Not offered by rvb_multi_* and rvb_pipeline_*: a sweep is a loop on one context.
 * MEASURED on one MI355X at 100 k rays x 128 in the 75 k-triangle cathedral (profiles/reshade_n1.txt, tools/reshade_bench.py; medians):
 *     rvb_trace, keeping off 4.49 ms (the commit before this feature: 4.65 ms, its repetitions spread over 0.20 ms); keeping on 4.80 ms,
 *     path_keep_kernel 0.335 ms (3.6 x its floor of 48 bytes per record at 6.6 TB/s: it fetches whole 64-byte records);
 *     rvb_reshade 0.63 ms — reshade_kernel 0.58 ms beside shadow_pair_kernel's 1.24 ms — against 47.6 ms for rvb_set_scene + rvb_trace. */
enum { RVB_KEEP_MATERIALS = 1, RVB_KEEP_LISTENER = 2 };
int rvb_keep_paths(rvb_ctx * ctx, int keep);
int rvb_reshade(rvb_ctx * ctx, const rvb_surface * surfaces, uint64_t nsurfaces, const float air_coefficient[8]);

/* ---- a new microphone on a kept trace without the path stage (csrc/relisten_kernels.hip) ------------------------------------------
 * The closest-hit / reflect chain of the reference (kernel.cpp:359-375, :459-461, :478, :492-501) never reads the microphone: hit
 * points, newDist, DIFF, triangles and the specular volume chain depend on scene, source and directions only.  The microphone enters in
 * the shadow ray of every record (:463-490), the image-source validation (:379-457) and the direct path (:335-357).  A caller that maps
 * one source over a grid of listeners traces ONCE with RVB_KEEP_LISTENER and then calls rvb_relisten per listener: one streaming pass
 * that puts the path stage's work records back, then the shadow and image stages of a trace as they are.  No reference counterpart.
 *
 * rvb_keep_paths(ctx, RVB_KEEP_MATERIALS | RVB_KEEP_LISTENER): the traces that follow keep, beside the side records of rvb_reshade, the
 * two words of a work record that nothing else recovers — the own-plane threshold of the shadow ray and the triangle —, written by the
 * same "path_keep_kernel".  Memory: 8 bytes per (ray, bounce) beside the 16 kept for re-shading — 102 MB at 100 k rays x 128 —, allocated
 * by the first such trace.  The grouping order of the records (4 bytes per (ray, bounce), which every trace allocates and fills) stays
 * where the trace left it: only a trace's grouping writes it, and the next trace voids the kept state.  Where the trace grouped nothing
 * (RVB_SHADOW_SORT=0, or 2^32 or more records) the shadow rays of a relisten run in natural order, as that trace's did.
 *
 * rvb_relisten(ctx, mics, npairs) — mics: [npairs][3]; npairs must equal that of the kept trace (1 after rvb_trace / rvb_trace_group):
 * the context is left in the state that rvb_trace / rvb_trace_pairs would have left with the new microphone(s), the same sources,
 * directions, nreflections and ray_offset, and the surface table, air and source patterns that the records reflect now (the scene's own
 * after a kept trace, those of the last rvb_reshade after one):
 *   - every byte of the diffuse records (padding too), of the direct slot(s) and of the image-source candidates as
 *     rvb_get_image_candidates returns them, and the per-pair diffuse time range equal that trace's; rvb_executed_bounces is unchanged;
 *   - like a trace it voids the IR configuration and a prepared exact list (rvb_ir_configure_* again; rvb_ir_select_pair is back at 0);
 *   - the kept trace stays valid and is now that of the new microphone(s), the kept image distances included: later rvb_reshade,
 *     rvb_reshade_grad and rvb_relisten calls work from there.  Repeatable in any order: A, B, C, then A again returns the original
 *     trace bit for bit;
 *   - asynchronous on the context's stream; rvb_last_timings: "relisten_records_kernel", "image_kernel", the shadow kernel's name and,
 *     with a source pattern, "source_pattern_kernel" — no path kernel and no record grouping.
 * RVB_ERR_INVALID (before any device is touched) for a NULL ctx or mics, a coordinate that is not finite, npairs other than the kept
 * trace's.  RVB_ERR_STATE, with a text that names the condition: nothing traced, the last trace made without RVB_KEEP_LISTENER, or
 * rvb_set_scene / rvb_share_scene / rvb_set_directions* since.  A failed call leaves the results as they were.
 * SCOPE.  One context; not offered by rvb_multi_* and rvb_pipeline_*, as rvb_reshade is not: a listener grid is a loop on one context.
 * MEASURED on one MI355X at 100 k rays x 128 in the 75 k-triangle cathedral (profiles/relisten_n1.txt, tools/relisten_bench.py; medians):
 *     rvb_trace, keeping off 4.50 ms (the commit before this feature: 4.48 ms, its repetitions spread over 0.11 ms); RVB_KEEP_MATERIALS
 *     4.79 ms, with RVB_KEEP_LISTENER 4.76 ms (path_keep_kernel 0.335 -> 0.343 ms: the 8 more bytes are not measurable in the trace);
 *     rvb_relisten 1.83 ms — relisten_records_kernel 0.46 ms, image_kernel 0.10 ms, shadow_pair_kernel 1.20 ms — against 4.49 ms for
 *     rvb_trace with the new microphone: 2.45 x.  With the kept grouping order ignored (natural order) 2.33 ms, the shadow kernel 1.70 ms. */
int rvb_relisten(rvb_ctx * ctx, const float * mics, uint64_t npairs);

/* ---- material gradients of a weighted impulse response from a kept trace (csrc/reshade_grad_kernels.hip) ---------------------------
 * The other half of a material sweep: a fit of absorption coefficients (or of the air) to a measured decay needs a gradient, and by
 * finite differences that is 16 x nsurfaces + 8 re-shades and binnings per step.  Everything the analytic gradient needs is in the
 * context after a kept trace: the side records, the records' positions and times, the current table and air, the speaker model.
 * No reference counterpart.
 *
 * THE QUANTITY.  H = what rvb_ir_accumulate(ctx, predelay, sample_rate, nbins, RVB_IR_FAST, zeroed) adds for the current records of the
 * selected pair (rvb_ir_select_pair) under the configured speaker model: every live diffuse record i adds speaker_gain_c(i) * volume_b(i)
 * to bin time_bin(time_i, predelay, sample_rate) of row (c, b); records whose bin is >= nbins are skipped.  With the weights w in the
 * histogram's own layout [nchannels][8][nbins] (device memory), L = sum_{c,b,bin} w[c][b][bin] * H[c][b][bin], and the call returns
 *     grad_surfaces[s].specular[b] = dL/dspecular[s][b],  grad_surfaces[s].diffuse[b] = dL/ddiffuse[s][b]   (host, the scene's nsurfaces)
 *     grad_air[b] = dL/dair_b                                                                                (host; may be NULL)
 * taken at the surface table, air and source pattern that the records reflect now: the scene's own table and the trace's air after a
 * kept trace, those of the last rvb_reshade after one.  A least-squares fit passes its residual, w = 2 (H - H_target).
 * H is taken as the polynomial in the coefficients that rvb_reshade's ARITHMETIC writes down (with d air_attenuation / d air =
 * dist * ln((float) M_E) * air_attenuation): a record whose volume is 0 because a coefficient is 0 still has its derivative.
 *   - the call never divides by a coefficient: per (ray, band), with P_k = vol_b(k), a_k = air_attenuation * DIFF * pattern gain *
 *     sum_c w[c][b][bin_k] * gain_c(k) (0 for an invisible or skipped record),
 *         dL/ddiffuse[s_k][b] += P_k a_k,   dL/dair_b += P_k a_k diffuse[s_k][b] dist_k ln((float) M_E),
 *         dL/dspecular[s_j][b] += -P_{j-1} B_j,   B_j = a_j diffuse[s_j][b] + (-specular[s_{j+1}][b]) B_{j+1};
 *   - with a source pattern set, band b's gain of the ray's own direction is a factor of every term of that ray;
 *   - a surface that no live record of the pair touches gets exactly 0; slots behind an escape and invisible records add nothing;
 *   - terms in binary32 with the trace's own functions; sums over records and rays in binary64, in a fixed order (a table per
 *     workgroup, no atomics; the tables added in a fixed order), rounded to float once: the error does not grow with the ray count and
 *     two calls return identical bytes.
 * SCOPE of this version.  Diffuse records only: the IR configuration must be rvb_ir_configure_speakers with which == RVB_IR_DIFFUSE and
 * 1 to 8 channels.  RVB_ERR_STATE, with a text that names the condition, for anything else (the HRTF model, RVB_IR_IMAGES or RVB_IR_ALL,
 * more than 8 channels, no configuration — rvb_reshade voids it: configure again) and where rvb_reshade itself would return
 * RVB_ERR_STATE (no kept trace; the scene or the directions changed since).  RVB_ERR_INVALID for a NULL ctx (before any device is
 * touched), d_weights or grad_surfaces, nbins == 0, a predelay or sample rate that is not finite.  RVB_ERR_CAPACITY above 2048
 * reflections (a ray's chain checkpoints live in LDS).  Image-source gradients are a follow-up (the merged list has lost its chains), as
 * are the HRTF model and more than 8 channels; not offered by rvb_multi_* and rvb_pipeline_*, as rvb_reshade is not.
 * CALLING.  Synchronous: waits for the context's stream and fills the host arrays.  Changes no byte of the records, of the direct slot,
 * of the candidates or of the time range; the IR configuration stays.  Uses the accumulation image's scratch for the transposed weights
 * (rvb_ir_accumulate may be called again afterwards as before).  rvb_last_timings: "reshade_grad_weights_kernel" (the weights into the
 * accumulation image's layout [bin][channel][band]: a record gathers one run of 32 x nchannels bytes), "reshade_grad_kernel",
 * "reshade_grad_reduce_kernel".  A failed call leaves everything as it was.  A scene of more than 64 surfaces is swept once per 64.
 * MEASURED on one MI355X at 100 k rays x 128 in the 75 k-triangle cathedral, 7 surfaces, stereo speakers, 846 731 bins
 * (profiles/reshade_grad_n1.txt, tools/reshade_grad_bench.py; medians of one run): rvb_reshade_grad 1.81 ms — reshade_grad_kernel 1.71 ms,
 *     reshade_grad_weights_kernel 0.026 ms, reshade_grad_reduce_kernel 0.023 ms — beside rvb_reshade 0.63 ms and rvb_ir_accumulate
 *     (RVB_IR_FAST) 0.61 ms: 1.46 forward evaluations, where finite differences take 16 x 7 + 8 = 120 of them (148 ms).  Neither the
 *     side records nor the weights bound it (0.36 TB/s of record bytes); the rest is arithmetic, one binary64 exponential per record
 *     and band and the fixed-order combine of the rays' terms (no counter run has been made). */
int rvb_reshade_grad(rvb_ctx * ctx, float predelay, float sample_rate, uint64_t nbins, const void * d_weights, rvb_surface * grad_surfaces,
                     float grad_air[8]);

/* ---- sensitivity map: the material gradients per TRIANGLE (csrc/reshade_grad_map_kernels.hip) --------------------------------------
 * rvb_reshade_grad says which coefficients matter; a room designer asks WHERE on the walls treatment changes this decay at this seat.
 * That is the same derivative kept per triangle instead of summed per surface.  A trace kept with RVB_KEEP_LISTENER holds what it takes:
 * the listener record beside the side record names the triangle of every (ray, bounce).  No reference counterpart.
 *
 * THE QUANTITY.  L is exactly the L of rvb_reshade_grad — the same H, the same weights layout [nchannels][8][nbins] (device memory), the
 * same selected pair, the same table, air and source directivity that the records reflect now.  Triangle t is treated as if it owned a
 * private copy of its surface's coefficients; with the terms of rvb_reshade_grad above,
 *     d_map[t].specular[b] = sum over the records (ray, j) with triangle_j == t of -P_{j-1} B_j
 *     d_map[t].diffuse[b]  = sum over the records (ray, k) with triangle_k == t of  P_k a_k
 * so that in exact arithmetic the entries of the triangles of a surface add up to that surface's grad_surfaces.  d_map is device memory,
 * [ntriangles] rvb_surface, t the caller's triangle index as passed to rvb_set_scene (ntriangles must be the scene's).  There is no
 * air derivative here: rvb_reshade_grad has it.
 *   - every term is the binary32 value rvb_reshade_grad forms, by the same device code (one kernel body, two places for a term); the
 *     call never divides by a coefficient;
 *   - the sums per triangle are binary64, rounded to float once.  The records of a triangle are taken in ascending (ray, bounce) order —
 *     a stable sort by triangle of (triangle, record number) —, cut by position in the sorted list: tiles of RVB_GRAD_MAP_TILE entries,
 *     16 segments per tile; a segment's records one after the other, a run's segments one after the other, its tiles one after the
 *     other.  No atomics, nothing depends on the order of dispatch: two calls return identical bytes, and the bytes do not depend on
 *     the surface numbers;
 *   - EVERY entry is written: exactly 0.0 in all 16 slots for a triangle that no live record of the pair touches, for one that lies
 *     behind an escape only and for one the BVH builder dropped.
 * SCOPE and errors mirror rvb_reshade_grad, each with a text that names the condition.  RVB_ERR_INVALID, before any device is touched,
 * for a NULL ctx, d_weights or d_map, nbins == 0, a predelay or sample rate that is not finite, ntriangles other than the scene's, d_map
 * overlapping d_weights.  RVB_ERR_STATE for nothing traced, a last trace made without RVB_KEEP_LISTENER, the scene or the directions
 * changed since, no IR configuration, the HRTF model, which != RVB_IR_DIFFUSE, more than 8 channels.  RVB_ERR_CAPACITY above 2048
 * reflections and for nrays * nreflections >= 2^32 in the pair (record numbers are 32-bit sort values).  A failed call writes nothing
 * and leaves everything as it was.  Image-source and direct-sound terms, the HRTF model and more than 8 channels are out of scope; not
 * offered by rvb_multi_* and rvb_pipeline_*, like the rest of the family.
 * CALLING.  Asynchronous on the context's stream, like rvb_decay_curve.  Changes no byte of the records, of the direct slot, of the
 * candidates or of the time range; the IR configuration stays.  It works after rvb_reshade and after rvb_relisten (the listener records
 * do not depend on the microphone).  It uses the sort buffers, so like rvb_ir_accumulate it voids a prepared exact list
 * (rvb_ir_exact_fold then returns RVB_ERR_STATE), and the accumulation image's scratch for the transposed weights, as the gradient does.
 * Its own scratch is one term row of 64 bytes per record of the pair (and 256 bytes per tile of the fold): 819 MB at 100 k x 128.  It
 * lives with the kept buffers, is allocated by the first call and freed by rvb_keep_paths(ctx, 0).  No table per triangle is kept per
 * workgroup: nothing but d_map grows with the triangle count.  rvb_last_timings: "reshade_grad_weights_kernel",
 * "reshade_grad_map_terms_kernel" (reshade_grad_kernel's sweep; a record's 16 terms go to its row, stored as whole 64-byte rows),
 * "reshade_grad_map_sort" (the stable sort and the run boundaries), "reshade_grad_map_fold_kernel", "reshade_grad_map_combine_kernel".
 * MEASURED on one MI355X at 100 k rays x 128, stereo speakers (profiles/reshade_grad_map_n1.txt, tools/reshade_grad_map_bench.py; medians of
 * one run, calls by the host clock to the synchronisation): in the 75 252-triangle cathedral rvb_reshade_grad_map 2.56 ms —
 *     reshade_grad_map_terms_kernel 1.75 ms, reshade_grad_map_sort 0.42 ms, reshade_grad_map_fold_kernel 0.30 ms, the weights 0.03 ms, the
 *     combine 0.01 ms — where rvb_reshade_grad on the scene relabelled with one surface per triangle takes 60.5 s (1 176 sweeps, each on
 *     the 64 workgroups whose tables fit its scratch); in the 3 006-triangle one 2.44 ms (sort 0.30 ms) against 832 ms (47 sweeps).  The
 *     terms pass bounds the call, and arithmetic bounds the terms pass as it bounds rvb_reshade_grad (1.62 ms): its 128 bytes per
 *     record are 0.94 TB/s against a floor of 0.25 ms at 6.6 TB/s.  The fold gathers its 72 bytes per record at 3.1 TB/s (floor
 *     0.14 ms), the sort stands at 0.42 ms over a floor of 0.09 ms for three passes of 17 key bits.  rvb_trace with keeping on and
 *     rvb_reshade_grad stand 0.06 - 0.07 ms and 0.015 ms from the parent commit's, inside the spread of its repetitions (0.09 - 0.10 ms,
 *     0.04 - 0.05 ms); the device code of the trace is the parent's line for line. */
#define RVB_GRAD_MAP_TILE 1024    /* sorted entries per workgroup tile of the fold; tests choose their edge shapes from it */
int rvb_reshade_grad_map(rvb_ctx * ctx, float predelay, float sample_rate, uint64_t nbins, const void * d_weights,
                         void * d_map /* device, [ntriangles] rvb_surface */, uint64_t ntriangles);

/* ---- decay curves: Schroeder integral, reverberation times, the loss against a measured decay and its adjoint (csrc/decay_kernels.hip) ---
 * What a fit of materials to a measured decay needs between rvb_ir_accumulate, which leaves the histogram H on the device, and
 * rvb_reshade_grad, which takes w = dL/dH: the energy decay curve of every row, a loss L against a target decay, and w.  Nothing leaves
 * the device but a few numbers per row.  No reference counterpart (the reference has no decay analysis).
 *
 * All three calls work on the caller's own device arrays of nrows rows of nbins floats, row r at element r * nbins; a histogram
 * [nchannels][8][nbins] is nrows = 8 * nchannels.  They use the context for its device, stream, scratch and timings only: no scene, trace
 * or IR configuration is needed, none of them voids an IR configuration or a prepared exact list or touches a record, and their scratch
 * is a block of its own in the context, grown on demand (never the sort buffers).
 * THE ORDER of every sum is fixed by the bin numbers alone.  A row is cut into tiles of RVB_DECAY_TILE bins; every call is a launch that
 * leaves one binary64 value per tile, a launch in which one wave per row combines the row's tiles one after the other, and a launch that
 * scans every tile again on top of its carry.  No atomics, no hand-off between workgroups inside a launch, no dependence on dispatch
 * order: this fixed order makes two calls return identical bytes.  Sums and logarithms are binary64; a result is rounded to float once.
 *
 * rvb_decay_curve   E[r][k] = sum_{j >= k} H[r][j]^2, the Schroeder integral: the squares (exact in binary64) and the sums in binary64,
 *                   per tile, then the tiles of a row from the last to the first, then every tile from its last bin to its first on top
 *                   of its carry.  |E - exact| <= one float ulp; E is exactly 0 where every later bin of H is 0.  Values are not
 *                   inspected.  d_curve is [nrows][nbins] float and must not overlap d_histogram (RVB_ERR_INVALID).  Asynchronous on the
 *                   context's stream.
 * rvb_decay_times   seconds[r] = the reverberation time of row r of a curve E, extrapolated to 60 dB from the range db_begin .. db_end
 *                   (-5, -35: T30; -5, -25: T20; 0, -10: the early decay time).  In binary64: level[k] = 10 log10(E[k] / E[0]); k0 is the
 *                   first k with level <= db_begin, k1 the first k with level < db_end, both found by comparing E[k] with
 *                   E[0] * 10^(db / 10), not through a logarithm per bin (a bin with E = 0 is below every level; E does not increase,
 *                   so [k0, k1) is one run).  The least-squares line of level over x = k - k0, x centred on the window, has
 *                   slope = sum (x - mean x) level / sum (x - mean x)^2 in dB per bin, the first sum over the bins in the fixed order,
 *                   the second in closed form; seconds = -60 / (slope * sample_rate).  The result is a quiet NaN — the "not available"
 *                   value — for a row with E[0] == 0, with fewer than 2 bins in the window, or whose curve never falls below db_end
 *                   inside nbins.  Synchronous.  RVB_ERR_INVALID unless db_end < db_begin <= 0 with both finite, and sample_rate finite
 *                   and > 0.
 * rvb_decay_loss    the loss against a target decay T (linear energy, [nrows][nbins] float) under a mask m ([nrows][nbins] float,
 *                   m >= 0: the caller zeroes what lies outside its evaluation range), with E the output of rvb_decay_curve for H or the
 *                   caller's own curve.  Bin k of row r counts when m > 0, E > 0 and T > 0; with RVB_DECAY_NORMALISED in `flags` a row
 *                   counts only when E[r][0] > 0 and T[r][0] > 0, and both curves are taken relative to their first bin:
 *                       d[k] = ln E[k] - ln T[k] - (normalised ? ln E[0] - ln T[0] : 0)
 *                       loss_rows[r] = sum_k m[k] d[k]^2                       (host; dB^2: scale by (10 / ln 10)^2)
 *                       g[k] = 2 m[k] d[k] / E[k], with the flag g[0] -= (sum_k 2 m[k] d[k]) / E[0]
 *                       w[r][j] = 2 H[r][j] * sum_{k <= j} g[k] = dL/dH[r][j]   (d_weights, device, H's layout)
 *                   — exactly the weights rvb_reshade_grad takes for L = sum_r loss_rows[r].  Everything in binary64 in the fixed order;
 *                   w is rounded to float once, is exactly 0 where H is 0 and in rows that do not count (their loss is 0), and no entry
 *                   is left unwritten.  d_weights == NULL: the loss only.  d_weights must not overlap any of the four inputs
 *                   (RVB_ERR_INVALID).  Synchronous.
 * ALL THREE: RVB_ERR_INVALID for a NULL ctx (before any device is touched), a NULL required pointer, nrows == 0 or nbins == 0;
 * RVB_ERR_CAPACITY for nrows > 4096 (and for 2^32 bins or more).  A failed call writes nothing.  rvb_last_timings names the kernels
 * of the last decay call: "decay_curve_sums_kernel", "decay_curve_carry_kernel", "decay_curve_scan_kernel"; "decay_times_find_kernel",
 * "decay_times_window_kernel", "decay_times_sums_kernel", "decay_times_fit_kernel"; "decay_loss_sums_kernel", "decay_loss_carry_kernel",
 * "decay_loss_scan_kernel" (the last only with d_weights).
 * MEASURED on one MI355X (profiles/decay_n1.txt, tools/decay_bench.py; medians of one run, calls by the host clock to the synchronisation,
 * kernels by HIP events), at workload C2's stereo histogram, 16 x 846 741, and at 512 x 846 741 (64 channels):
 *     rvb_decay_curve           0.085 ms / 0.93 ms — its three kernels 0.051 ms / 0.88 ms against a floor of 0.025 ms / 0.79 ms (H read
 *                               twice, E written once, 6.6 TB/s): at C2 launch overhead is most of the call, at 512 rows the kernels
 *                               run at 0.9 of the floor.  The float64 flip-cumsum-flip of the squares in torch on the same GPU, in the
 *                               same run: 2.14 ms / 8.9 ms (25 x / 9.6 x the call); the pinned download of the histogram, which a host-side
 *                               computation needs first: 0.96 ms / 30.4 ms;
 *     rvb_decay_times (T30)     0.127 ms / 1.45 ms (decay_times_sums_kernel, a binary64 logarithm per bin of the window: 0.045 / 1.05 ms);
 *     rvb_decay_loss            0.211 ms / 4.64 ms with weights, 0.120 ms / 2.37 ms without — kernels 0.167 ms / 4.58 ms against a floor of
 *                               0.066 ms / 2.10 ms (E, T, m read twice, H once, w written once): the two binary64 logarithms per
 *                               counting bin, taken in both passes, bound it, not the bytes (no counter run has been made). */
#define RVB_DECAY_TILE 4096      /* bins per workgroup tile of the decay kernels (tests choose their edge shapes from it) */
enum { RVB_DECAY_NORMALISED = 1 };
int rvb_decay_curve(rvb_ctx * ctx, const void * d_histogram, uint64_t nrows, uint64_t nbins, void * d_curve);
int rvb_decay_times(rvb_ctx * ctx, const void * d_curve, uint64_t nrows, uint64_t nbins, float sample_rate,
                    float db_begin, float db_end, float * seconds /* host [nrows] */);
int rvb_decay_loss(rvb_ctx * ctx, const void * d_histogram, const void * d_curve, const void * d_target, const void * d_mask,
                   uint64_t nrows, uint64_t nbins, unsigned flags, double * loss_rows /* host [nrows] */, void * d_weights);

/* ---- room acoustic parameters: EDT, T20, T30, C50, C80, D50, Ts of a curve, a loss against a measured table, its adjoint
 *      (csrc/decay_params_kernels.hip) ---------------------------------------------------------------------------------------------------
 * A room survey supplies the ISO 3382-1 single numbers per octave band, not a decay curve.  rvb_decay_params computes all seven for
 * every row of a curve E in ONE sweep; rvb_decay_params_loss adds a weighted squared loss against a table of targets and the adjoint
 * w = dL/dH, exactly the weights rvb_reshade_grad and rvb_reshade_grad_map take — the form rvb_decay_loss produces.  Shapes, row layout,
 * scratch rules and the determinism promise are those of the decay calls above: any array of rows of bins; the context's device, stream,
 * timings and decay scratch only; no scene, trace or IR configuration is needed, nothing is voided and no record is touched; all sums and
 * logarithms are binary64 in an order fixed by (tile, chunk, bin); no atomics; each result is rounded to float once; two calls return
 * identical bytes.  Both calls are synchronous.  No reference counterpart.
 *
 * DEFINITIONS.  All arithmetic is binary64 on the float32 values of E; fs is sample_rate widened to double; C10 = 10 / ln 10; the
 * "not available" value is a quiet NaN.
 *   EDT, T20, T30   exactly rvb_decay_times with (0, -10), (-5, -25), (-5, -35): the same thresholds, window [k0, k1), centred line and
 *                   -60 / (slope * fs).  For every row the three floats are byte-equal to what rvb_decay_times returns for that pair.
 *   C50, C80        ke = (uint64_t) (te * fs + 0.5), te the double literal 0.05 or 0.08; early = E[0] - E[ke], late = E[ke];
 *                   C = C10 (ln early - ln late), in dB.  NaN unless E[0] > 0, ke < nbins, early > 0 and late > 0.
 *   D50             D = (E[0] - E[k50]) / E[0].  NaN unless E[0] > 0 and k50 < nbins.
 *   Ts              Ts = (sum_{k=1}^{nbins-1} E[k]) / (fs E[0]) = sum_j (j / fs) H_j^2 / sum_j H_j^2, the centre time with bin j at time
 *                   j / fs, in seconds.  NaN unless E[0] > 0.
 * LOSS.  Parameter p of row r counts when param_weights[r][p] > 0 and the model's value q (binary64, before its rounding to float) is
 * finite; loss_rows[r] = sum_p weight (q - target)^2 over the counting parameters, in the order of the parameter numbers (a weight of
 * 1 / target^2 gives relative errors).  An unavailable model value adds nothing; the caller sees it in `params`.
 * ADJOINT.  With c_p = 2 weight (q - target) (0 when p does not count), g[k] = dL/dE[k] is the sum of
 *   each time p, window [k0, k1), slope s, n = k1 - k0, Sxx = n (n^2 - 1) / 12, xc_k = (k - k0) - (n - 1) / 2:
 *                   for k in the window  c_p (60 / (s^2 fs)) C10 xc_k / (Sxx E[k])   (the E[0] terms of the levels cancel: sum xc = 0; the
 *                   window ends are held fixed — step functions of E, so this is the exact derivative almost everywhere);
 *   C_te            g[0] += c C10 / early;  g[ke] -= c C10 (1 / early + 1 / late);
 *   D50             g[k50] -= c / E[0];  g[0] += c E[k50] / E[0]^2;
 *   Ts              g[k] += c / (fs E[0]) for every k >= 1;  g[0] -= c Ts / E[0];
 * and d_weights[r][j] = 2 H[r][j] * sum_{k <= j} g[k] = dL/dH[r][j] for L = sum_r loss_rows[r], in H's layout: exactly 0 where H is 0,
 * all-zero in a row with no counting parameter, no entry left unwritten.  The terms of one bin are added in the order of the parameter
 * numbers, the three time terms first and under one division by E[k].  g is evaluated from E and a block of coefficients per row; no
 * dense g array goes to memory.  d_weights == NULL: the loss (and params) only.  params may be NULL in rvb_decay_params_loss.
 * REFUSALS, before any device is touched; a failed call writes nothing.  RVB_ERR_INVALID: a NULL ctx or required pointer (d_curve,
 * params; for the loss d_histogram, d_curve, targets, param_weights, loss_rows), nrows == 0 or nbins == 0, a sample rate that is not
 * finite and > 0, a param_weight that is not finite or is negative, a target that is not finite where its weight is > 0, d_weights
 * overlapping the histogram or the curve.  RVB_ERR_CAPACITY as for rvb_decay_curve: more than 4096 rows, 2^32 bins or more.
 * rvb_last_timings names the kernels of the call: "decay_params_find_kernel" (one pass over E for the five thresholds of the three
 * windows), "decay_params_window_kernel", "decay_params_sums_kernel" (one pass over E: the three sums of xc * level, each where its window
 * meets the tile, and sum E), "decay_params_fit_kernel" (the seven parameters, the row's loss and its coefficients); with d_weights also
 * "decay_params_adjoint_sums_kernel", "decay_params_adjoint_carry_kernel", "decay_params_adjoint_scan_kernel".  The row's loss is left by
 * the fit kernel, so that the call without d_weights ends there.
 * MEASURED on one MI355X (profiles/decay_params_n1.txt, tools/decay_params_bench.py; medians of one run, calls by the host clock to the
 * synchronisation, kernels by HIP events), at workload C2's stereo histogram, 16 x 846 741, and at 512 x 846 741 (64 channels):
 *     rvb_decay_params          0.145 ms / 1.85 ms, where three rvb_decay_times calls take 0.343 ms / 3.03 ms and the pinned download of
 *                               the curve that a host-side C80, D50 or Ts needs on top 0.98 ms / 30.4 ms (9.1 x / 18 x the call).  Kernels
 *                               0.094 ms / 1.79 ms against a floor of 0.016 ms / 0.53 ms (E read twice, 6.6 TB/s): the find pass runs at
 *                               1.9 x / 1.3 x its floor, the sums pass at 7.0 x / 5.4 x — the binary64 logarithm per bin of the windows'
 *                               union (0 .. -35 dB, more than half the row here) bounds it, as it bounds decay_times_sums_kernel; at C2
 *                               launches and the download of the results are a third of the call;
 *     rvb_decay_params_loss     0.270 ms / 4.22 ms with weights, 0.170 ms / 2.16 ms without, beside rvb_decay_loss' 0.206 ms / 4.20 ms and
 *                               0.119 ms / 2.23 ms in the same loop.  The three adjoint kernels 0.084 ms / 2.31 ms against a floor of
 *                               0.033 ms / 1.05 ms (E read twice, H once, w written once): the sums pass at 4.0 x / 3.6 x its floor, the
 *                               scan at 1.8 x / 1.7 x; the binary64 division per window bin and the binary64 scan are the candidates (no
 *                               counter run has been made);
 *     the older calls           rvb_decay_curve, rvb_decay_times and rvb_decay_loss of this build against a build of the commit before, the
 *                               same loop in processes that take turns: medians differ by 0.000 / -0.013 ms, -0.001 / -0.033 ms and
 *                               -0.001 / -0.17 ms, inside the difference between the parent's own two processes (0.001 / 0.015 ms,
 *                               0.004 / 0.035 ms, 0.002 / 0.18 ms): their device code is unchanged.  (The logarithm-bound kernels follow
 *                               the clock: rvb_decay_loss takes 3.7 ms in that loop and 4.2 ms in the loop that also runs the new calls.) */
enum { RVB_DECAY_EDT = 0, RVB_DECAY_T20 = 1, RVB_DECAY_T30 = 2, RVB_DECAY_C50 = 3, RVB_DECAY_C80 = 4, RVB_DECAY_D50 = 5, RVB_DECAY_TS = 6 };
#define RVB_DECAY_NPARAMS 7
int rvb_decay_params(rvb_ctx * ctx, const void * d_curve, uint64_t nrows, uint64_t nbins, float sample_rate,
                     float * params /* host [nrows][RVB_DECAY_NPARAMS] */);
int rvb_decay_params_loss(rvb_ctx * ctx, const void * d_histogram, const void * d_curve, uint64_t nrows, uint64_t nbins, float sample_rate,
                          const float * targets /* host [nrows][7] */, const float * param_weights /* host [nrows][7] */,
                          double * loss_rows /* host [nrows] */, float * params /* host [nrows][7], may be NULL */,
                          void * d_weights /* device [nrows][nbins], may be NULL */);

/* Chooses the pair that rvb_get_direct and the rvb_ir_* calls below work on (pair 0 after a trace).  RVB_ERR_STATE: nothing traced;
 * RVB_ERR_INVALID: no such pair.  A successful call voids the IR configuration and a prepared exact list, which were made for the
 * records of the pair selected before (rvb_ir_configure_* again), also when it names the pair that is selected already. */
int rvb_ir_select_pair(rvb_ctx * ctx, uint64_t pair);

/* ---- raw results: replace getRawDiffuse / getRawImages (rayverb.cpp:687-714) ---------------- */
int rvb_get_diffuse(rvb_ctx * ctx, rvb_impulse * out /* host [nrays*nreflections] */);
/* Device address of the same array (valid until the next rvb_trace / rvb_destroy). */
int rvb_diffuse_device(rvb_ctx * ctx, const void ** d_impulses, uint64_t * count);
/* Direct-path impulse (slot 0; all-zero when the source is not visible from the microphone). */
int rvb_get_direct(rvb_ctx * ctx, rvb_impulse * out);
/* Valid image-source contributions of this context's rays, sorted by (ray, slot). */
int rvb_get_image_candidates(rvb_ctx * ctx, rvb_image_candidate * out, uint64_t capacity, uint64_t * count);
/* Host-only merge = the de-dup map of rayverb.cpp:654-676 followed by getRawImages
 * (rayverb.cpp:692-706): first (lowest) ray wins per key, output in std::map key order.
 * Candidates of several contexts (GPU shards) may be concatenated before the call. */
int rvb_merge_images(const rvb_image_candidate * candidates, uint64_t ncandidates,
                     const rvb_impulse * direct, int remove_direct,
                     rvb_impulse * out, uint64_t capacity, uint64_t * count);

/* ---- attenuation, materialised: replace SpeakerAttenuator::attenuate (rayverb.cpp:856-892 +
 * kernel attenuate, kernel.cpp:505-535) and HrtfAttenuator::attenuate (rayverb.cpp:765-818 +
 * kernel hrtf, kernel.cpp:537-625) for ONE channel.  Host in, host out.  Impulses whose volume
 * is all-zero give {0, 0} (the reference leaves them uninitialised, quirk Q2).
 * rvb_attenuate_speaker* leave the IR configuration, a prepared exact list and the sort buffers alone.  rvb_attenuate_hrtf* put their
 * one ear's table where the table of rvb_ir_configure_hrtf lives: they void the IR configuration (whichever model it names) and a
 * prepared exact list, and a following rvb_ir_configure_hrtf with table == NULL returns RVB_ERR_STATE. */
int rvb_attenuate_speaker(rvb_ctx * ctx, const float mic[3], const rvb_impulse * in, uint64_t n,
                          const rvb_speaker * speaker, rvb_attenuated_impulse * out);
/* The same kernel on device-resident buffers (e.g. rvb_diffuse_device): d_in / d_out are HBM arrays of n Impulse /
 * AttenuatedImpulse records, distinct.  Asynchronous on the context's stream; what SpeakerAttenuator::attenuate's
 * per-channel re-upload of the impulse array (rayverb.cpp:863-875) becomes when the trace results never leave HBM. */
int rvb_attenuate_speaker_device(rvb_ctx * ctx, const float mic[3], const void * d_in, uint64_t n,
                                 const rvb_speaker * speaker, void * d_out);
int rvb_attenuate_hrtf(rvb_ctx * ctx, const float mic[3], const rvb_impulse * in, uint64_t n,
                       const float * table /* [360*180*8] for this ear */,
                       const float facing[3], const float up[3], uint64_t channel,
                       rvb_attenuated_impulse * out);
/* ... and HrtfAttenuator::attenuate's kernel on device-resident buffers (table is host memory as above). */
int rvb_attenuate_hrtf_device(rvb_ctx * ctx, const float mic[3], const void * d_in, uint64_t n,
                              const float * table, const float facing[3], const float up[3], uint64_t channel, void * d_out);

/* ---- time binning, materialised: replaces flattenImpulses (rayverb.cpp:48-77) for one channel.
 * Bit-exact with the reference's serial summation order.  out is [8][*nbins].  Called with out == NULL it reports *nbins;
 * a following call with the same (in, n, sample_rate) finds the uploaded array and its keys still on the device, unless another
 * call on this context has used the sort buffers in between (then the fill uploads again).  PRECONDITION of that pair: the
 * caller does not change in[0 .. n) between the size query and the fill — the fill does not read the host array again. */
int rvb_flatten(rvb_ctx * ctx, const rvb_attenuated_impulse * in, uint64_t n, float sample_rate,
                float * out, uint64_t capacity_bins, uint64_t * nbins);

/* ---- fused, device-resident IR generation (attenuate + predelay + bin without materialising
 * AttenuatedImpulse): replaces the chain Attenuator::attenuate -> fixPredelay ->
 * flattenImpulses of cmd/main.cpp:280-298 + rayverb.h:49-97 + rayverb.cpp:28-77.
 *
 * 1. rvb_ir_configure_*   choose the attenuation model and which impulses take part;
 *                         extra image impulses (already merged) are uploaded here.
 * 2. rvb_ir_time_range    min non-zero / max attenuated time over all channels of this context
 *                         (the inputs of findPredelay and of MAX_SAMPLE); with several GPUs the
 *                         caller all-reduces (min, max) before step 3.
 * 3. rvb_ir_accumulate    adds this context's impulses into d_histogram [nchannels][8][nbins]
 *                         (device memory, caller-zeroed, float).  mode RVB_IR_FAST uses float
 *                         atomics (order-dependent in the last bits); RVB_IR_EXACT continues, bin by
 *                         bin, the reference's serial left-to-right float sum (rayverb.cpp:67-74) from
 *                         the values d_histogram holds: on a zeroed histogram that IS flattenImpulses
 *                         bit for bit, and contexts that hold consecutive ray shards reproduce the
 *                         single-context result when they accumulate into the same histogram in shard
 *                         order (diffuse shards first, the merged image sources last).
 */
enum { RVB_IR_DIFFUSE = 1, RVB_IR_IMAGES = 2, RVB_IR_ALL = 3 };   /* OutputMode, config.h:19-23 */
enum { RVB_IR_FAST = 0, RVB_IR_EXACT = 1 };

/* Speaker layouts: 1 .. RVB_MAX_SPEAKERS channels (a 22.2 layout is 24, a spherical microphone array 32); 0 or more than that is
 * RVB_ERR_INVALID at rvb_ir_configure_speakers, rvb_pipeline_configure_speakers and rvb_multi_ir_speakers.  Channel c of every
 * [nchannels][8][nbins] histogram is speaker c.  Up to 8 channels run the kernels of csrc/histogram_kernels.hip and csrc/exact_kernels.hip; above 8 the speaker table
 * is uploaded to the device at configure time (in stream order) and ONE sort and ONE fold serve all channels, every impulse record
 * gathered from HBM once (ordered_sum_wide_kernel, csrc/exact_kernels.hip).  Above 8 channels RVB_IR_FAST runs that sorted fold as well — per channel count it is
 * faster than float atomics, which pay 32 bytes of adds per live impulse and channel (profiles/speaker_arrays_n1.txt) — so there
 * both modes return the exact mode's sums; RVB_IR_FAST promises its rounding bound only, not a mechanism.
 * MEMORY: a histogram is nchannels x 8 x nbins floats — at workload C2's 846 741 bins 27 MB per channel, 1.73 GB at 64 channels — in
 * device memory per context (rvb_ir_download; the caller's own with rvb_ir_accumulate), and again in pinned host memory per exported copy. */
#define RVB_MAX_SPEAKERS 64
int rvb_ir_configure_speakers(rvb_ctx * ctx, const float mic[3], const rvb_speaker * speakers, uint64_t nspeakers,
                              int which, const rvb_impulse * images, uint64_t nimages);
/* table == NULL: the table of this context's previous rvb_ir_configure_hrtf call stays on the device (many listeners, one table: 4 MB
 * uploaded once instead of per impulse response); RVB_ERR_STATE if there is none.  A call with a table that fails with RVB_ERR_STATE
 * because nothing is traced has uploaded its table all the same: it is the table a later call with table == NULL finds.  Every
 * successful rvb_ir_configure_* copies the images, replaces the previous configuration as a whole (model, channels, `which`, images) and
 * voids a prepared exact list. */
int rvb_ir_configure_hrtf(rvb_ctx * ctx, const float mic[3], const float * table /* [2][360*180*8] or NULL */,
                          const float facing[3], const float up[3],
                          int which, const rvb_impulse * images, uint64_t nimages);
int rvb_ir_time_range(rvb_ctx * ctx, float * min_nonzero_time, float * max_time);
/* Optional first half of rvb_ir_time_range: enqueues what the range needs on the device (the HRTF model's pass over the impulses; nothing
 * for speakers) without waiting; the rvb_ir_time_range that follows only waits and reads.  A caller that finishes several contexts'
 * impulse responses together calls this on all of them first (csrc/pipeline.hip). */
int rvb_ir_time_range_begin(rvb_ctx * ctx);
/* nbins for a given max time / predelay exactly as rayverb.cpp:57 computes MAX_SAMPLE. */
uint64_t rvb_ir_bins(float max_time, float predelay, float sample_rate);
int rvb_ir_accumulate(rvb_ctx * ctx, float predelay, float sample_rate, uint64_t nbins, int mode,
                      void * d_histogram);
/* rvb_ir_accumulate as above, and the finished [nchannels][8][nbins] histogram on its way to
 * pinned_dst (pinned host memory of the same size: rvb_host_alloc, hipHostMalloc, torch's pin_memory) on the context's export stream:
 * rvb_synchronize_exports waits for it, rvb_synchronize does not, the context's next trace does not either.  In exact mode with the
 * exact mode the last kernel of the stage can fold the histogram in `slices` bin ranges, every range leaving as soon as it is final
 * (the copy of all but the last range then runs beside the folding of the later ones); 0 = the default, ONE piece (= rvb_ir_accumulate +
 * rvb_copy_to_pinned_host_async): at workload C2 the ranges buy nothing — 54 MB need 1.1 ms of the link whenever they start, the fold
 * they could hide behind is 0.27 ms (profiles/r04_export_slices_n1.txt).  The float-atomic mode always copies the finished histogram
 * in one piece.  d_histogram must stay untouched until
 * the export has been waited for.  Reference counterpart: the blocking cl::copy of every result (rayverb.cpp:645-651, :678, :816). */
int rvb_ir_accumulate_export(rvb_ctx * ctx, float predelay, float sample_rate, uint64_t nbins, int mode,
                             void * d_histogram, void * pinned_dst, uint32_t slices);
/* RVB_IR_EXACT in two steps, for callers that hand the histogram on BLOCK BY BLOCK (the systolic chain over devices of csrc/multi.hip,
 * distributed.generate_ir(chain_exact=True)):
 *   rvb_ir_exact_prepare   everything that does not depend on what the histogram holds — bin keys, the radix sort, where each bin's run
 *                          starts and ends; every device of a chain does this as soon as its trace is done;
 *   rvb_ir_exact_fold      bins [bin_begin, bin_end): each bin's impulses added in impulse order on top of what d_histogram holds
 *                          (rayverb.cpp:67-74) — folding all bins once equals rvb_ir_accumulate(..., RVB_IR_EXACT, ...).
 * The prepared list lives in the context's sort buffers: a call that reuses them (rvb_ir_configure_*, rvb_trace, rvb_flatten*,
 * a successful rvb_ir_accumulate* in either mode and with any nbins, rvb_ir_download, rvb_reshade_grad_map) or that changes what the list was made
 * from (rvb_reshade, rvb_relisten, rvb_ir_select_pair, rvb_attenuate_hrtf*, rvb_set_scene, rvb_share_scene, rvb_set_directions*)
 * voids it and rvb_ir_exact_fold then fails with RVB_ERR_STATE, as it does for an nbins other than the prepared one.  A second
 * rvb_ir_exact_prepare replaces the list.  Both are asynchronous on the context's stream. */
int rvb_ir_exact_prepare(rvb_ctx * ctx, float predelay, float sample_rate, uint64_t nbins);
int rvb_ir_exact_fold(rvb_ctx * ctx, uint64_t nbins, uint64_t bin_begin, uint64_t bin_end, void * d_histogram);
/* Convenience for one GPU: steps 1-3 done, histogram copied to host memory [nchannels][8][*nbins]. */
int rvb_ir_download(rvb_ctx * ctx, int trim_predelay, float sample_rate, int mode,
                    float * out, uint64_t capacity_bins, uint64_t * nbins);

/* ---- device-resident plumbing for the host mirror of the reference classes (host/rayverb_api.cpp) ------------------
 * The reference's API hands every stage's result over as a std::vector (rayverb.h:123-133, :290-293, rayverb.cpp:28-77);
 * its own implementation re-uploads those vectors stage by stage (rayverb.cpp:863-875).  A host that still holds the
 * device copy of a vector it produced can skip the re-upload: these calls give it the buffers and the kernels on them. */
int rvb_device_alloc(rvb_ctx * ctx, uint64_t bytes, void ** d_ptr);
int rvb_device_free(rvb_ctx * ctx, void * d_ptr);
/* Pageable host memory <-> HBM through pinned bounce buffers driven by several host threads (a plain hipMemcpy into fresh
 * pageable memory runs at a fraction of the link rate).  Synchronous; ordered after the work already on the context's stream. */
int rvb_copy_to_host(rvb_ctx * ctx, void * dst, const void * d_src, uint64_t bytes);
int rvb_copy_to_device(rvb_ctx * ctx, void * d_dst, const void * src, uint64_t bytes);
/* Pinned (page-locked, device-mapped) host memory, and a device -> pinned-host copy that is ASYNCHRONOUS: it starts when the work
 * enqueued so far on the context's stream has finished (e.g. the rvb_ir_accumulate that fills d_src) and runs on a stream of its
 * own, so the context's next trace does not wait for the link; rvb_synchronize_exports waits for it (rvb_synchronize does not).
 * d_src must stay untouched until then.  This is what carries a finished [nchannels][8][nbins] histogram to the host.
 * pinned_dst should be pinned memory (rvb_host_alloc, hipHostMalloc, torch's pin_memory): into pageable memory the runtime's
 * copy is staged and blocks the caller.  The reference's counterpart is the blocking cl::copy of every result buffer
 * (rayverb.cpp:645-651, :678, :816). */
int rvb_host_alloc(rvb_ctx * ctx, uint64_t bytes, void ** host_ptr);
int rvb_host_free(rvb_ctx * ctx, void * host_ptr);
int rvb_copy_to_pinned_host_async(rvb_ctx * ctx, void * pinned_dst, const void * d_src, uint64_t bytes);
int rvb_synchronize_exports(rvb_ctx * ctx);
/* fixPredelay (rayverb.h:76-90) on a device-resident AttenuatedImpulse array: time = time > seconds ? time - seconds : 0. */
int rvb_fix_predelay_device(rvb_ctx * ctx, void * d_attenuated, uint64_t n, float seconds);
/* rvb_flatten on a device-resident AttenuatedImpulse array (same result, no upload). */
int rvb_flatten_device(rvb_ctx * ctx, const void * d_attenuated, uint64_t n, float sample_rate,
                       float * out, uint64_t capacity_bins, uint64_t * nbins);

/* ---- several GPUs of one node (csrc/multi.hip) ---------------------------------------------------------------------------
 * The reference drives ONE device (rayverb.cpp:163, :176-177).  An rvb_multi owns one rvb_ctx and one host thread per listed
 * device: the scene is replicated, device g traces the contiguous ray range [g N / D, (g+1) N / D) of the directions handed to
 * rvb_multi_set_directions, image-source candidates are merged with the reference's lowest-ray-wins rule (rayverb.cpp:654-676)
 * and the per-band histograms are combined on the devices:
 *   RVB_IR_EXACT  the devices continue ONE left-to-right float sum in ray order (a chain of peer copies): bit-identical to a
 *                 single context and to the reference's flattenImpulses;
 *   RVB_IR_FAST   every device bins its shard at once, then one RCCL ncclAllReduce(sum) over xGMI (librccl.so is loaded at run
 *                 time; a device list RCCL cannot serve — the same GPU twice — is summed with peer copies instead).
 * devices == NULL means 0 .. ndevices-1.  Not thread-safe, like rvb_ctx. */
typedef struct rvb_multi rvb_multi;
enum { RVB_MULTI_REHEARSE_RCCL = 1 };     /* flags: run the RCCL all-reduce even for a single device (exercises the library binding) */
int rvb_multi_create(rvb_multi ** out, const int * devices, int ndevices, unsigned flags);
void rvb_multi_destroy(rvb_multi * m);
const char * rvb_multi_last_error(const rvb_multi * m);
int rvb_multi_devices(const rvb_multi * m);
/* The context of device slot `index` and the ray range it traced (e.g. to run independent (source, listener) pairs per device). */
int rvb_multi_context(rvb_multi * m, int index, rvb_ctx ** ctx, uint64_t * first_ray, uint64_t * nrays);
/* RVB_IR_EXACT over several devices is a SYSTOLIC chain: the [nchannels][8][nbins] histogram travels in `blocks` bin-range blocks
 * (default 8), device g folds block k while device g + 1 folds block k - 1 — (D + blocks - 1) / blocks folds and hops instead of D.
 * Any block count gives the same bytes (tests/test_gpu_multi.py forces 1, 3 and 8).  rvb_multi_peer_links: directed pairs of distinct
 * devices for which rvb_multi_create could enable peer access (0 on one GPU); without it the runtime stages the hops through the host. */
int rvb_multi_set_chain_blocks(rvb_multi * m, uint32_t blocks);
int rvb_multi_peer_links(const rvb_multi * m);
int rvb_multi_used_rccl(const rvb_multi * m);            /* 1 if the last RVB_IR_FAST histogram was summed by RCCL */
int rvb_multi_set_scene(rvb_multi * m, const rvb_triangle * triangles, uint64_t ntriangles, const rvb_float3 * vertices, uint64_t nvertices,
                        const rvb_surface * surfaces, uint64_t nsurfaces);
int rvb_multi_set_directions(rvb_multi * m, const rvb_float3 * directions, uint64_t nrays);
/* rvb_set_source_pattern(ctx, pattern, 1) on every device's context (NULL: off).  Every device scales its own ray shard with its own
 * slice of the directions, so the results stay the bytes one context gives. */
int rvb_multi_set_source_pattern(rvb_multi * m, const rvb_source_pattern * pattern);
/* Raytracer::raytrace on all devices at once (blocking, like the reference's). */
int rvb_multi_trace(rvb_multi * m, const float mic[3], const float source[3], uint64_t nreflections, const float air_coefficient[8]);
/* getRawDiffuse / getRawImages over all shards: ray-major [nrays * nreflections]; merged image sources in std::map key order. */
int rvb_multi_get_diffuse(rvb_multi * m, rvb_impulse * out);
int rvb_multi_get_images(rvb_multi * m, int remove_direct, rvb_impulse * out, uint64_t capacity, uint64_t * count);
/* attenuate -> fixPredelay -> flattenImpulses over all shards; out (host) is [nchannels][8][*nbins]; out == NULL reports *nbins.
 * 1 .. RVB_MAX_SPEAKERS speakers, in both modes.  The exact mode's chain moves nchannels x 8 rows per block: on distinct devices that
 * is one peer copy per row and block — 512 of them per block for a 64-channel layout — which this entry point does not batch. */
int rvb_multi_ir_speakers(rvb_multi * m, const float mic[3], const rvb_speaker * speakers, uint64_t nspeakers, int which, int remove_direct,
                          int trim_predelay, float sample_rate, int mode, float * out, uint64_t capacity_bins, uint64_t * nbins);
int rvb_multi_ir_hrtf(rvb_multi * m, const float mic[3], const float * table /* [2][360*180*8] */, const float facing[3], const float up[3],
                      int which, int remove_direct, int trim_predelay, float sample_rate, int mode,
                      float * out, uint64_t capacity_bins, uint64_t * nbins);

/* ---- impulse responses back to back (csrc/pipeline.hip) --------------------------------------------------------------------
 * What a batch caller of the reference does with cmd/main.cpp:241-298 in a loop — raytrace, attenuate per channel, fixPredelay,
 * flattenImpulses per impulse response, every stage blocking — as a pipeline over several contexts of ONE GPU.  The contexts are the
 * caller's and stay the caller's: every one holds the same scene (rvb_set_scene) and the same rays (rvb_set_directions*) before the
 * pipeline is created, and is not used for anything else while jobs are pending.  Job i runs on context i % count.  Jobs are traced
 * in groups of `group` contexts with ONE path-kernel launch per group (rvb_trace_group; 0 = count / 2, at most
 * RVB_PIPELINE_MAX_GROUP), the traces of the group after next go out before the current group is finished, the binning stages of a
 * group are enqueued together, and every histogram leaves for pinned host memory on its context's export stream, bin range by bin
 * range (rvb_ir_accumulate_export).  Measured at workload C2 with 4 contexts: the rate bench.py reports.
 *   rvb_pipeline_configure_*   the attenuation model and the binning of all jobs that follow (no jobs may be pending)
 *   rvb_pipeline_submit        one impulse response: microphone and source (HRTF: the configured facing / up; _oriented: its own).
 *                              Never blocks; RVB_ERR_CAPACITY when 4 x count jobs are pending (take results first)
 *   rvb_pipeline_next          blocks until the OLDEST pending job's [nchannels][8][nbins] histogram is in host memory; the result's
 *                              `histogram` points into the pipeline's ring of pinned buffers and stays valid until `count` further
 *                              results have been taken (or the pipeline is destroyed)
 * Results are those of rvb_trace + rvb_merge_images + rvb_ir_configure_* + rvb_ir_download on one context, bit for bit in
 * RVB_IR_EXACT (tests/cpp/test_pipeline.cpp).  Not thread-safe.
 * MEMORY with wide speaker layouts (1 .. RVB_MAX_SPEAKERS channels): every context keeps one device histogram per pair of a unit, and
 * the ring of pinned host buffers holds 2 x count histograms here, and "pending limit + validity window" = 3 x count x P of them with
 * lanes (rvb_pipeline_create_lanes below), once all are in use.  A histogram is nchannels x 8 x nbins floats (27 MB per channel at workload C2's 846 741 bins, 1.73 GB at 64 channels),
 * so a caller with wide layouts uses fewer contexts.  There is no limit of its own: a pinned or device allocation that fails surfaces
 * as RVB_ERR_HIP with the runtime's text. */
#define RVB_PIPELINE_MAX_GROUP 4
typedef struct rvb_pipeline rvb_pipeline;
typedef struct {
    uint64_t job;                 /* submission number: 0, 1, 2, ... */
    const float * histogram;      /* pinned host memory, [nchannels][8][nbins] */
    uint64_t nchannels, nbins;
    float predelay, max_time;     /* seconds: what fixPredelay subtracted (0 without trim_predelay); the latest arrival */
    uint64_t nimages;             /* merged image-source impulses that took part */
} rvb_pipeline_result;
int rvb_pipeline_create(rvb_pipeline ** out, rvb_ctx ** ctxs, uint64_t count, uint64_t group);
void rvb_pipeline_destroy(rvb_pipeline * p);
const char * rvb_pipeline_last_error(const rvb_pipeline * p);
int rvb_pipeline_configure_speakers(rvb_pipeline * p, const rvb_speaker * speakers, uint64_t nspeakers, int which, int remove_direct,
                                    int trim_predelay, float sample_rate, int mode, uint64_t nreflections, const float air_coefficient[8]);
int rvb_pipeline_configure_hrtf(rvb_pipeline * p, const float * table /* [2][360*180*8] */, const float facing[3], const float up[3],
                                int which, int remove_direct, int trim_predelay, float sample_rate, int mode, uint64_t nreflections,
                                const float air_coefficient[8]);
int rvb_pipeline_submit(rvb_pipeline * p, const float mic[3], const float source[3]);
int rvb_pipeline_submit_oriented(rvb_pipeline * p, const float mic[3], const float source[3], const float facing[3], const float up[3]);
/* Directional sources (rvb_set_source_pattern above) for the jobs that follow; no jobs may be pending, like _configure_*.
 *   rvb_pipeline_set_source_pattern   the shape per band and the default facing of the source (shape == NULL: off, direction ignored).
 *                                     From the first call on, the pipeline sets (or clears) the pattern of its contexts with every
 *                                     trace; a pipeline that never got the call leaves its contexts' patterns alone.
 *   rvb_pipeline_submit_directed      rvb_pipeline_submit_oriented for ONE job whose source faces `source_direction` (NULL: the default
 *                                     facing; facing / up may be NULL as in _submit).  RVB_ERR_STATE for a direction while the pattern
 *                                     is off.  With pairs_per_launch > 1 a unit's launch gets its jobs' patterns in the per-pair form.
 * RVB_ERR_INVALID for a non-finite value or a zero-length direction. */
int rvb_pipeline_set_source_pattern(rvb_pipeline * p, const float shape[8], const float direction[3]);
int rvb_pipeline_submit_directed(rvb_pipeline * p, const float mic[3], const float source[3], const float facing[3], const float up[3],
                                 const float source_direction[3]);
uint64_t rvb_pipeline_pending(const rvb_pipeline * p);
int rvb_pipeline_next(rvb_pipeline * p, rvb_pipeline_result * out);

/* The same pipeline over LANES — several GPUs of a node, or several schedules on one — and several pairs per path-kernel launch: what a
 * caller with many (source, listener) pairs of one hall does (BASELINE config C5: 64 pairs on 8 GPUs).  A lane is a run of consecutive
 * contexts of `ctxs`, lane_sizes[l] of them (they add up to `count`); the contexts of one lane share one device, different lanes may sit
 * on different devices or on the same one, a context appears once.  Every lane runs the schedule above (groups, early traces, staged
 * binning, its own zero-fill stream and ring) from a host thread of its own: that thread makes every HIP and rvb_* call on the lane's
 * contexts, from set-up in rvb_pipeline_create_lanes to tear-down in rvb_pipeline_destroy, so the caller does not touch them either
 * while the pipeline exists.
 *   options->pairs_per_launch  P = 1: one trace per job, as above.  P = 2 .. RVB_PIPELINE_MAX_PAIRS: a UNIT of P consecutive jobs is
 *                              traced by ONE rvb_trace_pairs launch on one context, then staged pair by pair (rvb_ir_select_pair, the
 *                              pair's own image-source candidates, its own facing), each pair into a device histogram of its own
 *   options->group             contexts per path-kernel launch inside a lane, as `group` above (0 = default); with P > 1 a unit is a
 *                              launch of its own and a group above 1 is refused
 *   options == NULL            group 0, P = 1
 * WHERE A JOB RUNS (deterministic): job i belongs to unit u = i / P; unit u goes to lane u % nlanes; inside the lane, the lane's k-th unit
 * (k = u / nlanes) runs on its context k % lane_sizes[l].  An incomplete last unit is traced with the pairs it has when
 * rvb_pipeline_next waits for one of its jobs.
 *   rvb_pipeline_configure_*, _submit, _submit_oriented, _pending, _next, _destroy work as above, with
 *   - the pending limit 2 x count x P (RVB_ERR_CAPACITY above it; submit never blocks);
 *   - results in submission order; `histogram` stays valid until count x P further results have been taken (or the pipeline is
 *     destroyed); the rings hold pending limit + that window buffers in all, allocated as they are first used;
 *   - a failing stage (e.g. RVB_ERR_STATE from rvb_trace on a context without a scene) fails its LANE: rvb_pipeline_next returns the
 *     code for that job and for every later job of the lane (each counts as taken), rvb_pipeline_last_error names the lane and the call
 *     ("lane 1: rvb_pipeline: trace: ..."); results of other lanes, and of earlier jobs, are unaffected.  A failed lane stays failed;
 *   - rvb_pipeline_destroy joins the lane threads, also after a failure.
 * Results are bit for bit those of rvb_trace + rvb_merge_images + rvb_ir_configure_* + rvb_ir_download on one context in RVB_IR_EXACT
 * (tests/cpp/test_pipeline_lanes.cpp), whatever the lanes and P.  Not thread-safe: one caller thread per pipeline. */
#define RVB_PIPELINE_MAX_PAIRS 8
typedef struct {
    uint64_t group;              /* contexts per path-kernel launch inside a lane (0 = default; must be 0 or 1 with pairs_per_launch > 1) */
    uint64_t pairs_per_launch;   /* 1 .. RVB_PIPELINE_MAX_PAIRS */
} rvb_pipeline_options;
int rvb_pipeline_create_lanes(rvb_pipeline ** out, rvb_ctx ** ctxs, uint64_t count, const uint64_t * lane_sizes, uint64_t nlanes,
                              const rvb_pipeline_options * options);

/* ---- measurement hooks (bench.py) ------------------------------------------------------------
 * Durations in milliseconds of the kernels of the last rvb_trace / rvb_ir_accumulate, taken with
 * HIP events on the context's stream; names is a ';'-separated list matching ms[]. */
int rvb_last_timings(rvb_ctx * ctx, char * names, uint64_t names_capacity, float * ms, uint64_t ms_capacity, uint64_t * count);
/* In-kernel cycle stamps of the last trace; all zero unless the library was built with -DRVB_STAMPS=1
 * (diagnostic build, never the shipped one).  out[0..15] path_kernel, out[16..31] shadow_kernel. */
int rvb_debug_stamps(rvb_ctx * ctx, uint64_t * out, uint64_t capacity);
/* Number of bounces actually executed by the last trace (escaped rays stop early). */
int rvb_executed_bounces(rvb_ctx * ctx, uint64_t * bounces);

#ifdef __cplusplus
}
#endif
#endif
