// context.hip — the context of include/rvb_capi.h: life cycle, scene, directions, timings, diagnostics (see ctx.h for the other stages).
#include "ctx.h"

#include <cstring>

static thread_local std::string g_create_error;     // the text of a failed rvb_create

int fail(rvb_ctx * ctx, int code, const std::string & what)
{
    if (ctx) ctx->error = what; else g_create_error = what;
    return code;
}

extern "C" {

int rvb_create(rvb_ctx ** out, int device, unsigned flags)
{
    (void) flags;
    if (!out)
        return fail(nullptr, RVB_ERR_INVALID, "rvb_create: out is NULL");
    *out = nullptr;
    int count = 0;
    hipError_t e = hipGetDeviceCount(&count);
    if (e != hipSuccess || count <= 0)
        return fail(nullptr, RVB_ERR_NO_DEVICE,
                    std::string("rvb_create: no HIP device (") + (e != hipSuccess ? hipGetErrorString(e) : "count 0") +
                    "); this library has no CPU path");
    if (device < 0 || device >= count)
        return fail(nullptr, RVB_ERR_INVALID, "rvb_create: device index out of range");
    hipDeviceProp_t prop;
    if ((e = hipGetDeviceProperties(&prop, device)) != hipSuccess)
        return fail(nullptr, RVB_ERR_NO_DEVICE, std::string("hipGetDeviceProperties: ") + hipGetErrorString(e));
    if (std::strncmp(prop.gcnArchName, "gfx950", 6) != 0)
        return fail(nullptr, RVB_ERR_NO_DEVICE, std::string("rvb_create: kernels are built for gfx950 only, device is ") + prop.gcnArchName);
    std::unique_ptr<rvb_ctx> ctx(new rvb_ctx());       // (a failure below releases what was made before it)
    ctx->device = device;
    ctx->arch = prop.gcnArchName;
    ctx->compute_units = prop.multiProcessorCount;
    ctx->hbm_bytes = prop.totalGlobalMem;
    // The side stream (image_kernel) runs at the lowest priority: the record grouping on the main stream is the critical
    // path between path_kernel and shadow_kernel and must not queue behind image_kernel's 14 k workgroups.
    int prio_least = 0, prio_greatest = 0;
    if ((e = hipSetDevice(device)) != hipSuccess || (e = hipDeviceGetStreamPriorityRange(&prio_least, &prio_greatest)) != hipSuccess ||
        (e = hipStreamCreateWithPriority(&ctx->stream.h, hipStreamNonBlocking, prio_greatest)) != hipSuccess ||
        (e = hipStreamCreateWithPriority(&ctx->side_stream.h, hipStreamNonBlocking, prio_least)) != hipSuccess ||
        (e = hipStreamCreateWithPriority(&ctx->export_stream.h, hipStreamNonBlocking, (prio_least + prio_greatest) / 2)) != hipSuccess ||
        (e = hipEventCreateWithFlags(&ctx->export_ready.h, hipEventDisableTiming)) != hipSuccess ||
        (e = hipEventCreateWithFlags(&ctx->path_done.h, hipEventDisableTiming)) != hipSuccess ||
        (e = hipEventCreateWithFlags(&ctx->side_done.h, hipEventDisableTiming)) != hipSuccess ||
        (e = hipEventCreateWithFlags(&ctx->prep_done.h, hipEventDisableTiming)) != hipSuccess ||
        (e = hipEventCreateWithFlags(&ctx->group_done.h, hipEventDisableTiming)) != hipSuccess ||
        (e = ctx->trace.create()) != hipSuccess)
        return fail(nullptr, RVB_ERR_HIP, std::string("rvb_create: ") + hipGetErrorString(e));
    *out = ctx.release();
    return RVB_OK;
}

void rvb_destroy(rvb_ctx * ctx)
{
    if (ctx) delete ctx;          // (~rvb_ctx waits for the context's streams; its members release what they hold)
}

const char * rvb_last_error(const rvb_ctx * ctx)
{
    return ctx ? ctx->error.c_str() : g_create_error.c_str();
}

int rvb_wait_for_event(rvb_ctx * ctx, void * hip_event)
{
    if (!ctx || !hip_event) return RVB_ERR_INVALID;
    RVB_BIND(ctx);
    RVB_HIP(fail, ctx, hipStreamWaitEvent(ctx->stream, reinterpret_cast<hipEvent_t>(hip_event), 0));
    return RVB_OK;
}

int rvb_record_event(rvb_ctx * ctx, void * hip_event)
{
    if (!ctx || !hip_event) return RVB_ERR_INVALID;
    RVB_BIND(ctx);
    RVB_HIP(fail, ctx, hipEventRecord(reinterpret_cast<hipEvent_t>(hip_event), ctx->stream));
    return RVB_OK;
}

int rvb_synchronize(rvb_ctx * ctx)
{
    if (!ctx) return RVB_ERR_INVALID;
    RVB_BIND(ctx);
    RVB_HIP(fail, ctx, hipStreamSynchronize(ctx->stream));
    return RVB_OK;
}

int rvb_device_info(rvb_ctx * ctx, char * arch, uint64_t arch_capacity, int * compute_units, uint64_t * hbm_bytes)
{
    if (!ctx) return RVB_ERR_INVALID;
    if (arch && arch_capacity) {
        std::strncpy(arch, ctx->arch.c_str(), arch_capacity - 1);
        arch[arch_capacity - 1] = 0;
    }
    if (compute_units) *compute_units = ctx->compute_units;
    if (hbm_bytes) *hbm_bytes = ctx->hbm_bytes;
    return RVB_OK;
}

int rvb_device_index(rvb_ctx * ctx, int * device)
{
    if (!ctx || !device) return RVB_ERR_INVALID;
    *device = ctx->device;
    return RVB_OK;
}

int rvb_set_scene(rvb_ctx * ctx, const rvb_triangle * triangles, uint64_t ntriangles,
                  const rvb_float3 * vertices, uint64_t nvertices,
                  const rvb_surface * surfaces, uint64_t nsurfaces)
{
    if (!ctx) return RVB_ERR_INVALID;
    if ((ntriangles && !triangles) || (nvertices && !vertices) || !surfaces || nsurfaces == 0)
        return fail(ctx, RVB_ERR_INVALID, "rvb_set_scene: null input or no surfaces");
    RVB_BIND(ctx);
    BuiltScene built;
    std::string err = rvb_build_scene(triangles, ntriangles, vertices, nvertices, nsurfaces, built);
    if (!err.empty())
        return fail(ctx, err.find("stack") != std::string::npos ? RVB_ERR_CAPACITY : RVB_ERR_INVALID, "rvb_set_scene: " + err);
    RVB_HIP(fail, ctx, hipStreamSynchronize(ctx->stream));
    ContextScene & scene = ctx->scene;
    scene.drop();                                   // (until set() below: a failure midway leaves no scene)
    ctx->void_trace();
    // a store other contexts hold stays theirs: this context gets a new one (buffers it holds alone are reused)
    if (!scene.store || scene.store.use_count() > 1) {
        scene.store = std::make_shared<SceneStore>();
        scene.store->device = ctx->device;
    }
    SceneStore & st = *scene.store;
    auto upload = [&](DevBuf & b, const void * src, size_t bytes) -> hipError_t {
        hipError_t e = b.ensure(bytes);
        if (e != hipSuccess || bytes == 0) return e;
        return hipMemcpy(b.p, src, bytes, hipMemcpyHostToDevice);
    };
    RVB_HIP(fail, ctx, upload(st.nodes, built.nodes.data(), built.nodes.size() * sizeof(BvhNode)));
    RVB_HIP(fail, ctx, upload(st.tris, built.tris.data(), built.tris.size() * sizeof(BvhTri)));
    // the eighth word of a shading record (the builder's plane-group number, of no use on the device) carries the triangle's position
    // in leaf order: the path kernel's record-grouping key comes with the 32 bytes it reads anyway instead of from a gather of its own
    for (size_t i = 0; i < built.shade.size() && i < built.leafpos.size(); ++i) built.shade[i].group = built.leafpos[i];
    RVB_HIP(fail, ctx, upload(st.shade, built.shade.data(), built.shade.size() * sizeof(TriShade)));
    RVB_HIP(fail, ctx, upload(st.corners, built.corners.data(), built.corners.size() * sizeof(TriCorners)));
    RVB_HIP(fail, ctx, upload(st.surfaces, surfaces, nsurfaces * sizeof(rvb_surface)));
    SceneDev dev;
    dev.nodes = st.nodes.as<const BvhNode>();
    dev.tris = st.tris.as<const BvhTri>();
    dev.shade = st.shade.as<const TriShade>();
    dev.corners = st.corners.as<const TriCorners>();
    dev.surfaces = st.surfaces.as<const rvb_surface>();
    dev.ntris = (uint32_t) built.tris.size();
    // cull slack along the ray: the float distance of a triangle may differ from the exact one
    dev.cull_abs = built.pad;
    dev.cull_rel = 1e-4f;
    scene.set(dev, built.nodes.size(), built.tris.size(), built.depth, built.stack_need, nsurfaces, ntriangles);
    return RVB_OK;
}

int rvb_share_scene(rvb_ctx * ctx, rvb_ctx * from)
{
    if (!ctx || !from) return RVB_ERR_INVALID;
    if (ctx == from) return RVB_OK;
    if (!from->scene.have() || !from->scene.store) return fail(ctx, RVB_ERR_STATE, "rvb_share_scene: the other context holds no scene");
    if (from->device != ctx->device) return fail(ctx, RVB_ERR_INVALID, "rvb_share_scene: the contexts are on different devices (a scene is shared within one GPU's memory)");
    RVB_BIND(ctx);
    RVB_HIP(fail, ctx, hipStreamSynchronize(ctx->stream));        // nothing of this context reads its old scene any more
    ctx->scene = from->scene;                                       // the store, where the kernels find it, every count
    ctx->void_trace();
    return RVB_OK;
}

int rvb_scene_info(rvb_ctx * ctx, uint64_t * nodes, uint64_t * kept_triangles, uint32_t * depth)
{
    if (!ctx) return RVB_ERR_INVALID;
    if (!ctx->scene.have()) return fail(ctx, RVB_ERR_STATE, "rvb_scene_info: no scene");
    if (nodes) *nodes = ctx->scene.nnodes;
    if (kept_triangles) *kept_triangles = ctx->scene.kept_triangles;
    if (depth) *depth = ctx->scene.depth;
    return RVB_OK;
}

int rvb_set_directions(rvb_ctx * ctx, const rvb_float3 * directions, uint64_t nrays)
{
    if (!ctx) return RVB_ERR_INVALID;
    if (nrays && !directions) return fail(ctx, RVB_ERR_INVALID, "rvb_set_directions: null directions");
    // Unit vectors are the contract (reference getRandomDirections, helpers.cpp:63-81): distances, times and the diffuse cosine
    // are only meaningful for |d| = 1.  The pruning margins of the acceleration structure (box padding, cull slack, the
    // triangles dropped as unhittable at build time) hold for 0.5 <= |d| <= 2; anything outside, or not finite, is refused
    // rather than traced with weaker guarantees.
    for (uint64_t i = 0; i < nrays; ++i) {
        const float * d = directions[i].s;
        const float len2 = d[0] * d[0] + d[1] * d[1] + d[2] * d[2];
        if (!(len2 >= 0.25f && len2 <= 4.0f))
            return fail(ctx, RVB_ERR_INVALID, "rvb_set_directions: direction " + std::to_string(i) + " is not a unit vector (length^2 = " +
                                              std::to_string(len2) + "; 0.5 <= length <= 2 is accepted)");
    }
    RVB_BIND(ctx);
    RVB_HIP(fail, ctx, hipStreamSynchronize(ctx->stream));
    RVB_HIP(fail, ctx, ctx->directions_own.ensure(nrays * sizeof(rvb_float3)));
    if (nrays)
        RVB_HIP(fail, ctx, hipMemcpy(ctx->directions_own.p, directions, nrays * sizeof(rvb_float3), hipMemcpyHostToDevice));
    ctx->directions = ctx->directions_own.as<const float4>();
    ctx->nrays = nrays;
    ctx->void_trace();
    return RVB_OK;
}

int rvb_set_directions_device(rvb_ctx * ctx, const void * d_directions, uint64_t nrays)
{
    if (!ctx) return RVB_ERR_INVALID;
    if (nrays && !d_directions) return fail(ctx, RVB_ERR_INVALID, "rvb_set_directions_device: null directions");
    ctx->directions = reinterpret_cast<const float4 *>(d_directions);
    ctx->nrays = nrays;
    ctx->void_trace();
    return RVB_OK;
}

int rvb_set_concurrent_traces(rvb_ctx * ctx, uint32_t traces)
{
    if (!ctx) return RVB_ERR_INVALID;
    if (traces == 0 || traces > (1u << 20)) return fail(ctx, RVB_ERR_INVALID, "rvb_set_concurrent_traces: 1 .. 2^20");
    ctx->concurrent_traces = traces;
    return RVB_OK;
}

int rvb_set_path_lanes(rvb_ctx * ctx, uint32_t lanes)
{
    if (!ctx) return RVB_ERR_INVALID;
    if (lanes != 0 && lanes != 1 && lanes != 2 && lanes != 4) return fail(ctx, RVB_ERR_INVALID, "rvb_set_path_lanes: 0 (automatic), 1, 2 or 4");
    ctx->path_lanes = lanes;
    return RVB_OK;
}

int rvb_last_timings(rvb_ctx * ctx, char * names, uint64_t names_capacity, float * ms, uint64_t ms_capacity, uint64_t * count)
{
    if (!ctx || !count) return RVB_ERR_INVALID;
    RVB_BIND(ctx);
    RVB_HIP(fail, ctx, hipStreamSynchronize(ctx->stream));
    std::string joined;
    uint64_t n = 0;
    for (const Timing & t : ctx->timings) {
        float v = 0.0f;
        RVB_HIP(fail, ctx, hipEventElapsedTime(&v, t.start, t.stop));
        if (ms && n < ms_capacity) ms[n] = v;
        if (!joined.empty()) joined += ';';
        joined += t.name;
        ++n;
    }
    *count = n;
    if (names && names_capacity) {
        std::strncpy(names, joined.c_str(), names_capacity - 1);
        names[names_capacity - 1] = 0;
    }
    return RVB_OK;
}

int rvb_debug_stamps(rvb_ctx * ctx, uint64_t * out, uint64_t capacity)
{
    if (!ctx || !out) return RVB_ERR_INVALID;
    if (!ctx->trace.traced()) return fail(ctx, RVB_ERR_STATE, "rvb_debug_stamps: nothing traced");
    RVB_BIND(ctx);
    RVB_HIP(fail, ctx, hipStreamSynchronize(ctx->stream));
    unsigned long long v[32];
    RVB_HIP(fail, ctx, hipMemcpy(v, ctx->trace.stamps.p, sizeof(v), hipMemcpyDeviceToHost));
    for (uint64_t i = 0; i < capacity && i < 32; ++i) out[i] = v[i];
    return RVB_OK;
}

int rvb_executed_bounces(rvb_ctx * ctx, uint64_t * bounces)
{
    if (!ctx || !bounces) return RVB_ERR_INVALID;
    if (!ctx->trace.traced()) return fail(ctx, RVB_ERR_STATE, "rvb_executed_bounces: nothing traced");
    RVB_BIND(ctx);
    int rc = fetch_small(ctx);
    if (rc != RVB_OK) return rc;
    *bounces = ctx->trace.host->small.executed;
    return RVB_OK;
}

}  // extern "C"
