// rayverb_api.cpp — the reference's host classes (rayverb/rayverb.h) on top of the rvb C-ABI.
// Every compute step goes through librvb_hip.so (HIP kernels); nothing here computes results on
// the CPU except the reference's own host-side steps (bounds warnings, vector plumbing).
#include "../../include/rayverb/rayverb.h"
#include "../../include/rvb_capi.h"
#include "resident_cache.h"
#include "scene_loader.h"

#include <cmath>
#include <cstdlib>
#include <cstring>
#include <iostream>
#include <mutex>
#include <thread>

#include <sys/mman.h>

static_assert(sizeof(Triangle) == sizeof(rvb_triangle), "Triangle");
static_assert(sizeof(cl_float3) == sizeof(rvb_float3), "cl_float3");
static_assert(sizeof(Surface) == sizeof(rvb_surface), "Surface");
static_assert(sizeof(Impulse) == sizeof(rvb_impulse), "Impulse");
static_assert(sizeof(AttenuatedImpulse) == sizeof(rvb_attenuated_impulse), "AttenuatedImpulse");
static_assert(sizeof(Speaker) == sizeof(rvb_speaker), "Speaker");

namespace {

int device_from_env()
{
    const char * e = std::getenv("RVB_DEVICE");
    return e ? std::atoi(e) : 0;
}

int devices_from_env()
{
    const char * e = std::getenv("RVB_DEVICES");
    return e ? std::max(1, std::atoi(e)) : 1;
}

std::shared_ptr<rvb_ctx> make_context()
{
    rvb_ctx * raw = nullptr;
    const int rc = rvb_create(&raw, device_from_env(), 0);
    if (rc != RVB_OK)
        throw cl::Error(rc, rvb_last_error(nullptr));       // the reference throws cl::Error from cl::Context
    return std::shared_ptr<rvb_ctx>(raw, rvb_destroy);
}

// flattenImpulses is a free function in the reference; it gets a lazily created context of its own.
rvb_ctx * shared_context()
{
    static std::shared_ptr<rvb_ctx> ctx = make_context();
    return ctx.get();
}

// A std::vector of n elements whose storage is NOT value-initialised: the vectors this API returns hold up to a gigabyte that
// the next line overwrites from the device, and std::vector<T>(n) would first zero-fill it on one core (0.1-0.15 s per
// 819 MB vector).  libstdc++ only (the size is set through the vector base's own pointers); any other standard library gets
// the ordinary zero-filled vector.
template <class T>
std::vector<T> uninitialized_vector(size_t n)
{
#if defined(__GLIBCXX__) && !defined(_GLIBCXX_DEBUG) && !defined(RVB_SAFE_VECTORS)
    struct Access : std::vector<T> {
        void adopt(size_t count) { this->_M_impl._M_finish = this->_M_impl._M_start + count; }
    };
    static_assert(sizeof(Access) == sizeof(std::vector<T>), "no state of its own");
    std::vector<T> v;
    v.reserve(n);
    static_cast<Access &>(v).adopt(n);         // T is a POD of this library (Impulse, AttenuatedImpulse)
    // the buffer is fresh address space that the download is about to touch for the first time: ask for 2 MiB pages (400 page
    // faults instead of 200 000 per 819 MB where the kernel grants them)
    static const bool huge = !(std::getenv("RVB_HUGE_PAGES") && std::getenv("RVB_HUGE_PAGES")[0] == '0');
    if (huge && n * sizeof(T) >= (8u << 20)) {
        const uintptr_t lo = (reinterpret_cast<uintptr_t>(v.data()) + (2u << 20) - 1) & ~(uintptr_t) ((2u << 20) - 1);
        const uintptr_t hi = (reinterpret_cast<uintptr_t>(v.data()) + n * sizeof(T)) & ~(uintptr_t) ((2u << 20) - 1);
        if (hi > lo) (void) madvise(reinterpret_cast<void *>(lo), hi - lo, MADV_HUGEPAGE);
    }
    return v;
#else
    return std::vector<T>(n);
#endif
}

unsigned host_threads()
{
    static const unsigned n = [] {
        if (const char * e = std::getenv("RVB_HOST_THREADS")) return (unsigned) std::max(1, std::atoi(e));
        const unsigned hw = std::thread::hardware_concurrency();
        return std::max(1u, std::min(8u, hw ? hw / 2 : 4u));
    }();
    return n;
}

// f(first, last) over [0, n) on several threads
template <class F>
void parallel_ranges(size_t n, F f)
{
    const size_t threads = n < (1u << 16) ? 1 : host_threads();
    if (threads <= 1) { f((size_t) 0, n); return; }
    std::vector<std::thread> pool;
    const size_t per = (n + threads - 1) / threads;
    for (size_t t = 0; t < threads; ++t) {
        const size_t lo = t * per, hi = std::min(n, lo + per);
        if (lo >= hi) break;
        pool.emplace_back([=] { f(lo, hi); });
    }
    for (std::thread & t : pool) t.join();
}

// the one ResidentCache of the process (resident_cache.h: the mechanism, the caller's promise and why it is opt-in).  Never
// destroyed: whatever it still holds at exit is abandoned without a device call, as the shared context goes away beside it.
ResidentCache & resident()
{
    static ResidentCache * const cache = [] {
        const char * e = std::getenv("RVB_API_RESIDENT");
        return new ResidentCache(e && e[0] == '1', (size_t) 6 << 30, 251);
    }();
    return *cache;
}

// a device allocation of the shared context under an owner: freed when the last holder (the cache, a reader) lets go
std::shared_ptr<void> owned_device(void * d_ptr)
{
    return std::shared_ptr<void>(d_ptr, [](void * p) { (void) rvb_device_free(shared_context(), p); });
}

// rvb_device_alloc that gives the resident cache's device copies back before it reports a failure
int device_alloc_evicting(rvb_ctx * ctx, uint64_t bytes, void ** d_ptr)
{
    int rc = rvb_device_alloc(ctx, bytes, d_ptr);
    if (rc != RVB_OK && resident().evict(0))
        rc = rvb_device_alloc(ctx, bytes, d_ptr);
    return rc;
}

void throw_on(int rc, rvb_ctx * ctx, const char * where)
{
    if (rc != RVB_OK)
        throw cl::Error(rc, (std::string(where) + ": " + rvb_last_error(ctx)).c_str());
}

}  // namespace

// ---- context -------------------------------------------------------------------------------------

ContextProvider::ContextProvider() : ctx_(make_context()) {}

void ContextProvider::check(int rc, const char * where) const { throw_on(rc, ctx_.get(), where); }

void Raytracer::check_multi(int rc, const char * where) const
{
    if (rc != RVB_OK)
        throw cl::Error(rc, (std::string(where) + ": " + rvb_multi_last_error(multi_.get())).c_str());
}

KernelLoader::KernelLoader() : KernelLoader(false) {}

KernelLoader::KernelLoader(bool verbose)
{
    if (verbose) {
        char arch[64];
        int cus = 0;
        uint64_t hbm = 0;
        check(rvb_device_info(context(), arch, sizeof(arch), &cus, &hbm), "rvb_device_info");
        std::cerr << "rvb: " << arch << ", " << cus << " compute units, " << (hbm >> 30) << " GiB HBM (ahead-of-time kernels, no build log)"
                  << std::endl;
    }
}

// ---- time binning and predelay -------------------------------------------------------------------------

std::vector<std::vector<float>> flattenImpulses(const std::vector<AttenuatedImpulse> & impulse, float samplerate)
{
    rvb_ctx * ctx = shared_context();
    uint64_t nbins = 0;
    std::vector<float> flat;
    const ResidentCache::Found r = resident().find(impulse.data(), impulse.size(), sizeof(AttenuatedImpulse));
    const bool have = r && r.device_count == impulse.size();      // the attenuator's device copy (kept in step by fixPredelay): no upload
    const rvb_attenuated_impulse * in = reinterpret_cast<const rvb_attenuated_impulse *>(impulse.data());
    auto flatten = [&](float * out, uint64_t capacity) {
        if (have) throw_on(rvb_flatten_device(ctx, r.device, impulse.size(), samplerate, out, capacity, &nbins), ctx, "rvb_flatten_device");
        else throw_on(rvb_flatten(ctx, in, impulse.size(), samplerate, out, capacity, &nbins), ctx, "rvb_flatten");
    };
    flatten(nullptr, 0);                       // the size query: uploads once where nothing is resident, leaves array and keys on the device ...
    flat.resize(8 * nbins);
    flatten(flat.data(), nbins);               // ... and the fill works from them, not from another upload
    std::vector<std::vector<float>> flattened(sizeof(VolumeType) / sizeof(float));
    for (size_t b = 0; b < flattened.size(); ++b)
        flattened[b].assign(flat.begin() + (long) (b * nbins), flat.begin() + (long) ((b + 1) * nbins));
    return flattened;
}

std::vector<std::vector<std::vector<float>>> flattenImpulses(const std::vector<std::vector<AttenuatedImpulse>> & attenuated, float samplerate)
{
    std::vector<std::vector<std::vector<float>>> flattened(attenuated.size());
    for (size_t i = 0; i < attenuated.size(); ++i)
        flattened[i] = flattenImpulses(attenuated[i], samplerate);
    return flattened;
}

// reference rayverb.h:49-74: the smallest non-zero time, 0 if there is none (min is order-independent: threads may split the range)
float findPredelay(const std::vector<AttenuatedImpulse> & ret)
{
    std::mutex m;
    float a = 0.0f;
    parallel_ranges(ret.size(), [&](size_t lo, size_t hi) {
        float part = 0.0f;                     // one partial per range
        for (size_t i = lo; i < hi; ++i) {
            const float pd = ret[i].time;
            if (pd != 0.0f && (part == 0.0f || pd < part)) part = pd;
        }
        std::lock_guard<std::mutex> lock(m);
        if (part != 0.0f && (a == 0.0f || part < a)) a = part;
    });
    return a;
}

float findPredelay(const std::vector<std::vector<AttenuatedImpulse>> & ret)
{
    float a = 0.0f;
    for (const std::vector<AttenuatedImpulse> & channel : ret) {
        const float pd = findPredelay(channel);
        if (pd != 0.0f && (a == 0.0f || pd < a)) a = pd;
    }
    return a;
}

// reference rayverb.h:76-90, on the host vector and on its device copy if there is one
void fixPredelay(std::vector<AttenuatedImpulse> & ret, float seconds)
{
    // the device copy takes part only if the vector still reads as it did when the copy was made (sample comparison)
    const ResidentCache::Found r = resident().find(ret.data(), ret.size(), sizeof(AttenuatedImpulse));
    const bool have = r && r.owned && r.device_count == ret.size();
    AttenuatedImpulse * a = ret.data();
    parallel_ranges(ret.size(), [a, seconds](size_t lo, size_t hi) {
        for (size_t i = lo; i < hi; ++i) a[i].time = a[i].time > seconds ? a[i].time - seconds : 0;
    });
    if (!have) return;
    rvb_ctx * ctx = shared_context();
    throw_on(rvb_fix_predelay_device(ctx, r.device, r.device_count, seconds), ctx, "rvb_fix_predelay_device");
    resident().resample(ret.data(), ret.size(), sizeof(AttenuatedImpulse));
}

void fixPredelay(std::vector<std::vector<AttenuatedImpulse>> & ret, float seconds)
{
    for (std::vector<AttenuatedImpulse> & channel : ret)
        fixPredelay(channel, seconds);
}

void fixPredelay(std::vector<AttenuatedImpulse> & ret) { fixPredelay(ret, findPredelay(ret)); }
void fixPredelay(std::vector<std::vector<AttenuatedImpulse>> & ret) { fixPredelay(ret, findPredelay(ret)); }

// ---- ray tracer ------------------------------------------------------------------------------------

struct Raytracer::SceneData : public LoadedScene {
    SceneData(const std::string & objpath, const std::string & materialFileName, bool verbose)
        : LoadedScene(loadScene(objpath, materialFileName, verbose)) {}
};

namespace {

// reference rayverb.cpp:194-239
std::pair<cl_float3, cl_float3> getBounds(const std::vector<cl_float3> & vertices)
{
    cl_float3 lo = {{0, 0, 0, 0}}, hi = {{0, 0, 0, 0}};
    if (!vertices.empty()) {
        lo = hi = vertices.front();
        for (const cl_float3 & v : vertices)
            for (int i = 0; i < 4; ++i) {
                lo.s[i] = std::min(lo.s[i], v.s[i]);
                hi.s[i] = std::max(hi.s[i], v.s[i]);
            }
    }
    return std::make_pair(lo, hi);
}

bool inside(const std::pair<cl_float3, cl_float3> & bounds, const cl_float3 & point)
{
    // the reference loops over all four lanes of cl_float3 (rayverb.cpp:235); lane 3 is padding
    for (int i = 0; i < 3; ++i)
        if (!(bounds.first.s[i] <= point.s[i] && point.s[i] <= bounds.second.s[i]))
            return false;
    return true;
}

}  // namespace

Raytracer::Raytracer(unsigned long nreflections, std::vector<Triangle> & triangles, std::vector<cl_float3> & vertices,
                     std::vector<Surface> & surfaces, bool verbose)
    : KernelLoader(verbose), nreflections(nreflections), nrays(0), bounds(getBounds(vertices))
{
    storedMicpos = cl_float3{{0, 0, 0, 0}};
    upload(triangles, vertices, surfaces);
}

Raytracer::Raytracer(unsigned long nreflections, const std::string & objpath, const std::string & materialFileName, bool verbose)
    : Raytracer(nreflections, SceneData(objpath, materialFileName, verbose), verbose)
{
}

Raytracer::Raytracer(unsigned long nreflections, SceneData sceneData, bool verbose)
    : Raytracer(nreflections, sceneData.triangles, sceneData.vertices, sceneData.surfaces, verbose)
{
}

void Raytracer::upload(std::vector<Triangle> & triangles, std::vector<cl_float3> & vertices, std::vector<Surface> & surfaces)
{
    const int ndev = devices_from_env();
    if (ndev > 1) {
        rvb_multi * raw = nullptr;
        const int rc = rvb_multi_create(&raw, nullptr, ndev, 0);
        if (rc != RVB_OK)
            throw cl::Error(rc, rvb_last_error(nullptr));
        multi_ = std::shared_ptr<rvb_multi>(raw, rvb_multi_destroy);
        check_multi(rvb_multi_set_scene(raw, reinterpret_cast<const rvb_triangle *>(triangles.data()), triangles.size(),
                                        reinterpret_cast<const rvb_float3 *>(vertices.data()), vertices.size(),
                                        reinterpret_cast<const rvb_surface *>(surfaces.data()), surfaces.size()),
                    "rvb_multi_set_scene");
        return;
    }
    check(rvb_set_scene(context(), reinterpret_cast<const rvb_triangle *>(triangles.data()), triangles.size(),
                        reinterpret_cast<const rvb_float3 *>(vertices.data()), vertices.size(),
                        reinterpret_cast<const rvb_surface *>(surfaces.data()), surfaces.size()),
          "rvb_set_scene");
}

Raytracer::~Raytracer()
{
    // entries that borrow the context's trace buffer: void once the context may go away (copies of this object share the
    // context; treating every destruction as the end of the buffer only costs an upload)
    resident().owner_traces(context());
}

void Raytracer::raytrace(const cl_float3 & micpos, const cl_float3 & source, const std::vector<cl_float3> & directions, bool verbose)
{
    storedMicpos = micpos;
    resident().owner_traces(context());        // the trace buffer is about to be overwritten (copies of this object share it)

    // reference rayverb.cpp:547-583: warn when mic or source lie outside the model's bounding box
    const bool micinside = inside(bounds, micpos);
    const bool srcinside = inside(bounds, source);
    if (verbose && !(micinside && srcinside)) {
        std::cerr << "model bounds: [" << bounds.first.s[0] << ", " << bounds.first.s[1] << ", " << bounds.first.s[2] << "], ["
                  << bounds.second.s[0] << ", " << bounds.second.s[1] << ", " << bounds.second.s[2] << "]" << std::endl;
        if (!micinside) {
            std::cerr << "WARNING: microphone position may be outside model" << std::endl;
            std::cerr << "mic position: [" << micpos.s[0] << ", " << micpos.s[1] << ", " << micpos.s[2] << "]" << std::endl;
        }
        if (!srcinside) {
            std::cerr << "WARNING: source position may be outside model" << std::endl;
            std::cerr << "src position: [" << source.s[0] << ", " << source.s[1] << ", " << source.s[2] << "]" << std::endl;
        }
    }

    // air absorption per band, reference rayverb.cpp:632-641
    const float air[8] = {(float) (0.001 * -0.1), (float) (0.001 * -0.2), (float) (0.001 * -0.5), (float) (0.001 * -1.1),
                          (float) (0.001 * -2.7), (float) (0.001 * -9.4), (float) (0.001 * -29.0), (float) (0.001 * -60.0)};
    nrays = directions.size();
    if (multi_) {
        int rc = rvb_multi_set_directions(multi_.get(), reinterpret_cast<const rvb_float3 *>(directions.data()), directions.size());
        if (rc == RVB_OK) rc = rvb_multi_trace(multi_.get(), micpos.s, source.s, nreflections, air);     // blocking, every device at once
        check_multi(rc, "rvb_multi_trace");
        return;
    }
    check(rvb_set_directions(context(), reinterpret_cast<const rvb_float3 *>(directions.data()), directions.size()), "rvb_set_directions");
    check(rvb_trace(context(), micpos.s, source.s, nreflections, air, 0), "rvb_trace");
    check(rvb_synchronize(context()), "rvb_synchronize");     // the reference's raytrace() is blocking
}

void Raytracer::setSourcePattern(const cl_float3 & direction, const std::array<float, 8> & shape)
{
    rvb_source_pattern p;
    for (int i = 0; i < 4; ++i) p.direction[i] = direction.s[i];
    for (int b = 0; b < 8; ++b) p.shape[b] = shape[(size_t) b];
    if (multi_) {
        check_multi(rvb_multi_set_source_pattern(multi_.get(), &p), "rvb_multi_set_source_pattern");
        return;
    }
    check(rvb_set_source_pattern(context(), &p, 1), "rvb_set_source_pattern");
}

void Raytracer::clearSourcePattern()
{
    if (multi_) (void) rvb_multi_set_source_pattern(multi_.get(), nullptr);
    else check(rvb_set_source_pattern(context(), nullptr, 0), "rvb_set_source_pattern");
}

// diffuse impulses into out[0 .. nrays * nreflections), and the note that this buffer has a device copy
void Raytracer::fetchDiffuse(std::vector<Impulse> & out)
{
    const size_t n = nrays * nreflections;
    if (multi_) {                              // every device writes its slice of the array; no single device copy to remember
        check_multi(rvb_multi_get_diffuse(multi_.get(), reinterpret_cast<rvb_impulse *>(out.data())), "rvb_multi_get_diffuse");
        return;
    }
    const uint64_t stamp = resident().trace_count(context());       // read before the buffer is: a trace meanwhile voids the entry
    check(rvb_get_diffuse(context(), reinterpret_cast<rvb_impulse *>(out.data())), "rvb_get_diffuse");
    const void * d = nullptr;
    uint64_t count = 0;
    if (n && rvb_diffuse_device(context(), &d, &count) == RVB_OK && count == n)
        resident().remember_borrowed(out.data(), out.size(), sizeof(Impulse), const_cast<void *>(d), n, context(), stamp);
}

std::vector<Impulse> Raytracer::mergedImages(bool removeDirect)
{
    if (multi_) {
        uint64_t count = 0;
        int rc = rvb_multi_get_images(multi_.get(), removeDirect, nullptr, 0, &count);
        std::vector<Impulse> ret(count);
        if (rc == RVB_OK) rc = rvb_multi_get_images(multi_.get(), removeDirect, reinterpret_cast<rvb_impulse *>(ret.data()), count, &count);
        check_multi(rc, "rvb_multi_get_images");
        return ret;
    }
    uint64_t ncand = 0;
    check(rvb_get_image_candidates(context(), nullptr, 0, &ncand), "rvb_get_image_candidates");
    std::vector<rvb_image_candidate> cand(ncand);
    check(rvb_get_image_candidates(context(), cand.data(), cand.size(), &ncand), "rvb_get_image_candidates");
    rvb_impulse direct;
    check(rvb_get_direct(context(), &direct), "rvb_get_direct");
    const rvb_impulse * direct_ptr = nrays ? &direct : nullptr;
    uint64_t count = 0;
    check(rvb_merge_images(cand.data(), cand.size(), direct_ptr, removeDirect, nullptr, 0, &count), "rvb_merge_images");
    std::vector<Impulse> ret(count);
    check(rvb_merge_images(cand.data(), cand.size(), direct_ptr, removeDirect, reinterpret_cast<rvb_impulse *>(ret.data()), count, &count),
          "rvb_merge_images");
    return ret;
}

RaytracerResults Raytracer::getRawDiffuse()
{
    std::vector<Impulse> diffuse = uninitialized_vector<Impulse>(nrays * nreflections);
    fetchDiffuse(diffuse);
    return RaytracerResults(std::move(diffuse), storedMicpos);
}

RaytracerResults Raytracer::getRawImages(bool removeDirect)
{
    return RaytracerResults(mergedImages(removeDirect), storedMicpos);
}

RaytracerResults Raytracer::getAllRaw(bool removeDirect)
{
    // diffuse, then images (reference rayverb.cpp:708-714) — built in one buffer, no intermediate vectors
    const std::vector<Impulse> image = mergedImages(removeDirect);
    const size_t nd = nrays * nreflections;
    std::vector<Impulse> all = uninitialized_vector<Impulse>(nd + image.size());
    std::copy(image.begin(), image.end(), all.begin() + (long) nd);
    fetchDiffuse(all);
    return RaytracerResults(std::move(all), storedMicpos);
}

// ---- attenuators -------------------------------------------------------------------------------------

namespace {

typedef std::array<std::array<std::array<cl_float8, 180>, 360>, 2> HrtfTable;

// The reference's HRTF_DATA (rayverb/hrtf.cpp, derived from the IRCAM Listen database) is not part
// of the reference checkout (.MISSING_LARGE_BLOBS).  This stand-in is a smooth analytic head-shadow
// pattern with the same shape; override getHrtfData() to supply measured data.
const HrtfTable & standin_hrtf()
{
    static HrtfTable storage;                 // static storage honours the 32-byte alignment of cl_float8
    static HrtfTable * const table = &storage;
    static std::once_flag once;
    std::call_once(once, [] {
        const double pi = 3.14159265358979323846;
        for (int ch = 0; ch < 2; ++ch) {
            const double sign = ch == 0 ? -1.0 : 1.0;
            for (int a = 0; a < 360; ++a)
                for (int e = 0; e < 180; ++e) {
                    const double az = (a - 180.0) * pi / 180.0, el = (90.0 - e) * pi / 180.0;
                    const double lateral = sign * std::sin(az) * std::cos(el);
                    for (int b = 0; b < 8; ++b)
                        (*table)[ch][a][e].s[b] = (float) (0.55 + 0.45 * std::exp(-0.08 * (b + 1.0) * (1.0 - lateral)));
                }
        }
    });
    return *table;
}

}  // namespace

HrtfAttenuator::HrtfAttenuator() {}

const std::array<std::array<std::array<cl_float8, 180>, 360>, 2> & HrtfAttenuator::getHrtfData() const
{
    return standin_hrtf();
}

std::vector<std::vector<AttenuatedImpulse>> HrtfAttenuator::attenuate(const RaytracerResults & results, const HrtfConfig & config)
{
    return attenuate(results, config.facing, config.up);
}

// The impulses of `results` on the shared context's device: the trace buffer they were downloaded from when the vector is
// the one getAllRaw / getRawDiffuse returned (plus the few image impulses behind it), else an upload.
namespace {
struct DeviceImpulses {
    explicit DeviceImpulses(rvb_ctx * c) : ctx(c) {}
    DeviceImpulses(const DeviceImpulses &) = delete;
    DeviceImpulses & operator=(const DeviceImpulses &) = delete;
    rvb_ctx * ctx;
    const void * head = nullptr;      // first `nhead` impulses (a Raytracer's trace buffer, borrowed, or the whole upload)
    size_t nhead = 0;
    void * tail = nullptr;            // the rest (uploaded; owned)
    size_t ntail = 0;
    void * upload = nullptr;          // owned storage behind `head` when nothing was resident
    std::shared_ptr<void> lease;      // the reader's reference to a resident `head`
    ~DeviceImpulses()
    {
        if (tail) (void) rvb_device_free(ctx, tail);
        if (upload) (void) rvb_device_free(ctx, upload);
    }
    // launch(input, count, output) on the head, then on the tail behind the head's results
    template <class Launch>
    int launch_parts(void * d_out, Launch launch) const
    {
        int rc = launch(head, nhead, d_out);
        if (rc == RVB_OK && ntail) rc = launch(tail, ntail, static_cast<char *>(d_out) + nhead * sizeof(AttenuatedImpulse));
        return rc;
    }
};

void stage_impulses(const std::vector<Impulse> & impulses, DeviceImpulses & dev)
{
    rvb_ctx * ctx = dev.ctx;
    const size_t n = impulses.size();
    const ResidentCache::Found r = resident().find(impulses.data(), n, sizeof(Impulse));
    if (r && !r.owned && r.device_count <= n) {
        // getRawDiffuse / getAllRaw: the diffuse impulses are still in the tracer's buffer; the few image impulses that
        // getAllRaw put behind them come from the host vector
        dev.lease = r.lease;
        dev.head = r.device;
        dev.nhead = r.device_count;
        dev.ntail = n - r.device_count;
        if (dev.ntail) {
            throw_on(device_alloc_evicting(ctx, dev.ntail * sizeof(Impulse), &dev.tail), ctx, "rvb_device_alloc");
            throw_on(rvb_copy_to_device(ctx, dev.tail, impulses.data() + dev.nhead, dev.ntail * sizeof(Impulse)), ctx, "rvb_copy_to_device");
        }
        return;
    }
    if (n == 0) return;
    throw_on(device_alloc_evicting(ctx, n * sizeof(Impulse), &dev.upload), ctx, "rvb_device_alloc");
    throw_on(rvb_copy_to_device(ctx, dev.upload, impulses.data(), n * sizeof(Impulse)), ctx, "rvb_copy_to_device");
    dev.head = dev.upload;
    dev.nhead = n;
}

// one channel: kernel on the staged input, result downloaded into a fresh vector whose device copy is remembered
template <class Launch>
std::vector<AttenuatedImpulse> attenuate_channel(const DeviceImpulses & dev, Launch launch)
{
    rvb_ctx * ctx = dev.ctx;
    const size_t n = dev.nhead + dev.ntail;
    std::vector<AttenuatedImpulse> ret = uninitialized_vector<AttenuatedImpulse>(n);
    if (n == 0) return ret;
    void * d_out = nullptr;
    throw_on(device_alloc_evicting(ctx, n * sizeof(AttenuatedImpulse), &d_out), ctx, "rvb_device_alloc");
    std::shared_ptr<void> out = owned_device(d_out);          // freed by whoever holds it last: this frame on an error or with the cache off
    int rc = dev.launch_parts(d_out, launch);
    if (rc == RVB_OK) rc = rvb_copy_to_host(ctx, ret.data(), d_out, n * sizeof(AttenuatedImpulse));
    throw_on(rc, ctx, "attenuate");
    resident().remember_owned(ret.data(), n, sizeof(AttenuatedImpulse), std::move(out));
    return ret;
}
}  // namespace

std::vector<std::vector<AttenuatedImpulse>> HrtfAttenuator::attenuate(const RaytracerResults & results, const cl_float3 & facing, const cl_float3 & up)
{
    // channels {0, 1}, rayverb.cpp:751.  The kernels run on the library's shared context: this object is usually a temporary
    // (cmd/main.cpp:286) and the device copies of what it returns have to outlive it.
    DeviceImpulses dev(shared_context());
    stage_impulses(results.impulses, dev);
    std::vector<std::vector<AttenuatedImpulse>> attenuated(2);
    for (unsigned long ch = 0; ch < 2; ++ch) {
        // [360][180] of cl_float8 is contiguous: exactly the flattened table of rayverb.cpp:774-780
        const float * table = reinterpret_cast<const float *>(getHrtfData()[ch].data());
        const cl_float3 mic = results.mic;
        attenuated[ch] = attenuate_channel(dev, [&](const void * in, size_t count, void * d_out) {
            return rvb_attenuate_hrtf_device(dev.ctx, mic.s, in, count, table, facing.s, up.s, ch, d_out);
        });
    }
    return attenuated;
}

SpeakerAttenuator::SpeakerAttenuator() {}

std::vector<std::vector<AttenuatedImpulse>> SpeakerAttenuator::attenuate(const RaytracerResults & results, const std::vector<Speaker> & speakers)
{
    // the impulse array is staged ONCE for all speakers (the reference uploads it per speaker, rayverb.cpp:863-875)
    DeviceImpulses dev(shared_context());
    stage_impulses(results.impulses, dev);
    std::vector<std::vector<AttenuatedImpulse>> attenuated(speakers.size());
    for (size_t i = 0; i < speakers.size(); ++i) {
        const cl_float3 mic = results.mic;
        const rvb_speaker * sp = reinterpret_cast<const rvb_speaker *>(&speakers[i]);
        attenuated[i] = attenuate_channel(dev, [&](const void * in, size_t count, void * d_out) {
            return rvb_attenuate_speaker_device(dev.ctx, mic.s, in, count, sp, d_out);
        });
    }
    return attenuated;
}
