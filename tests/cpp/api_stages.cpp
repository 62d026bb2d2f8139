// api_stages.cpp — the reference's production call sequence (cmd/main.cpp:241-298) through the C++ mirror of its classes, with EVERY
// stage's result written out as raw bytes: tests/test_gpu_cpp_stages.py holds each file to the CPU oracle, tests/test_predelay_host.py
// the predelay functions alone.  Arguments are name=value pairs in any order; out= names an existing directory.
//
//   mode=trace    triangles= vertices= surfaces= directions= nrefl= source=x,y,z mic=x,y,z  <model>  rate=
//       Raytracer(nrefl, triangles, vertices, surfaces, false), raytrace, then
//       getRawDiffuse -> diffuse.bin, getRawImages(false / true) -> images_0.bin / images_1.bin, getAllRaw(false / true) -> all_0.bin /
//       all_1.bin, and attenuate(getAllRaw(false), ...) with the steps below
//   mode=records  records= mic=x,y,z  <model>  rate=
//       RaytracerResults(records, mic) -> attenuate with the steps below
//   mode=predelay channels=N in=PREFIX         (never constructs a context: nothing is resident, no device call)
//       the library's findPredelay / fixPredelay overloads and the header's templates on PREFIX0.bin .. PREFIX<N-1>.bin
//
//   <model>: speakers=FILE (Speaker records)  |  hrtf=FILE ([2][360][180][8] floats, returned by an overridden getHrtfData())
//            facing=x,y,z up=x,y,z
//   steps behind attenuate, c = channel: attenuated_c.bin; flattenImpulses before any predelay step -> flat_raw_c.bin;
//       findPredelay -> predelay.bin (one float; per_channel=1: one per channel); fixPredelay -> fixed_c.bin;
//       flattenImpulses -> flat_c.bin (8 bands of the channel's own length, band after band)
//   handover=vectors  every stage gets the very vectors the stage before returned (cmd/main.cpp does this)
//   handover=copies   every stage gets a copy in a fresh buffer
//   per_channel=1     findPredelay and fixPredelay channel by channel, each channel with its own predelay
#include "rayverb/rayverb.h"

#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <fstream>
#include <iostream>
#include <map>
#include <sstream>

typedef std::array<std::array<std::array<cl_float8, 180>, 360>, 2> HrtfTable;
typedef std::vector<std::vector<AttenuatedImpulse>> Channels;

static std::map<std::string, std::string> args;

static const std::string & arg(const std::string & name)
{
    const auto it = args.find(name);
    if (it == args.end()) { std::cerr << "api_stages: missing argument " << name << "=" << std::endl; std::exit(1); }
    return it->second;
}

static bool has(const std::string & name) { return args.count(name) != 0; }

static cl_float3 arg_float3(const std::string & name)
{
    cl_float3 v = {{0, 0, 0, 0}};
    std::stringstream in(arg(name));
    std::string word;
    for (int i = 0; i < 3 && std::getline(in, word, ','); ++i)
        v.s[i] = std::strtof(word.c_str(), nullptr);      // "%.9g" text of a binary32 value: reads back exactly
    return v;
}

static void slurp_bytes(const std::string & path, void * to, size_t bytes)
{
    std::ifstream f(path.c_str(), std::ios::binary);
    if (!f || (bytes && !f.read(static_cast<char *>(to), (std::streamsize) bytes))) { std::cerr << "api_stages: cannot read " << path << std::endl; std::exit(1); }
}

template <class T> static std::vector<T> slurp(const std::string & path)
{
    std::ifstream f(path.c_str(), std::ios::binary | std::ios::ate);
    if (!f) { std::cerr << "api_stages: cannot open " << path << std::endl; std::exit(1); }
    const size_t bytes = (size_t) f.tellg();
    f.close();
    if (bytes % sizeof(T)) { std::cerr << "api_stages: " << path << " is no whole number of records" << std::endl; std::exit(1); }
    std::vector<T> v(bytes / sizeof(T));
    slurp_bytes(path, v.data(), bytes);
    return v;
}

static void dump_bytes(const std::string & name, const void * from, size_t bytes)
{
    const std::string path = arg("out") + "/" + name;
    std::ofstream f(path.c_str(), std::ios::binary);
    if (bytes) f.write(static_cast<const char *>(from), (std::streamsize) bytes);
    f.close();
    if (!f) { std::cerr << "api_stages: cannot write " << path << std::endl; std::exit(1); }
}

template <class T> static void dump(const std::string & name, const std::vector<T> & v) { dump_bytes(name, v.data(), v.size() * sizeof(T)); }

static std::string numbered(const char * stem, size_t c) { return std::string(stem) + std::to_string(c) + ".bin"; }

// the table of the file behind the hook the reference's own test fixture overrides (tests/hrtf_tests.h:28)
class FileHrtf : public HrtfAttenuator {
public:
    explicit FileHrtf(const std::string & path)
    {
        static HrtfTable storage;                  // static storage honours the 32-byte alignment of cl_float8
        slurp_bytes(path, &storage, sizeof(storage));
        table = &storage;
    }
    virtual const HrtfTable & getHrtfData() const { return *table; }
private:
    const HrtfTable * table;
};

static bool copies;

// what a stage is handed: the caller's vector itself, or (handover=copies) the same values in a fresh buffer
template <class T> static const T & handed(const T & mine, T & scratch)
{
    if (!copies) return mine;
    scratch = T();
    scratch = mine;
    return scratch;
}

static Channels attenuate(const RaytracerResults & results)
{
    if (has("speakers"))
        return SpeakerAttenuator().attenuate(results, slurp<Speaker>(arg("speakers")));     // every speaker in ONE call: one staging
    return FileHrtf(arg("hrtf")).attenuate(results, arg_float3("facing"), arg_float3("up"));
}

// everything behind the tracer
static void later_stages(const RaytracerResults & results)
{
    const float rate = std::strtof(arg("rate").c_str(), nullptr);
    const bool per_channel = has("per_channel") && arg("per_channel") == "1";
    RaytracerResults results_copy;
    if (copies) results_copy = RaytracerResults(results.impulses, results.mic);
    Channels attenuated = attenuate(copies ? results_copy : results);
    for (size_t c = 0; c < attenuated.size(); ++c) dump(numbered("attenuated_", c), attenuated[c]);

    Channels scratch;
    {
        const auto flat = flattenImpulses(handed(attenuated, scratch), rate);
        for (size_t c = 0; c < flat.size(); ++c) {
            std::vector<float> bands;
            for (const std::vector<float> & band : flat[c]) bands.insert(bands.end(), band.begin(), band.end());
            dump(numbered("flat_raw_", c), bands);
        }
    }

    if (copies) { Channels fresh = attenuated; attenuated.swap(fresh); }                     // the predelay steps edit a copy
    std::vector<float> predelay;
    if (per_channel) {
        for (std::vector<AttenuatedImpulse> & channel : attenuated) {
            predelay.push_back(findPredelay(channel));
            fixPredelay(channel);
        }
    } else {
        predelay.push_back(findPredelay(attenuated));
        fixPredelay(attenuated);
    }
    dump("predelay.bin", predelay);
    for (size_t c = 0; c < attenuated.size(); ++c) dump(numbered("fixed_", c), attenuated[c]);

    const auto flat = flattenImpulses(handed(attenuated, scratch), rate);
    for (size_t c = 0; c < flat.size(); ++c) {
        if (flat[c].size() != 8) { std::cerr << "api_stages: " << flat[c].size() << " bands" << std::endl; std::exit(1); }
        std::vector<float> bands;
        for (const std::vector<float> & band : flat[c]) {
            if (band.size() != flat[c][0].size()) { std::cerr << "api_stages: bands of unequal length" << std::endl; std::exit(1); }
            bands.insert(bands.end(), band.begin(), band.end());
        }
        dump(numbered("flat_", c), bands);
    }
    std::printf("channels %zu\n", attenuated.size());
}

static void trace_mode()
{
    std::vector<Triangle> triangles = slurp<Triangle>(arg("triangles"));
    std::vector<cl_float3> vertices = slurp<cl_float3>(arg("vertices"));
    std::vector<Surface> surfaces = slurp<Surface>(arg("surfaces"));
    const std::vector<cl_float3> directions = slurp<cl_float3>(arg("directions"));
    Raytracer raytracer(std::strtoul(arg("nrefl").c_str(), nullptr, 10), triangles, vertices, surfaces, false);
    raytracer.raytrace(arg_float3("mic"), arg_float3("source"), directions, false);
    dump("diffuse.bin", raytracer.getRawDiffuse().impulses);
    dump("images_0.bin", raytracer.getRawImages(false).impulses);
    dump("images_1.bin", raytracer.getRawImages(true).impulses);
    const RaytracerResults all = raytracer.getAllRaw(false);
    dump("all_0.bin", all.impulses);
    dump("all_1.bin", raytracer.getAllRaw(true).impulses);
    later_stages(all);
}

static void records_mode()
{
    later_stages(RaytracerResults(slurp<Impulse>(arg("records")), arg_float3("mic")));
}

// ---- mode=predelay ---------------------------------------------------------------------------------------------------------------------

// A record the library has no overloads for: findPredelay / fixPredelay on vectors of it can only be the header's templates, all the
// way down to the AttenuatedImpulse overloads (a plain std::vector<AttenuatedImpulse> inside a template would pick the library's).
struct Plain : AttenuatedImpulse {};
static_assert(sizeof(Plain) == sizeof(AttenuatedImpulse), "same record");

template <class T> static std::vector<float> times_of(const std::vector<T> & v)
{
    std::vector<float> t(v.size());
    for (size_t i = 0; i < v.size(); ++i) t[i] = v[i].time;
    return t;
}

// records whose volume or padding no longer reads as in `before`
template <class T, class U> static size_t touched(const std::vector<T> & after, const std::vector<U> & before)
{
    size_t n = after.size() == before.size() ? 0 : 1;
    for (size_t i = 0; i < after.size() && i < before.size(); ++i) {
        AttenuatedImpulse a = after[i], b = before[i];
        a.time = b.time = 0;
        n += std::memcmp(&a, &b, sizeof(a)) != 0;
    }
    return n;
}

// For the library (T = AttenuatedImpulse) and the templates (T = Plain): the predelay of all channels and of each; the times after
// fixPredelay(all channels), after fixPredelay(channel) for each, and after fixPredelay(all channels, half the predelay).
template <class T> static size_t predelay_forms(const std::string & stem, const std::vector<std::vector<T>> & in)
{
    size_t bad = 0;
    std::vector<float> found(1, findPredelay(in));
    for (const std::vector<T> & channel : in) found.push_back(findPredelay(channel));
    dump(stem + "_find.bin", found);
    std::vector<std::vector<T>> nested = in, each = in, half = in;
    fixPredelay(nested);
    for (std::vector<T> & channel : each) fixPredelay(channel);
    fixPredelay(half, found[0] * 0.5f);
    for (size_t c = 0; c < in.size(); ++c) {
        dump(stem + numbered("_nested_", c), times_of(nested[c]));
        dump(stem + numbered("_each_", c), times_of(each[c]));
        dump(stem + numbered("_half_", c), times_of(half[c]));
        bad += touched(nested[c], in[c]) + touched(each[c], in[c]) + touched(half[c], in[c]);
    }
    return bad;
}

static void predelay_mode()
{
    const size_t n = std::strtoul(arg("channels").c_str(), nullptr, 10);
    std::vector<std::vector<AttenuatedImpulse>> in(n);
    std::vector<std::vector<Plain>> plain(n);
    for (size_t c = 0; c < n; ++c) {
        in[c] = slurp<AttenuatedImpulse>(arg("in") + std::to_string(c) + ".bin");
        plain[c] = slurp<Plain>(arg("in") + std::to_string(c) + ".bin");
    }
    const size_t bad = predelay_forms("library", in) + predelay_forms("template", plain);
    std::printf("touched %zu\n", bad);
}

int main(int argc, char ** argv)
{
    for (int i = 1; i < argc; ++i) {
        const char * eq = std::strchr(argv[i], '=');
        if (!eq) { std::cerr << "api_stages: not name=value: " << argv[i] << std::endl; return 1; }
        args[std::string(argv[i], (size_t) (eq - argv[i]))] = std::string(eq + 1);
    }
    try {
        const std::string & mode = arg("mode");
        if (mode == "predelay") { predelay_mode(); return 0; }
        copies = arg("handover") == "copies";
        if (!copies && arg("handover") != "vectors") { std::cerr << "api_stages: handover=vectors|copies" << std::endl; return 1; }
        if (mode == "trace") trace_mode();
        else if (mode == "records") records_mode();
        else { std::cerr << "api_stages: mode=trace|records|predelay" << std::endl; return 1; }
    } catch (const cl::Error & e) {
        std::cerr << "cl::Error " << e.err() << ": " << e.what() << std::endl;
        return 2;
    } catch (const std::exception & e) {
        std::cerr << "exception: " << e.what() << std::endl;
        return 3;
    }
    return 0;
}
