// test_pipeline_source.cpp — directional sources (rvb_set_source_pattern, rvb_pipeline_set_source_pattern, rvb_pipeline_submit_directed)
// through the pipeline and through the C++ mirror.  Eight speaker jobs, each with a source facing of its own, go through one lane of two
// contexts with one pair per launch and through two lanes of one context with two pairs per launch (the per-pair form of the pattern);
// every histogram must equal, bit for bit, rvb_set_source_pattern + rvb_trace + rvb_merge_images + rvb_ir_configure_speakers +
// rvb_ir_download on a separate context (exact mode).  Then the refusals, a pipeline whose pattern is switched off again, and
// Raytracer::setSourcePattern through getAllRaw against the C-ABI's records.
// Exit code 0 = all passed; 2 = no GPU.
#include "rvb_capi.h"
#include "rayverb/rayverb.h"

#include <array>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

static int failures = 0;
#define CHECK(cond)                                                                   \
    do {                                                                              \
        if (!(cond)) { ++failures; std::printf("FAIL %s:%d: %s\n", __FILE__, __LINE__, #cond); } \
    } while (0)
#define OK(call)                                                                      \
    do {                                                                              \
        const int rc_ = (call);                                                       \
        if (rc_ != RVB_OK) { ++failures; std::printf("FAIL %s:%d: %s -> %d\n", __FILE__, __LINE__, #call, rc_); } \
    } while (0)

// a 24 x 9 x 14 m hall whose six walls are grids of quads (two triangles each) with a few pillars: 2 700 triangles
struct Scene {
    std::vector<rvb_triangle> tris;
    std::vector<rvb_float3> verts;
    std::vector<rvb_surface> surfaces;
    void quad_grid(const float o[3], const float du[3], const float dv[3], int nu, int nv, uint64_t surface)
    {
        const uint64_t base = verts.size();
        for (int j = 0; j <= nv; ++j)
            for (int i = 0; i <= nu; ++i) {
                rvb_float3 v;
                for (int k = 0; k < 3; ++k) v.s[k] = o[k] + du[k] * i + dv[k] * j;
                v.s[3] = 0.0f;
                verts.push_back(v);
            }
        for (int j = 0; j < nv; ++j)
            for (int i = 0; i < nu; ++i) {
                const uint64_t a = base + (uint64_t) j * (nu + 1) + i, b = a + 1, c = a + nu + 1, d = c + 1;
                tris.push_back(rvb_triangle{surface, a, b, d});
                tris.push_back(rvb_triangle{surface, a, d, c});
            }
    }
    void box(const float lo[3], const float hi[3], int n, uint64_t surface)
    {
        const float sx = (hi[0] - lo[0]) / n, sy = (hi[1] - lo[1]) / n, sz = (hi[2] - lo[2]) / n;
        const float X[3] = {sx, 0, 0}, Y[3] = {0, sy, 0}, Z[3] = {0, 0, sz};
        const float p[3] = {lo[0], lo[1], lo[2]}, qx[3] = {hi[0], lo[1], lo[2]}, qy[3] = {lo[0], hi[1], lo[2]}, qz[3] = {lo[0], lo[1], hi[2]};
        quad_grid(p, X, Y, n, n, surface); quad_grid(qz, X, Y, n, n, surface);
        quad_grid(p, X, Z, n, n, surface); quad_grid(qy, X, Z, n, n, surface);
        quad_grid(p, Y, Z, n, n, surface); quad_grid(qx, Y, Z, n, n, surface);
    }
    Scene()
    {
        for (int s = 0; s < 3; ++s) {
            rvb_surface sf;
            for (int b = 0; b < 8; ++b) { sf.specular[b] = 0.97f - 0.01f * b - 0.02f * s; sf.diffuse[b] = 0.9f - 0.03f * b; }
            surfaces.push_back(sf);
        }
        const float lo[3] = {-12.0f, 0.0f, -7.0f}, hi[3] = {12.0f, 9.0f, 7.0f};
        box(lo, hi, 14, 1);
        for (int k = 0; k < 4; ++k) {
            const float cx = -7.5f + 5.0f * k;
            const float plo[3] = {cx - 0.4f, 0.0f, 2.6f}, phi[3] = {cx + 0.4f, 6.5f, 3.4f};
            box(plo, phi, 3, 2);
        }
    }
};

static std::vector<rvb_float3> directions(uint64_t n, uint64_t seed)
{
    std::vector<rvb_float3> d(n);
    uint64_t x = seed * 0x9E3779B97F4A7C15ull + 1;
    auto next = [&x]() { x ^= x << 13; x ^= x >> 7; x ^= x << 17; return (double) (x >> 11) / 9007199254740992.0; };
    for (uint64_t i = 0; i < n; ++i) {
        const double z = 2.0 * next() - 1.0, th = 6.283185307179586 * next() - 3.141592653589793, r = std::sqrt(1.0 - z * z);
        d[i].s[0] = (float) (r * std::cos(th)); d[i].s[1] = (float) (r * std::sin(th)); d[i].s[2] = (float) z; d[i].s[3] = 0.0f;
    }
    return d;
}

static const float AIR[8] = {0.001f * -0.1f, 0.001f * -0.2f, 0.001f * -0.5f, 0.001f * -1.1f, 0.001f * -2.7f, 0.001f * -9.4f, 0.001f * -29.0f, 0.001f * -60.0f};

static const float SHAPE[8] = {0.0f, 0.125f, 0.25f, 0.5f, 0.625f, 0.75f, 0.875f, 1.0f};

static void job_geometry(int i, float mic[3], float src[3], float facing[3])
{
    mic[0] = -9.0f + 1.9f * i; mic[1] = 1.5f + 0.05f * (i % 5); mic[2] = -4.0f + 0.7f * i;
    src[0] = 8.0f - 1.5f * i; src[1] = 1.7f + 0.1f * (i % 3); src[2] = -5.0f + 0.3f * ((i * 7) % 20);
    // the source faces away from the microphone for odd jobs (gains of both signs), not a unit vector
    const float s = (i & 1) ? -2.0f : 0.5f;
    facing[0] = s * (mic[0] - src[0]); facing[1] = 0.3f * i; facing[2] = s * (mic[2] - src[2]);
}

static rvb_source_pattern pattern_of(const float facing[3])
{
    rvb_source_pattern p;
    for (int k = 0; k < 3; ++k) p.direction[k] = facing[k];
    p.direction[3] = 0.0f;
    std::memcpy(p.shape, SHAPE, sizeof(SHAPE));
    return p;
}

// the same impulse response by the step-by-step calls on one context (facing == NULL: no pattern)
static std::vector<float> solo_ir(rvb_ctx * ctx, const float mic[3], const float src[3], const float * facing, uint64_t nrefl, const rvb_speaker * sp,
                                  uint64_t nsp, uint64_t * nbins_out, uint64_t * nimages_out)
{
    if (facing) { const rvb_source_pattern p = pattern_of(facing); OK(rvb_set_source_pattern(ctx, &p, 1)); }
    else OK(rvb_set_source_pattern(ctx, nullptr, 0));
    OK(rvb_trace(ctx, mic, src, nrefl, AIR, 0));
    uint64_t ncand = 0, nimg = 0;
    OK(rvb_get_image_candidates(ctx, nullptr, 0, &ncand));
    std::vector<rvb_image_candidate> cand(ncand);
    if (ncand) OK(rvb_get_image_candidates(ctx, cand.data(), ncand, &ncand));
    rvb_impulse direct;
    OK(rvb_get_direct(ctx, &direct));
    OK(rvb_merge_images(cand.data(), ncand, &direct, 0, nullptr, 0, &nimg));
    std::vector<rvb_impulse> images(nimg);
    if (nimg) OK(rvb_merge_images(cand.data(), ncand, &direct, 0, images.data(), nimg, &nimg));
    OK(rvb_ir_configure_speakers(ctx, mic, sp, nsp, RVB_IR_ALL, images.data(), nimg));
    uint64_t nbins = 0;
    OK(rvb_ir_download(ctx, 1, 44100.0f, RVB_IR_EXACT, nullptr, 0, &nbins));
    std::vector<float> out((size_t) (nsp * 8 * nbins));
    OK(rvb_ir_download(ctx, 1, 44100.0f, RVB_IR_EXACT, out.data(), nbins, &nbins));
    *nbins_out = nbins;
    *nimages_out = nimg;
    return out;
}

struct Got {
    std::vector<float> hist;
    uint64_t job, nbins, nimages;
};

// all jobs through the pipeline, as many pending as it takes (`limit`: 2 x contexts x pairs per launch)
static std::vector<Got> run(rvb_pipeline * pipe, int njobs, uint64_t limit, bool directed)
{
    std::vector<Got> got;
    float mic[3], src[3], facing[3];
    int sent = 0;
    while ((int) got.size() < njobs) {
        while (sent < njobs && rvb_pipeline_pending(pipe) < limit) {
            job_geometry(sent, mic, src, facing);
            OK(rvb_pipeline_submit_directed(pipe, mic, src, nullptr, nullptr, directed ? facing : nullptr));
            ++sent;
        }
        rvb_pipeline_result res;
        const int rc = rvb_pipeline_next(pipe, &res);
        OK(rc);
        if (rc != RVB_OK) { std::printf("%s\n", rvb_pipeline_last_error(pipe)); break; }
        Got g;
        g.hist.assign(res.histogram, res.histogram + res.nchannels * 8 * res.nbins);
        g.job = res.job; g.nbins = res.nbins; g.nimages = res.nimages;
        got.push_back(g);
    }
    return got;
}

static bool same(const std::vector<float> & a, const std::vector<float> & b)
{
    return a.size() == b.size() && std::memcmp(a.data(), b.data(), a.size() * sizeof(float)) == 0;
}

int main()
{
    const uint64_t nrays = 6000, nrefl = 16;
    const int NJOBS = 8;
    Scene scene;
    const std::vector<rvb_float3> dirs = directions(nrays, 3);
    rvb_ctx * ctxs[3] = {nullptr, nullptr, nullptr};
    for (int i = 0; i < 3; ++i) {
        const int rc = rvb_create(&ctxs[i], 0, 0);
        if (rc != RVB_OK) { std::printf("rvb_create: %s\n", rvb_last_error(nullptr)); return 2; }      // no GPU: there is no CPU path
        if (i == 0 || i == 2) OK(rvb_set_scene(ctxs[i], scene.tris.data(), scene.tris.size(), scene.verts.data(), scene.verts.size(), scene.surfaces.data(), scene.surfaces.size()));
        else OK(rvb_share_scene(ctxs[i], ctxs[0]));
        OK(rvb_set_directions(ctxs[i], dirs.data(), dirs.size()));
    }
    rvb_ctx * solo = ctxs[2];
    rvb_speaker speakers[2];
    std::memset(speakers, 0, sizeof(speakers));
    speakers[0].direction[0] = -1.0f; speakers[0].direction[2] = -1.0f; speakers[0].coefficient = 0.5f;
    speakers[1].direction[0] = 1.0f; speakers[1].direction[2] = -1.0f; speakers[1].coefficient = 0.5f;
    const float default_facing[3] = {0.0f, 0.0f, 3.0f};

    // what every job must give, with its own facing, with the default facing and without a pattern (job 0 only)
    std::vector<std::vector<float> > want((size_t) NJOBS);
    std::vector<uint64_t> want_bins((size_t) NJOBS), want_images((size_t) NJOBS);
    float mic[3], src[3], facing[3];
    for (int i = 0; i < NJOBS; ++i) {
        job_geometry(i, mic, src, facing);
        want[(size_t) i] = solo_ir(solo, mic, src, facing, nrefl, speakers, 2, &want_bins[(size_t) i], &want_images[(size_t) i]);
        bool any = false;
        for (float v : want[(size_t) i]) any = any || v != 0.0f;
        CHECK(any);
    }
    job_geometry(0, mic, src, facing);
    uint64_t nb = 0, ni = 0;
    const std::vector<float> want_default = solo_ir(solo, mic, src, default_facing, nrefl, speakers, 2, &nb, &ni);
    const std::vector<float> want_plain = solo_ir(solo, mic, src, nullptr, nrefl, speakers, 2, &nb, &ni);
    CHECK(!same(want_default, want[0]) && !same(want_plain, want[0]) && !same(want_plain, want_default));

    for (int form = 0; form < 2; ++form) {
        // form 0: one lane of two contexts, one pair per launch; form 1: two lanes of one context, two pairs per launch
        rvb_pipeline * pipe = nullptr;
        const uint64_t one_lane[1] = {2}, two_lanes[2] = {1, 1};
        rvb_pipeline_options opt;
        opt.group = 0; opt.pairs_per_launch = form ? 2 : 1;
        OK(rvb_pipeline_create_lanes(&pipe, ctxs, 2, form ? two_lanes : one_lane, form ? 2 : 1, &opt));
        OK(rvb_pipeline_configure_speakers(pipe, speakers, 2, RVB_IR_ALL, 0, 1, 44100.0f, RVB_IR_EXACT, nrefl, AIR));
        job_geometry(0, mic, src, facing);
        CHECK(rvb_pipeline_submit_directed(pipe, mic, src, nullptr, nullptr, facing) == RVB_ERR_STATE);         // no pattern yet
        const float zero[3] = {0.0f, 0.0f, 0.0f}, inf[3] = {INFINITY, 0.0f, 0.0f};
        CHECK(rvb_pipeline_set_source_pattern(pipe, SHAPE, zero) == RVB_ERR_INVALID);
        CHECK(rvb_pipeline_set_source_pattern(pipe, SHAPE, inf) == RVB_ERR_INVALID);
        CHECK(rvb_pipeline_set_source_pattern(pipe, SHAPE, nullptr) == RVB_ERR_INVALID);
        OK(rvb_pipeline_set_source_pattern(pipe, SHAPE, default_facing));
        CHECK(rvb_pipeline_submit_directed(pipe, mic, src, nullptr, nullptr, zero) == RVB_ERR_INVALID);
        const std::vector<Got> got = run(pipe, NJOBS, 2 * 2 * opt.pairs_per_launch, true);
        CHECK((int) got.size() == NJOBS);
        for (int i = 0; i < (int) got.size(); ++i) {
            const Got & g = got[(size_t) i];
            CHECK(g.job == (uint64_t) i && g.nbins == want_bins[(size_t) i] && g.nimages == want_images[(size_t) i]);
            CHECK(same(g.hist, want[(size_t) i]));
        }
        // the default facing for a job without one; pending jobs forbid a change; off again: the trace without a pattern
        OK(rvb_pipeline_submit(pipe, mic, src));
        CHECK(rvb_pipeline_set_source_pattern(pipe, nullptr, nullptr) == RVB_ERR_STATE);
        rvb_pipeline_result res;
        OK(rvb_pipeline_next(pipe, &res));
        CHECK(std::vector<float>(res.histogram, res.histogram + res.nchannels * 8 * res.nbins) == want_default);
        OK(rvb_pipeline_set_source_pattern(pipe, nullptr, nullptr));
        OK(rvb_pipeline_submit(pipe, mic, src));
        OK(rvb_pipeline_next(pipe, &res));
        CHECK(std::vector<float>(res.histogram, res.histogram + res.nchannels * 8 * res.nbins) == want_plain);
        rvb_pipeline_destroy(pipe);
        std::printf("%s: %d directed jobs equal the step-by-step calls bit for bit\n", form ? "two lanes, two pairs per launch" : "one lane, one pair per launch", NJOBS);
    }

    // ---- rvb_set_source_pattern's own refusals ---------------------------------------------------------------------------------------
    {
        job_geometry(1, mic, src, facing);
        rvb_source_pattern bad = pattern_of(facing);
        bad.shape[3] = NAN;
        CHECK(rvb_set_source_pattern(solo, &bad, 1) == RVB_ERR_INVALID);
        bad = pattern_of(facing);
        bad.direction[0] = bad.direction[1] = bad.direction[2] = 0.0f;
        CHECK(rvb_set_source_pattern(solo, &bad, 1) == RVB_ERR_INVALID);
        const rvb_source_pattern two[2] = {pattern_of(facing), pattern_of(default_facing)};
        OK(rvb_set_source_pattern(solo, two, 2));
        CHECK(rvb_trace(solo, mic, src, nrefl, AIR, 0) == RVB_ERR_INVALID);       // rvb_trace takes one pattern only
        OK(rvb_set_source_pattern(solo, nullptr, 0));
    }

    // ---- the C++ mirror: Raytracer::setSourcePattern through getAllRaw against the C-ABI's records --------------------------------------
    {
        job_geometry(3, mic, src, facing);
        const rvb_source_pattern p = pattern_of(facing);
        OK(rvb_set_source_pattern(solo, &p, 1));
        // (the mirror's raytrace() takes the air coefficients as the reference writes them, rayverb.cpp:632-641: a double product rounded once)
        const float air[8] = {(float) (0.001 * -0.1), (float) (0.001 * -0.2), (float) (0.001 * -0.5), (float) (0.001 * -1.1),
                              (float) (0.001 * -2.7), (float) (0.001 * -9.4), (float) (0.001 * -29.0), (float) (0.001 * -60.0)};
        OK(rvb_trace(solo, mic, src, nrefl, air, 0));
        std::vector<rvb_impulse> want_raw((size_t) (nrays * nrefl));
        OK(rvb_get_diffuse(solo, want_raw.data()));
        uint64_t ncand = 0, nimg = 0;
        OK(rvb_get_image_candidates(solo, nullptr, 0, &ncand));
        std::vector<rvb_image_candidate> cand(ncand);
        if (ncand) OK(rvb_get_image_candidates(solo, cand.data(), ncand, &ncand));
        rvb_impulse direct;
        OK(rvb_get_direct(solo, &direct));
        OK(rvb_merge_images(cand.data(), ncand, &direct, 0, nullptr, 0, &nimg));
        want_raw.resize((size_t) (nrays * nrefl + nimg));
        if (nimg) OK(rvb_merge_images(cand.data(), ncand, &direct, 0, want_raw.data() + nrays * nrefl, nimg, &nimg));
        OK(rvb_set_source_pattern(solo, nullptr, 0));

        static_assert(sizeof(Triangle) == sizeof(rvb_triangle) && sizeof(cl_float3) == sizeof(rvb_float3) && sizeof(Surface) == sizeof(rvb_surface) &&
                      sizeof(Impulse) == sizeof(rvb_impulse), "the mirror's PODs are the C-ABI's");
        std::vector<Triangle> tris(scene.tris.size());
        std::vector<cl_float3> verts(scene.verts.size()), rays(dirs.size());
        std::vector<Surface> surfaces(scene.surfaces.size());
        std::memcpy(tris.data(), scene.tris.data(), tris.size() * sizeof(Triangle));
        std::memcpy(verts.data(), scene.verts.data(), verts.size() * sizeof(cl_float3));
        std::memcpy(surfaces.data(), scene.surfaces.data(), surfaces.size() * sizeof(Surface));
        std::memcpy(rays.data(), dirs.data(), rays.size() * sizeof(cl_float3));
        cl_float3 m, s, f;
        for (int k = 0; k < 3; ++k) { m.s[k] = mic[k]; s.s[k] = src[k]; f.s[k] = facing[k]; }
        m.s[3] = s.s[3] = f.s[3] = 0.0f;
        std::array<float, 8> shape;
        for (int b = 0; b < 8; ++b) shape[(size_t) b] = SHAPE[b];
        Raytracer tracer(nrefl, tris, verts, surfaces, false);
        tracer.setSourcePattern(f, shape);
        tracer.raytrace(m, s, rays, false);
        const std::vector<Impulse> scaled = tracer.getAllRaw(false).impulses;
        CHECK(scaled.size() == want_raw.size() && std::memcmp(scaled.data(), want_raw.data(), scaled.size() * sizeof(Impulse)) == 0);
        tracer.clearSourcePattern();
        tracer.raytrace(m, s, rays, false);
        const std::vector<Impulse> plain = tracer.getAllRaw(false).impulses;
        CHECK(plain.size() == scaled.size() && std::memcmp(plain.data(), scaled.data(), plain.size() * sizeof(Impulse)) != 0);
        std::printf("Raytracer::setSourcePattern: getAllRaw equals the C-ABI's scaled records\n");
    }

    for (int i = 0; i < 3; ++i) rvb_destroy(ctxs[i]);
    if (failures) { std::printf("%d check(s) failed\n", failures); return 1; }
    std::printf("all source pattern pipeline checks passed\n");
    return 0;
}
