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

#include "pipeline_rig.h"

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
    return solo_ir(ctx, mic, src, nrefl, sp, nsp, nullptr, nullptr, nullptr, RVB_IR_EXACT, nbins_out, nimages_out);
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
