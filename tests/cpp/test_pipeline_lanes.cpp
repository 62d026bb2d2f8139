// test_pipeline_lanes.cpp — a C++11 caller of the pipeline over lanes with several pairs per launch (rvb_pipeline_create_lanes,
// csrc/pipeline.hip), on rvb_capi.h alone: what a caller with many (source, listener) pairs of one hall does on a node (BASELINE
// config C5).  Sixteen HRTF jobs with a facing of their own go through two lanes of two contexts (all on device 0) with four pairs per
// launch, ten speaker jobs through one lane of three contexts with three pairs per launch (an incomplete last unit); every result must
// equal, bit for bit, the same impulse response generated on a fifth context with the step-by-step calls (rvb_trace -> rvb_merge_images
// -> rvb_ir_configure_* -> rvb_ir_download, exact mode).  Then the refusals, the pending limit and a failing lane.
// Exit code 0 = all passed; 2 = no GPU.
#include "rvb_capi.h"

#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "pipeline_rig.h"

static void job_geometry(int i, float mic[3], float src[3], float facing[3])
{
    mic[0] = -9.0f + 0.9f * i; mic[1] = 1.5f + 0.05f * (i % 5); mic[2] = -4.0f + 0.35f * i;
    src[0] = 8.0f - 0.7f * i; src[1] = 1.7f + 0.1f * (i % 3); src[2] = -5.0f + 0.3f * ((i * 7) % 20);
    const float d[3] = {src[0] - mic[0], 0.0f, src[2] - mic[2]};
    const float l = std::sqrt(d[0] * d[0] + d[2] * d[2]);
    facing[0] = d[0] / l; facing[1] = 0.0f; facing[2] = d[2] / l;
}

struct Got {
    std::vector<float> hist;
    uint64_t job, nchannels, nbins, nimages;
};

// all jobs through the pipeline, as many pending as it takes; HRTF jobs with their own facing
static std::vector<Got> run(rvb_pipeline * pipe, int njobs, uint64_t limit, bool hrtf)
{
    std::vector<Got> got;
    float mic[3], src[3], facing[3];
    const float up[3] = {0.0f, 1.0f, 0.0f};
    int sent = 0;
    while ((int) got.size() < njobs) {
        while (sent < njobs && rvb_pipeline_pending(pipe) < limit) {
            job_geometry(sent, mic, src, facing);
            if (hrtf) OK(rvb_pipeline_submit_oriented(pipe, mic, src, facing, up));
            else OK(rvb_pipeline_submit(pipe, mic, src));
            ++sent;
        }
        rvb_pipeline_result res;
        const int rc = rvb_pipeline_next(pipe, &res);
        OK(rc);
        if (rc != RVB_OK) break;
        Got g;
        g.hist.assign(res.histogram, res.histogram + res.nchannels * 8 * res.nbins);
        g.job = res.job; g.nchannels = res.nchannels; g.nbins = res.nbins; g.nimages = res.nimages;
        got.push_back(g);
    }
    return got;
}

static void check_against_solo(rvb_ctx * solo, const std::vector<Got> & got, int njobs, uint64_t nrefl, const rvb_speaker * sp, uint64_t nsp,
                               const float * table)
{
    CHECK((int) got.size() == njobs);
    float mic[3], src[3], facing[3];
    const float up[3] = {0.0f, 1.0f, 0.0f};
    for (int i = 0; i < (int) got.size(); ++i) {
        job_geometry(i, mic, src, facing);
        uint64_t nbins = 0, nimg = 0;
        const std::vector<float> want = solo_ir(solo, mic, src, nrefl, sp, nsp, table, facing, up, RVB_IR_EXACT, &nbins, &nimg);
        const Got & g = got[(size_t) i];
        CHECK(g.job == (uint64_t) i && g.nbins == nbins && g.nimages == nimg && g.nchannels == (table ? 2u : nsp));
        CHECK(want.size() == g.hist.size() && std::memcmp(want.data(), g.hist.data(), want.size() * sizeof(float)) == 0);
        bool any = false;
        for (float v : want) any = any || v != 0.0f;
        CHECK(any);
    }
}

int main()
{
    const uint64_t nrays = 20000, nrefl = 32;
    Scene scene;
    const std::vector<rvb_float3> dirs = directions(nrays, 3);
    const int NCTX = 4;
    rvb_ctx * ctxs[NCTX + 2] = {nullptr, nullptr, nullptr, nullptr, nullptr, nullptr};
    for (int i = 0; i < NCTX + 2; ++i) {
        const int rc = rvb_create(&ctxs[i], 0, 0);
        if (rc != RVB_OK) { std::printf("rvb_create: %s\n", rvb_last_error(nullptr)); return 2; }      // no GPU: there is no CPU path
        // the lane contexts 1-3 read context 0's scene (rvb_share_scene); the solo context builds its own; the last one has none
        if (i == 0 || i == NCTX) OK(rvb_set_scene(ctxs[i], scene.tris.data(), scene.tris.size(), scene.verts.data(), scene.verts.size(), scene.surfaces.data(), scene.surfaces.size()));
        else if (i < NCTX) OK(rvb_share_scene(ctxs[i], ctxs[0]));
        OK(rvb_set_directions(ctxs[i], dirs.data(), dirs.size()));
    }
    rvb_ctx * solo = ctxs[NCTX];
    rvb_ctx * sceneless = ctxs[NCTX + 1];
    rvb_speaker speakers[2];
    std::memset(speakers, 0, sizeof(speakers));
    speakers[0].direction[0] = -1.0f; speakers[0].direction[2] = -1.0f; speakers[0].coefficient = 0.5f;
    speakers[1].direction[0] = 1.0f; speakers[1].direction[2] = -1.0f; speakers[1].coefficient = 0.5f;
    std::vector<float> table((size_t) 2 * 360 * 180 * 8);
    for (int e = 0; e < 2; ++e)
        for (int a = 0; a < 360; ++a)
            for (int el = 0; el < 180; ++el)
                for (int b = 0; b < 8; ++b)
                    table[(((size_t) e * 360 + a) * 180 + el) * 8 + b] = 0.35f + 0.25f * std::cos(0.017453292f * (a - (e ? 90 : 270))) * std::sin(0.017453292f * el) + 0.02f * b;
    const float facing0[3] = {0.0f, 0.0f, 1.0f}, up[3] = {0.0f, 1.0f, 0.0f};

    // ---- HRTF, a facing per job: two lanes of two contexts, four pairs per launch -------------------------------------------------
    {
        rvb_pipeline * pipe = nullptr;
        const uint64_t sizes[2] = {2, 2};
        rvb_pipeline_options opt;
        opt.group = 0; opt.pairs_per_launch = 4;
        OK(rvb_pipeline_create_lanes(&pipe, ctxs, 4, sizes, 2, &opt));
        OK(rvb_pipeline_configure_hrtf(pipe, table.data(), facing0, up, RVB_IR_ALL, 0, 1, 44100.0f, RVB_IR_EXACT, nrefl, AIR));
        const std::vector<Got> got = run(pipe, 16, 2 * 4 * 4, true);
        rvb_pipeline_destroy(pipe);
        check_against_solo(solo, got, 16, nrefl, nullptr, 0, table.data());
        std::printf("hrtf: 16 jobs through lanes [2, 2] with 4 pairs per launch equal the step-by-step calls bit for bit\n");
    }

    // ---- speakers: one lane of three contexts, three pairs per launch (ten jobs: the last unit is incomplete) --------------------
    {
        rvb_pipeline * pipe = nullptr;
        const uint64_t sizes[1] = {3};
        rvb_pipeline_options opt;
        opt.group = 0; opt.pairs_per_launch = 3;
        OK(rvb_pipeline_create_lanes(&pipe, ctxs, 3, sizes, 1, &opt));
        OK(rvb_pipeline_configure_speakers(pipe, speakers, 2, RVB_IR_ALL, 0, 1, 44100.0f, RVB_IR_EXACT, nrefl, AIR));
        const std::vector<Got> got = run(pipe, 10, 2 * 3 * 3, false);
        rvb_pipeline_destroy(pipe);
        check_against_solo(solo, got, 10, nrefl, speakers, 2, nullptr);
        std::printf("speakers: 10 jobs through lane [3] with 3 pairs per launch equal the step-by-step calls bit for bit\n");
    }

    // ---- refusals ------------------------------------------------------------------------------------------------------------------
    {
        rvb_pipeline * pipe = nullptr;
        rvb_pipeline_options opt;
        opt.group = 0; opt.pairs_per_launch = 2;
        rvb_ctx * twice[4] = {ctxs[0], ctxs[1], ctxs[1], ctxs[2]};
        const uint64_t two_two[2] = {2, 2}, two_one[2] = {2, 1}, two_three[2] = {2, 3};
        CHECK(rvb_pipeline_create_lanes(&pipe, twice, 4, two_two, 2, &opt) == RVB_ERR_INVALID && pipe == nullptr);     // a context twice
        CHECK(rvb_pipeline_create_lanes(&pipe, ctxs, 4, two_one, 2, &opt) == RVB_ERR_INVALID);                         // sizes do not add up
        CHECK(rvb_pipeline_create_lanes(&pipe, ctxs, 4, two_three, 2, &opt) == RVB_ERR_INVALID);
        opt.pairs_per_launch = 0;
        CHECK(rvb_pipeline_create_lanes(&pipe, ctxs, 4, two_two, 2, &opt) == RVB_ERR_INVALID);
        opt.pairs_per_launch = RVB_PIPELINE_MAX_PAIRS + 1;
        CHECK(rvb_pipeline_create_lanes(&pipe, ctxs, 4, two_two, 2, &opt) == RVB_ERR_INVALID);
        opt.pairs_per_launch = 2; opt.group = 2;                                                                        // no groups of pairs
        CHECK(rvb_pipeline_create_lanes(&pipe, ctxs, 4, two_two, 2, &opt) == RVB_ERR_INVALID);
        CHECK(pipe == nullptr);
        std::printf("refusals: a context twice, lane sizes, pairs per launch 0 and above the maximum, group > 1 with pairs\n");
    }

    // ---- the pending limit (2 x contexts x pairs per launch), then a failing lane -----------------------------------------------------
    {
        rvb_pipeline * pipe = nullptr;
        const uint64_t sizes[2] = {1, 1};
        OK(rvb_pipeline_create_lanes(&pipe, ctxs, 2, sizes, 2, nullptr));       // NULL options: one trace per job
        float mic[3], src[3], facing[3];
        CHECK(rvb_pipeline_submit(pipe, mic, src) == RVB_ERR_STATE);          // not configured yet
        OK(rvb_pipeline_configure_speakers(pipe, speakers, 2, RVB_IR_ALL, 0, 1, 44100.0f, RVB_IR_EXACT, nrefl, AIR));
        rvb_pipeline_result res;
        CHECK(rvb_pipeline_next(pipe, &res) == RVB_ERR_STATE);                // nothing pending
        job_geometry(0, mic, src, facing);
        for (int i = 0; i < 4; ++i) OK(rvb_pipeline_submit(pipe, mic, src));
        CHECK(rvb_pipeline_submit(pipe, mic, src) == RVB_ERR_CAPACITY);
        std::vector<float> first;
        for (int i = 0; i < 4; ++i) {
            OK(rvb_pipeline_next(pipe, &res));
            CHECK(res.job == (uint64_t) i);
            if (i == 0) first.assign(res.histogram, res.histogram + 16 * res.nbins);
            else CHECK(first.size() == 16 * res.nbins && std::memcmp(first.data(), res.histogram, first.size() * sizeof(float)) == 0);
        }
        OK(rvb_pipeline_submit(pipe, mic, src));                             // and afterwards
        OK(rvb_pipeline_next(pipe, &res));
        CHECK(res.job == 4 && first.size() == 16 * res.nbins && std::memcmp(first.data(), res.histogram, first.size() * sizeof(float)) == 0);
        rvb_pipeline_destroy(pipe);

        rvb_ctx * mixed[2] = {ctxs[0], sceneless};
        OK(rvb_pipeline_create_lanes(&pipe, mixed, 2, sizes, 2, nullptr));
        OK(rvb_pipeline_configure_speakers(pipe, speakers, 2, RVB_IR_ALL, 0, 1, 44100.0f, RVB_IR_EXACT, nrefl, AIR));
        for (int i = 0; i < 3; ++i) {
            job_geometry(i, mic, src, facing);
            OK(rvb_pipeline_submit(pipe, mic, src));
        }
        OK(rvb_pipeline_next(pipe, &res));                                    // job 0, lane 0: fine
        uint64_t nbins = 0, nimg = 0;
        job_geometry(0, mic, src, facing);
        const std::vector<float> want = solo_ir(solo, mic, src, nrefl, speakers, 2, nullptr, nullptr, nullptr, RVB_IR_EXACT, &nbins, &nimg);
        CHECK(res.job == 0 && res.nbins == nbins && std::memcmp(want.data(), res.histogram, want.size() * sizeof(float)) == 0);
        CHECK(rvb_pipeline_next(pipe, &res) == RVB_ERR_STATE);                // job 1, lane 1: no scene
        const std::string why = rvb_pipeline_last_error(pipe);
        CHECK(why.find("lane 1") != std::string::npos && why.find("trace") != std::string::npos);
        std::printf("failing lane: %s\n", why.c_str());
        OK(rvb_pipeline_next(pipe, &res));                                    // job 2, lane 0 again: fine
        job_geometry(2, mic, src, facing);
        const std::vector<float> want2 = solo_ir(solo, mic, src, nrefl, speakers, 2, nullptr, nullptr, nullptr, RVB_IR_EXACT, &nbins, &nimg);
        CHECK(res.job == 2 && res.nbins == nbins && std::memcmp(want2.data(), res.histogram, want2.size() * sizeof(float)) == 0);
        CHECK(rvb_pipeline_pending(pipe) == 0);
        rvb_pipeline_destroy(pipe);                                           // joins the lane threads after the failure
    }

    for (int i = 0; i < NCTX + 2; ++i) rvb_destroy(ctxs[i]);
    if (failures) { std::printf("%d check(s) failed\n", failures); return 1; }
    std::printf("all pipeline lane checks passed\n");
    return 0;
}
