// pipeline_rig.h — what the C++ callers of the pipeline share (test_pipeline.cpp, test_pipeline_lanes.cpp, test_pipeline_source.cpp):
// the check macros, the hall scene, the ray directions, the air coefficients and the step-by-step reference impulse response.
// Include it after rvb_capi.h, once per program.
#pragma once

#include <cmath>
#include <cstdio>
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

// the same impulse response by the step-by-step calls on one context
static std::vector<float> solo_ir(rvb_ctx * ctx, const float mic[3], const float src[3], uint64_t nrefl, const rvb_speaker * sp, uint64_t nsp,
                                  const float * table, const float * facing, const float * up, int mode, uint64_t * nbins_out, uint64_t * nimages_out)
{
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
    if (table) OK(rvb_ir_configure_hrtf(ctx, mic, table, facing, up, RVB_IR_ALL, images.data(), nimg));
    else OK(rvb_ir_configure_speakers(ctx, mic, sp, nsp, RVB_IR_ALL, images.data(), nimg));
    uint64_t nbins = 0;
    OK(rvb_ir_download(ctx, 1, 44100.0f, mode, nullptr, 0, &nbins));
    const uint64_t nch = table ? 2 : nsp;
    std::vector<float> out((size_t) (nch * 8 * nbins));
    OK(rvb_ir_download(ctx, 1, 44100.0f, mode, out.data(), nbins, &nbins));
    *nbins_out = nbins;
    *nimages_out = nimg;
    return out;
}
