// san_driver.cpp -- host sanitizer harness ("host ASan/UBSan on
// the oracle", TSan on the threaded BVH builder).  Built from the scene
// library's sources and the oracle with -fsanitize=... by tools/sanitize/
// Makefile, so the instrumented code runs in an instrumented executable (no
// preloading into Python).  Test infrastructure; not part of the product.
//
//   san_driver decode FILE...   every image decoder LoadTexture reaches
//                               (LoadImageFloat, LoadImageRGBA8): "ok W H" or
//                               "error: ..." per file; a crash or sanitizer
//                               report is the failure
//   san_driver model FILE...    LoadModelAsPrefab (OBJ/MTL + textures) + PackSceneData
//   san_driver scene FILE...    LoadScene + PackSceneData
//   san_driver render           configs C1-C5 packed; oracle Reset/Run(2)/Run(1)
//                               on small frames, resolve, preview
//   san_driver bvh FACES        random triangle soup through CreateMesh (the
//                               threaded builder, PT_BVH_THREADS) + PackSceneData
//   san_driver denoise          ptsDenoise on random small images: sizes below
//                               the 2 * step halo, every iteration count, an
//                               all-empty image, rejected arguments
//   san_driver stats            ptsFrameStatistics and the ptsStats* helpers on
//                               small random, empty and NaN / inf / denormal
//                               images, single and pair, one pixel included;
//                               rejected arguments
//   san_driver tile_stats       ptsTileStatistics on random, empty and NaN / inf /
//                               denormal images from 1x1 to 67x45, single and
//                               pair, thresholds 0 to +inf, against
//                               ptsFrameStatistics' totals; rejected arguments
//   san_driver reproject_moving ptsShapeMotion and ptsReprojectMoving on random
//                               tables with NaN and flagged records, 1x1 to 67x45
//   san_driver reproject        ptsReproject and ptsCentralCameraRay on random
//                               small frames (1x1 and differing previous and
//                               current sizes included) under cameras of every
//                               model that project inside, far outside, behind
//                               and to non-finite positions, with random,
//                               empty and NaN / inf histories; rejected arguments
//   san_driver rectify          ptsRectifyHistory on random, all-empty and NaN /
//                               inf / denormal images from 1x1 to 67x45, every
//                               Radius, MinNeighbours 1 and 49, Sigma 0,
//                               ClampedHistory +inf, in place and out of
//                               place; rejected arguments
//   san_driver despike          ptsDespike on random, all-empty and NaN / inf /
//                               denormal images from 1x1 to 67x45, every Radius
//                               and Rank, MinNeighbours from Rank to every
//                               neighbour, Scale 0, Floor > 0; rejected arguments
//   san_driver guides           include/pt_guides.h's classification and bounce
//                               functions: every material type, roughness on
//                               both sides of the bound and NaN, bounce counts
//                               up to and past the cap; unit, grazing (c = 0
//                               included), zero, NaN, infinite and denormal
//                               vectors; indices 1, below 1, 0, negative, NaN
//                               and infinite; the restart's packed round trip
#include "../../path-tracer_amd/csrc/scene/scene.hpp"
#include "../../path-tracer_amd/csrc/scene/configs.hpp"
#include "../../path-tracer_amd/csrc/scene/image.hpp"
#include "../../oracle/pt_oracle.h"
#include "../../include/pt_scene.h"
#include "../../include/pt_guides.h"

#include <cmath>
#include <cstdio>
#include <cstring>
#include <random>
#include <string>
#include <vector>

using namespace pth;

static int Decode(int argc, char** argv)
{
    for (int i = 0; i < argc; i++) {
        int w = 0, h = 0;
        std::vector<uint8_t> rgba;
        std::string e1;
        FILE* fp = std::fopen(argv[i], "rb");
        char magic[2] = {0, 0};
        if (fp) { (void)!std::fread(magic, 1, 2, fp); std::fclose(fp); }
        if (magic[0] == '#' && magic[1] == '?') {   // Radiance HDR: the float path only
            std::vector<vec4> px;
            if (LoadImageFloat(argv[i], w, h, px, e1)) std::printf("%s: ok %d %d\n", argv[i], w, h);
            else std::printf("%s: error: %s\n", argv[i], e1.c_str());
            continue;
        }
        if (!LoadImageRGBA8(argv[i], w, h, rgba, e1)) {
            std::printf("%s: error: %s\n", argv[i], e1.c_str());
            continue;
        }
        std::printf("%s: ok %d %d\n", argv[i], w, h);
        // LoadTexture's float path (16 B/px) only for images of sane size:
        // the crafted huge-but-legal headers of the corpus would otherwise
        // allocate gigabytes under ASan.
        if ((uint64_t)w * (uint64_t)h <= (16u << 20)) {
            std::vector<vec4> px;
            std::string e2;
            int w2 = 0, h2 = 0;
            if (!LoadImageFloat(argv[i], w2, h2, px, e2) || w2 != w || h2 != h)
                std::printf("%s: float path disagrees: %s\n", argv[i], e2.c_str());
        }
    }
    return 0;
}

static int Model(int argc, char** argv)
{
    for (int i = 0; i < argc; i++) {
        scene* s = CreateScene();
        load_model_options opt;
        std::string err;
        prefab* p = LoadModelAsPrefab(s, argv[i], &opt, &err);
        if (p) {
            CreateEntity(s, p, nullptr);
            PackSceneData(s);
            std::printf("%s: ok\n", argv[i]);
        } else {
            std::printf("%s: error: %s\n", argv[i], err.c_str());
        }
        DestroyScene(s);
    }
    return 0;
}

static int Scene(int argc, char** argv)
{
    for (int i = 0; i < argc; i++) {
        std::string err;
        scene* s = LoadScene(argv[i], &err);
        if (s) {
            PackSceneData(s);
            std::printf("%s: ok\n", argv[i]);
            DestroyScene(s);
        } else {
            std::printf("%s: error: %s\n", argv[i], err.c_str());
        }
    }
    return 0;
}

static int Render()
{
    for (int c = 1; c <= 5; c++) {
        config_info info{};
        scene* s = CreateConfigScene(c, &info);
        if (!s) { std::printf("C%d: no scene\n", c); return 1; }
        pt_scene_packs packs{};
        GetScenePacks(s, &packs);
        const uint32_t W = 48, H = 40;
        for (uint32_t nranks : {1u, 2u}) {
            oracle_renderer* o = oracle_create(&packs, W, H, 0, nranks, 4);
            pt_basic_renderer_params* P = oracle_params(o);
            P->RenderFlags = 3;
            P->CameraIndex = c == 5 ? 1 : 0;
            oracle_reset(o);
            oracle_run(o, 2);
            oracle_run(o, 1);
            std::vector<float> acc(4 * W * H);
            oracle_read_accum(o, acc.data());
            std::vector<pt_pixel_state> st(W * H);
            oracle_read_state(o, st.data());
            std::vector<float> out(4 * W * H);
            std::vector<uint8_t> out8(4 * W * H);
            pt_resolve_parameters rp{1.0f, 3, 1.0f};
            oracle_resolve(acc.data(), W * H, &rp, out.data(), out8.data());
            uint64_t rays = 0, samples = 0;
            oracle_counters(o, &rays, &samples);
            std::printf("C%d nranks %u: rays %llu samples %llu\n", c, nranks, (unsigned long long)rays,
                        (unsigned long long)samples);
            oracle_destroy(o);
        }
        pt_preview_parameters pp{};
        std::memcpy(&pp.CameraTransform, &packs.cameras[0].Transform, sizeof(pp.CameraTransform));
        pp.RenderMode = 1; pp.Brightness = 1; pp.SelectedShapeIndex = 0xFFFFFFFFu;
        pp.RenderSizeX = 32; pp.RenderSizeY = 24; pp.MouseX = 3; pp.MouseY = 4;
        std::vector<float> img(4 * 32 * 24);
        std::vector<pt_preview_aov> aov(32 * 24);
        uint32_t q = 0;
        oracle_preview(&packs, &pp, img.data(), aov.data(), &q);
        DestroyScene(s);
    }
    return 0;
}

static int Bvh(uint32_t faces)
{
    std::mt19937 rng(7);
    std::uniform_real_distribution<float> u(-10.0f, 10.0f), d(-0.3f, 0.3f);
    std::vector<float> pos(9 * (size_t)faces);
    std::vector<uint32_t> idx(3 * (size_t)faces);
    for (uint32_t f = 0; f < faces; f++) {
        float cx = u(rng), cy = u(rng), cz = u(rng);
        for (int k = 0; k < 3; k++) {
            pos[9 * (size_t)f + 3 * k + 0] = cx + d(rng);
            pos[9 * (size_t)f + 3 * k + 1] = cy + d(rng);
            pos[9 * (size_t)f + 3 * k + 2] = cz + d(rng);
            idx[3 * (size_t)f + k] = 3 * f + k;
        }
    }
    scene* s = CreateScene();
    mesh* m = CreateMesh(s, "soup", 3 * faces, pos.data(), nullptr, nullptr, faces, idx.data());
    entity* e = CreateEntity(s, ENTITY_TYPE_MESH_INSTANCE, nullptr);
    e->Mesh = m;
    PackSceneData(s);
    std::printf("bvh: %u faces, %zu nodes, depth %u\n", faces, m->Nodes.size(), m->Depth);
    DestroyScene(s);
    return 0;
}

static int Denoise()
{
    std::mt19937 rng(11);
    std::uniform_real_distribution<float> u(0.0f, 4.0f), s(-1.0f, 1.0f);
    const uint32_t sizes[][2] = {{1, 1}, {1, 7}, {3, 2}, {5, 5}, {16, 16}, {17, 33}, {40, 24}, {67, 45}};
    for (auto& wh : sizes) {
        const uint32_t W = wh[0], H = wh[1];
        const size_t n = (size_t)W * H;
        for (int empty = 0; empty < 2; empty++) {
            std::vector<float> acc(4 * n), out(4 * n, -1.0f);
            std::vector<pt_denoise_guide> g(n);
            for (size_t i = 0; i < n; i++) {
                for (int k = 0; k < 3; k++) acc[4 * i + k] = u(rng);
                acc[4 * i + 3] = empty ? 0.0f : (float)(rng() % 5);   // some pixels empty
                for (int k = 0; k < 3; k++) { g[i].normal[k] = s(rng); g[i].albedo[k] = 0.5f * u(rng); }
                g[i].time = 1.0f + u(rng);
                g[i].shape = rng() % 4 == 0 ? 0xFFFFFFFFu : rng() % 3;
            }
            for (uint32_t it = 0; it <= 8; it++) {
                pt_denoise_parameters p{it, 1.0f, 0.5f, 0.5f, 0.5f};
                if (ptsDenoise(W, H, acc.data(), g.data(), &p, out.data()) != 0) { std::printf("denoise: failed\n"); return 1; }
                size_t filled = 0;
                for (size_t i = 0; i < n; i++) filled += out[4 * i + 3] == 1.0f;
                std::printf("denoise %ux%u empty %d iterations %u: %zu of %zu pixels\n", W, H, empty, it, filled, n);
            }
        }
    }
    // rejected arguments leave `out` untouched
    float acc[4] = {1, 1, 1, 1}, out[4] = {7, 7, 7, 7};
    pt_denoise_guide g{};
    pt_denoise_parameters ok{5, 1, 1, 1, 1}, many{9, 1, 1, 1, 1}, zero{5, 1, 0, 1, 1};
    int bad = 0;
    bad += ptsDenoise(1, 1, nullptr, &g, &ok, out) == 0;
    bad += ptsDenoise(1, 1, acc, nullptr, &ok, out) == 0;
    bad += ptsDenoise(1, 1, acc, &g, nullptr, out) == 0;
    bad += ptsDenoise(1, 1, acc, &g, &ok, nullptr) == 0;
    bad += ptsDenoise(1, 1, acc, &g, &many, out) == 0;
    bad += ptsDenoise(1, 1, acc, &g, &zero, out) == 0;
    bad += ptsDenoise(0, 1, acc, &g, &ok, out) == 0;
    for (float v : out) bad += v != 7.0f;
    std::printf("denoise: %d argument checks wrong\n", bad);
    return bad != 0;
}

static int Stats()
{
    std::mt19937 rng(12);
    std::uniform_real_distribution<float> u(0.0f, 4.0f);
    const float nan = std::nanf(""), inf = HUGE_VALF;
    const float odd[] = {0.0f, -0.0f, -1.0f, nan, inf, -inf, 1e-45f, 1e-38f, 3e38f, 1.0f, 4294967296.0f, 2.3283064e-10f};
    const uint32_t sizes[][2] = {{1, 1}, {1, 7}, {3, 2}, {16, 16}, {17, 33}, {40, 24}, {67, 45}};
    int bad = 0;
    for (auto& wh : sizes) {
        const uint32_t W = wh[0], H = wh[1];
        const size_t n = (size_t)W * H;
        // kind 0: random; 1: all empty; 2: every component drawn from the odd values (NaN, inf, denormals ...)
        for (int kind = 0; kind < 3; kind++) {
            std::vector<float> a(4 * n), b(4 * n);
            for (std::vector<float>* v : {&a, &b}) {
                for (size_t i = 0; i < 4 * n; i++) {
                    if (kind == 0) (*v)[i] = i % 4 == 3 ? (float)(rng() % 5) : u(rng);
                    else if (kind == 1) (*v)[i] = 0.0f;
                    else (*v)[i] = odd[rng() % (sizeof(odd) / sizeof(odd[0]))];
                }
            }
            for (int pair = 0; pair < 2; pair++) {
                pt_frame_statistics s;
                if (ptsFrameStatistics(W, H, a.data(), pair ? b.data() : nullptr, &s) != 0) { std::printf("stats: failed\n"); return 1; }
                uint64_t lum = 0, noise = 0;
                for (int k = 0; k < PT_STATS_BINS; k++) { lum += s.luminance_histogram[k]; noise += s.noise_histogram[k]; }
                bad += s.pixels != n || s.filled + s.empty + s.nonfinite != n || lum + s.dark != s.filled ||
                       noise != s.noise_pixels || (!pair && (s.noise_pixels || s.noise_skipped));
                std::printf("stats %ux%u kind %d pair %d: filled %llu empty %llu nonfinite %llu dark %llu noise %llu + %llu, "
                            "brightness %g noise %g\n", W, H, kind, pair, (unsigned long long)s.filled,
                            (unsigned long long)s.empty, (unsigned long long)s.nonfinite, (unsigned long long)s.dark,
                            (unsigned long long)s.noise_pixels, (unsigned long long)s.noise_skipped,
                            ptsStatsAutoBrightness(&s, 0.18, 0.01, 0.99), ptsStatsNoise(&s, 0.95));
                for (double q : {1e-12, 0.5, 1.0}) {
                    const int p = ptsStatsPercentileBin(s.luminance_histogram, q);
                    bad += p < -1 || p > 255 || (lum == 0) != (p == -1);
                    (void)ptsStatsLogAverage(s.luminance_histogram, q, 1.0);
                }
            }
        }
    }
    // rejected arguments leave `out` untouched
    float acc[4] = {1, 1, 1, 1};
    pt_frame_statistics out;
    std::memset(&out, 0x55, sizeof(out));
    const pt_frame_statistics before = out;
    bad += ptsFrameStatistics(1, 1, nullptr, nullptr, &out) == 0;
    bad += ptsFrameStatistics(1, 1, acc, nullptr, nullptr) == 0;
    bad += ptsFrameStatistics(0, 1, acc, nullptr, &out) == 0;
    bad += ptsFrameStatistics(1, 0, acc, nullptr, &out) == 0;
    bad += ptsFrameStatistics(1, 1, acc, acc, &out) == 0;
    bad += std::memcmp(&out, &before, sizeof(out)) != 0;
    bad += ptsStatsPercentileBin(nullptr, 0.5) != -1 || ptsStatsBinEdge(-1) != 0.0 || ptsStatsBinEdge(257) != 0.0;
    for (float v : odd) bad += ptsStatsBin(v) < 0 || ptsStatsBin(v) > 255;
    std::printf("stats: %d checks wrong\n", bad);
    return bad != 0;
}

// ptsTileStatistics: the records lie in an array of
// exactly tiles_x * tiles_y elements, so a write past the last tile is ASan's.
static int TileStats()
{
    std::mt19937 rng(15);
    std::uniform_real_distribution<float> u(0.0f, 4.0f);
    const float nan = std::nanf(""), inf = HUGE_VALF;
    const float odd[] = {0.0f, -0.0f, -1.0f, nan, inf, -inf, 1e-45f, 1e-38f, 3e38f, 1.0f, 4294967296.0f, 2.3283064e-10f};
    const uint32_t sizes[][2] = {{1, 1}, {1, 7}, {3, 2}, {15, 15}, {16, 16}, {17, 16}, {16, 17}, {17, 33}, {33, 31},
                                 {40, 24}, {67, 45}};
    const float thresholds[] = {0.0f, 0.1f, 1.0f, inf};
    int bad = 0;
    for (auto& wh : sizes) {
        const uint32_t W = wh[0], H = wh[1];
        const size_t n = (size_t)W * H, tiles = (size_t)((W + 15) / 16) * ((H + 15) / 16);
        // kind 0: random; 1: all empty; 2: every component drawn from the odd values (NaN, inf, denormals ...)
        for (int kind = 0; kind < 3; kind++) {
            std::vector<float> a(4 * n), b(4 * n);
            for (std::vector<float>* v : {&a, &b}) {
                for (size_t i = 0; i < 4 * n; i++) {
                    if (kind == 0) (*v)[i] = i % 4 == 3 ? (float)(rng() % 5) : u(rng);
                    else if (kind == 1) (*v)[i] = 0.0f;
                    else (*v)[i] = odd[rng() % (sizeof(odd) / sizeof(odd[0]))];
                }
            }
            for (int pair = 0; pair < 2; pair++) {
                pt_frame_statistics f;
                if (ptsFrameStatistics(W, H, a.data(), pair ? b.data() : nullptr, &f) != 0) { std::printf("tile_stats: failed\n"); return 1; }
                uint64_t over_before = ~0ull;
                for (float t : thresholds) {
                    std::vector<pt_tile_statistics> s(tiles);
                    if (ptsTileStatistics(W, H, a.data(), pair ? b.data() : nullptr, t, s.data()) != 0) { std::printf("tile_stats: failed\n"); return 1; }
                    uint64_t filled = 0, empty = 0, nonfinite = 0, pairs = 0, over = 0;
                    for (const pt_tile_statistics& r : s) {
                        filled += r.filled; empty += r.empty; nonfinite += r.nonfinite; pairs += r.pair; over += r.over;
                        bad += r.over > r.pair || r.reserved != 0 || r.filled + r.empty + r.nonfinite > 256;
                        bad += r.filled ? !(r.min_count > 0.0f && r.min_count <= r.max_count) : (r.min_count != 0.0f || r.max_count != 0.0f);
                    }
                    bad += filled != f.filled || empty != f.empty || nonfinite != f.nonfinite || pairs != f.noise_pixels;
                    bad += over > over_before || (t == inf && over != 0) || (!pair && pairs != 0);
                    over_before = over;
                    std::printf("tile_stats %ux%u kind %d pair %d threshold %g: %zu tiles, filled %llu empty %llu nonfinite %llu "
                                "pair %llu over %llu\n", W, H, kind, pair, (double)t, tiles, (unsigned long long)filled,
                                (unsigned long long)empty, (unsigned long long)nonfinite, (unsigned long long)pairs,
                                (unsigned long long)over);
                }
            }
        }
    }
    // rejected arguments leave `out` untouched
    float acc[4] = {1, 1, 1, 1}, other[4] = {1, 2, 1, 1};
    pt_tile_statistics out;
    std::memset(&out, 0x55, sizeof(out));
    const pt_tile_statistics before = out;
    bad += ptsTileStatistics(1, 1, nullptr, nullptr, 0.1f, &out) == 0;
    bad += ptsTileStatistics(1, 1, acc, nullptr, 0.1f, nullptr) == 0;
    bad += ptsTileStatistics(0, 1, acc, nullptr, 0.1f, &out) == 0;
    bad += ptsTileStatistics(1, 0, acc, nullptr, 0.1f, &out) == 0;
    bad += ptsTileStatistics(1, 1, acc, acc, 0.1f, &out) == 0;
    bad += ptsTileStatistics(1, 1, acc, other, nan, &out) == 0;
    bad += ptsTileStatistics(1, 1, acc, other, -0.5f, &out) == 0;
    bad += ptsTileStatistics(1, 1, acc, other, -inf, &out) == 0;
    bad += std::memcmp(&out, &before, sizeof(out)) != 0;
    bad += ptsTileStatistics(1, 1, acc, other, -0.0f, &out) != 0 || out.pair != 1 || out.over != 1;
    std::printf("tile_stats: %d checks wrong\n", bad);
    return bad != 0;
}

// A camera record at `pos`, turned by `yaw` about z from the configs' forward
// direction (+y); To = T R, From = R^-1 T^-1, column-major.
static pt_packed_camera SanCamera(uint32_t model, const float pos[3], float yaw)
{
    pt_packed_camera c{};
    c.Model = model;
    c.FocalLength = 0.05f;
    c.SensorDistance = 0.0508f;
    c.SensorSize[0] = 0.032f;
    c.SensorSize[1] = 0.016f;
    const float cs = std::cos(yaw), sn = std::sin(yaw);
    // camera axes in the world: x' = (cs, sn, 0), y' = (0, 0, 1), z' = x' cross y' (the camera looks along -z')
    const float X[3] = {cs, sn, 0.0f}, Y[3] = {0.0f, 0.0f, 1.0f}, Z[3] = {sn, -cs, 0.0f};
    float* To = c.Transform.To;
    float* From = c.Transform.From;
    for (int r = 0; r < 3; r++) {
        To[0 + r] = X[r]; To[4 + r] = Y[r]; To[8 + r] = Z[r]; To[12 + r] = pos[r];
        From[4 * r + 0] = X[r]; From[4 * r + 1] = Y[r]; From[4 * r + 2] = Z[r];
    }
    To[15] = From[15] = 1.0f;
    for (int r = 0; r < 3; r++) {
        const float* A = r == 0 ? X : (r == 1 ? Y : Z);
        From[12 + r] = -(A[0] * pos[0] + A[1] * pos[1] + A[2] * pos[2]);
    }
    return c;
}

static int Reproject()
{
    std::mt19937 rng(13);
    std::uniform_real_distribution<float> u(0.0f, 4.0f), s(-1.0f, 1.0f);
    const float nan = std::nanf(""), inf = HUGE_VALF;
    const float odd[] = {0.0f, -0.0f, -1.0f, nan, inf, -inf, 1e-45f, 1e-38f, 3e38f, 1.0f};
    const uint32_t sizes[][4] = {{1, 1, 1, 1}, {1, 1, 5, 3}, {7, 1, 1, 9}, {3, 2, 3, 2}, {16, 16, 16, 16},
                                 {29, 33, 37, 21}, {64, 32, 37, 21}, {17, 33, 40, 24}};
    const float origin[3] = {0.0f, -4.0f, 1.0f}, aside[3] = {0.4f, -4.0f, 1.0f}, far_away[3] = {1e30f, -4.0f, 1.0f},
                nowhere[3] = {nan, inf, 0.0f};
    int bad = 0;
    for (auto& z : sizes) {
        const uint32_t Wp = z[0], Hp = z[1], W = z[2], H = z[3];
        const size_t np = (size_t)Wp * Hp, n = (size_t)W * H;
        for (uint32_t model = 0; model < 4; model++) {       // 3: an unknown model
            // the previous camera: a small move, turned away, far outside, non-finite, a zero matrix
            pt_packed_camera prev[6] = {SanCamera(model, aside, 0.1f), SanCamera(model, origin, 3.14159265f),
                                        SanCamera(model, origin, 1.2f), SanCamera(model, far_away, 0.0f),
                                        SanCamera(model, nowhere, nan), SanCamera(model, origin, 0.0f)};
            std::memset(&prev[5].Transform, 0, sizeof(prev[5].Transform));
            const pt_packed_camera cur = SanCamera(model == 3 ? 0 : model, origin, 0.0f);
            for (int pc = 0; pc < 6; pc++) {
                for (int kind = 0; kind < 3; kind++) {        // history: random, empty, odd values
                    std::vector<float> acc(4 * np), out(4 * n, -1.0f);
                    std::vector<pt_denoise_guide> gp(np), gc(n);
                    for (size_t i = 0; i < 4 * np; i++)
                        acc[i] = kind == 0 ? (i % 4 == 3 ? (float)(rng() % 5) : u(rng))
                                           : (kind == 1 ? 0.0f : odd[rng() % (sizeof(odd) / sizeof(odd[0]))]);
                    for (std::vector<pt_denoise_guide>* g : {&gp, &gc}) {
                        for (pt_denoise_guide& r : *g) {
                            for (int k = 0; k < 3; k++) { r.normal[k] = s(rng); r.albedo[k] = 0.5f * u(rng); }
                            r.time = rng() % 16 == 0 ? odd[rng() % (sizeof(odd) / sizeof(odd[0]))] : 1.0f + u(rng);
                            r.shape = rng() % 4 == 0 ? 0xFFFFFFFFu : rng() % 3;
                        }
                    }
                    pt_reproject_parameters p{0.5f, 0.5f, 0.25f, kind == 2 ? inf : 8.0f};
                    if (ptsReproject(Wp, Hp, acc.data(), gp.data(), &prev[pc], W, H, gc.data(), &cur, &p, out.data()) != 0) {
                        std::printf("reproject: failed\n");
                        return 1;
                    }
                    size_t carried = 0;
                    for (size_t i = 0; i < n; i++) {
                        carried += out[4 * i + 3] > 0.0f;
                        bad += !(out[4 * i + 3] >= 0.0f);                       // a count, never NaN or negative
                        bad += kind != 2 && out[4 * i + 3] > 8.0f;             // capped
                    }
                    bad += kind == 1 && carried != 0;                            // an empty history carries nothing
                    bad += (model == 3 || pc == 4 || pc == 5) && carried != 0;   // no projection: no history
                    std::printf("reproject %ux%u -> %ux%u model %u prev %d history %d: %zu of %zu pixels\n", Wp, Hp, W,
                                H, model, pc, kind, carried, n);
                }
            }
            float o[3], v[3];
            for (uint32_t y = 0; y < H; y++)
                for (uint32_t x = 0; x < W; x++) bad += (ptsCentralCameraRay(&cur, x, y, W, H, o, v) != 0);
            bad += ptsCentralCameraRay(&prev[4], 0, 0, W, H, o, v) != (model == 3 ? -1 : 0);
        }
    }
    // rejected arguments leave `out` untouched
    float acc[4] = {1, 1, 1, 1}, out[4] = {7, 7, 7, 7};
    pt_denoise_guide gp{}, gc{};
    const pt_packed_camera cam = SanCamera(0, origin, 0.0f);
    pt_reproject_parameters ok{0.9f, 0.05f, 0.25f, 64.0f}, cosine{-1.0f, 0.02f, 0.25f, 64.0f}, depth{0.9f, 0.0f, 0.25f, 64.0f},
        weight{0.9f, 0.02f, 1.5f, 64.0f}, cap{0.9f, 0.02f, 0.25f, nan};
    bad += ptsReproject(1, 1, nullptr, &gp, &cam, 1, 1, &gc, &cam, &ok, out) == 0;
    bad += ptsReproject(1, 1, acc, nullptr, &cam, 1, 1, &gc, &cam, &ok, out) == 0;
    bad += ptsReproject(1, 1, acc, &gp, nullptr, 1, 1, &gc, &cam, &ok, out) == 0;
    bad += ptsReproject(1, 1, acc, &gp, &cam, 1, 1, nullptr, &cam, &ok, out) == 0;
    bad += ptsReproject(1, 1, acc, &gp, &cam, 1, 1, &gc, nullptr, &ok, out) == 0;
    bad += ptsReproject(1, 1, acc, &gp, &cam, 1, 1, &gc, &cam, nullptr, out) == 0;
    bad += ptsReproject(1, 1, acc, &gp, &cam, 1, 1, &gc, &cam, &ok, nullptr) == 0;
    bad += ptsReproject(1, 1, acc, &gp, &cam, 1, 1, &gp, &cam, &ok, out) == 0;
    bad += ptsReproject(0, 1, acc, &gp, &cam, 1, 1, &gc, &cam, &ok, out) == 0;
    bad += ptsReproject(1, 1, acc, &gp, &cam, 1, 0, &gc, &cam, &ok, out) == 0;
    for (pt_reproject_parameters* p : {&cosine, &depth, &weight, &cap})
        bad += ptsReproject(1, 1, acc, &gp, &cam, 1, 1, &gc, &cam, p, out) == 0;
    for (float v : out) bad += v != 7.0f;
    std::printf("reproject: %d checks wrong\n", bad);
    return bad != 0;
}

// ptsShapeMotion and ptsReprojectMoving on random tables:
// every flag combination, NaN / infinite / zero matrices, tables shorter than
// the guides' shape indices, frames from 1x1 to 67x45.
static int ReprojectMoving()
{
    std::mt19937 rng(14);
    std::uniform_real_distribution<float> u(0.0f, 4.0f), s(-1.0f, 1.0f);
    const float nan = std::nanf(""), inf = HUGE_VALF;
    const float odd[] = {0.0f, -0.0f, -1.0f, nan, inf, -inf, 1e-45f, 1e-38f, 3e38f, 1.0f};
    const size_t nodd = sizeof(odd) / sizeof(odd[0]);
    const uint32_t sizes[][4] = {{1, 1, 1, 1}, {1, 1, 5, 3}, {7, 1, 1, 9}, {16, 16, 17, 16}, {29, 33, 37, 21},
                                 {64, 40, 50, 37}, {67, 45, 67, 45}};
    const float origin[3] = {0.0f, -4.0f, 1.0f}, aside[3] = {0.4f, -4.0f, 1.0f};
    int bad = 0;
    for (auto& z : sizes) {
        const uint32_t Wp = z[0], Hp = z[1], W = z[2], H = z[3];
        const size_t np = (size_t)Wp * Hp, n = (size_t)W * H;
        for (uint32_t model = 0; model < 3; model++) {
            const pt_packed_camera prev = SanCamera(model, aside, 0.1f), cur = SanCamera(model, origin, 0.0f);
            for (uint32_t shapes = 0; shapes < 6; shapes += 1 + shapes / 2) {     // 0, 1, 2, 4 records; guides index 0..4 and beyond
                // two packs: a small move, an equal transform, another type, a NaN, an odd value per shape
                std::vector<pt_packed_shape> a(5), b(5);
                for (int i = 0; i < 5; i++) {
                    const float pos[3] = {s(rng), s(rng), u(rng)};
                    const pt_packed_camera t0 = SanCamera(0, pos, s(rng)), t1 = SanCamera(0, aside, s(rng));
                    a[i].Transform = t0.Transform;
                    b[i].Transform = rng() % 3 == 0 ? t0.Transform : t1.Transform;
                    a[i].Type = b[i].Type = 2;
                    if (rng() % 5 == 0) b[i].Type = 3;
                    if (rng() % 5 == 0) b[i].MeshRootNodeIndex = 7;
                    if (rng() % 4 == 0) b[i].Transform.From[rng() % 16] = odd[rng() % nodd];
                    if (rng() % 4 == 0) a[i].Transform.To[rng() % 16] = odd[rng() % nodd];
                }
                std::vector<pt_shape_motion> table(shapes + 1);
                if (ptsShapeMotion(a.data(), shapes > 2 ? shapes - 1 : shapes, b.data(), shapes, table.data()) != 0) {
                    std::printf("shape motion: failed\n");
                    return 1;
                }
                for (uint32_t i = 0; i < shapes; i++) {
                    bad += table[i].Flags > 2;
                    if (table[i].Flags == PT_SHAPE_MOTION_NO_HISTORY)
                        for (float v : table[i].Point) bad += v != 0.0f;
                }
                for (int kind = 0; kind < 3; kind++) {        // the table: as computed, flags scrambled, odd entries
                    std::vector<pt_shape_motion> m(table.begin(), table.begin() + shapes);
                    for (pt_shape_motion& r : m) {
                        if (kind >= 1) r.Flags = rng() % 8;
                        if (kind == 2)
                            for (int k = 0; k < 4; k++) (rng() % 2 ? r.Point[rng() % 12] : r.Normal[rng() % 9]) = odd[rng() % nodd];
                    }
                    std::vector<float> acc(4 * np), out(4 * n, -1.0f);
                    std::vector<pt_denoise_guide> gp(np), gc(n);
                    for (size_t i = 0; i < 4 * np; i++)
                        acc[i] = kind == 2 && rng() % 8 == 0 ? odd[rng() % nodd] : (i % 4 == 3 ? (float)(rng() % 5) : u(rng));
                    for (std::vector<pt_denoise_guide>* g : {&gp, &gc}) {
                        for (pt_denoise_guide& r : *g) {
                            for (int k = 0; k < 3; k++) { r.normal[k] = s(rng); r.albedo[k] = 0.5f * u(rng); }
                            r.time = rng() % 16 == 0 ? odd[rng() % nodd] : 1.0f + u(rng);
                            r.shape = rng() % 4 == 0 ? 0xFFFFFFFFu : (rng() % 16 == 0 ? rng() : rng() % 5);
                        }
                    }
                    pt_reproject_parameters p{0.5f, 0.5f, 0.25f, 8.0f};
                    // shapes == 0: a table of no records (a valid pointer, count 0)
                    if (ptsReprojectMoving(Wp, Hp, acc.data(), gp.data(), &prev, W, H, gc.data(), &cur, table.data(), 0, &p, out.data()) != 0 ||
                        ptsReprojectMoving(Wp, Hp, acc.data(), gp.data(), &prev, W, H, gc.data(), &cur,
                                           shapes ? m.data() : table.data(), shapes, &p, out.data()) != 0) {
                        std::printf("reproject_moving: failed\n");
                        return 1;
                    }
                    size_t carried = 0;
                    for (size_t i = 0; i < n; i++) {
                        carried += out[4 * i + 3] > 0.0f;
                        bad += !(out[4 * i + 3] >= 0.0f);                       // a count, never NaN or negative
                        bad += out[4 * i + 3] > 8.0f;                           // capped
                        // beyond the table or flagged NO_HISTORY: nothing carried
                        const uint32_t sh = gc[i].shape;
                        if (sh != 0xFFFFFFFFu && (sh >= shapes || (m[sh].Flags & PT_SHAPE_MOTION_NO_HISTORY)))
                            bad += out[4 * i + 3] != 0.0f;
                    }
                    std::printf("reproject_moving %ux%u -> %ux%u model %u records %u table %d: %zu of %zu pixels\n", Wp,
                                Hp, W, H, model, shapes, kind, carried, n);
                }
            }
        }
    }
    // rejected arguments leave `out` untouched; no table is ptsReproject
    float acc[4] = {1, 1, 1, 1}, out[4] = {7, 7, 7, 7}, row8[4], none[4];
    pt_denoise_guide gp{}, gc{};
    pt_shape_motion m{};
    const pt_packed_camera cam = SanCamera(0, origin, 0.0f);
    pt_reproject_parameters ok{0.9f, 0.05f, 0.25f, 64.0f}, depth{0.9f, 0.0f, 0.25f, 64.0f};
    bad += ptsReprojectMoving(1, 1, acc, &gp, &cam, 1, 1, &gc, &cam, nullptr, 1, &ok, out) == 0;
    bad += ptsReprojectMoving(1, 1, nullptr, &gp, &cam, 1, 1, &gc, &cam, &m, 1, &ok, out) == 0;
    bad += ptsReprojectMoving(1, 1, acc, &gp, &cam, 1, 1, &gp, &cam, &m, 1, &ok, out) == 0;
    bad += ptsReprojectMoving(1, 1, acc, &gp, &cam, 0, 1, &gc, &cam, &m, 1, &ok, out) == 0;
    bad += ptsReprojectMoving(1, 1, acc, &gp, &cam, 1, 1, &gc, &cam, &m, 1, &depth, out) == 0;
    bad += ptsReprojectMoving(1, 1, acc, &gp, &cam, 1, 1, &gc, &cam, &m, 1, &ok, nullptr) == 0;
    bad += ptsReprojectMoving(1, 1, acc, &gp, &cam, 1, 1, &gc, nullptr, nullptr, 0, &ok, out) == 0;
    for (float v : out) bad += v != 7.0f;
    bad += ptsShapeMotion(nullptr, 1, nullptr, 0, nullptr) == 0;
    bad += ptsShapeMotion(nullptr, 0, nullptr, 1, &m) == 0;
    bad += ptsShapeMotion(nullptr, 0, nullptr, 0, nullptr) != 0;
    bad += ptsReproject(1, 1, acc, &gp, &cam, 1, 1, &gc, &cam, &ok, row8) != 0;
    bad += ptsReprojectMoving(1, 1, acc, &gp, &cam, 1, 1, &gc, &cam, nullptr, 0, &ok, none) != 0;
    bad += std::memcmp(row8, none, sizeof(row8)) != 0;
    std::printf("reproject_moving: %d checks wrong\n", bad);
    return bad != 0;
}

// ptsRectifyHistory: the images lie in arrays of exactly
// 4 * W * H floats and W * H guide records, so a window tap past an edge is
// ASan's.  A count is only ever cut; in place equals out of place.
static int Rectify()
{
    std::mt19937 rng(17);
    std::uniform_real_distribution<float> u(0.0f, 4.0f);
    const float nan = std::nanf(""), inf = HUGE_VALF;
    const float odd[] = {0.0f, -0.0f, -1.0f, nan, inf, -inf, 1e-45f, 1e-38f, 3e38f, 1.0f, 4294967296.0f, 2.3283064e-10f};
    const uint32_t sizes[][2] = {{1, 1}, {1, 7}, {3, 2}, {5, 3}, {15, 15}, {16, 16}, {17, 16}, {16, 17}, {33, 18}, {67, 45}};
    const pt_rectify_parameters sets[] = {{1, 1, 1.0f, 8.0f, 0.9f}, {2, 6, 0.0f, 8.0f, 0.9f}, {3, 9, 1.0f, inf, 0.9f},
                                          {3, 49, 1.0f, 8.0f, 1.0f}, {2, 1, 2.5f, 0.5f, -0.999f}};
    int bad = 0;
    for (auto& wh : sizes) {
        const uint32_t W = wh[0], H = wh[1];
        const size_t n = (size_t)W * H;
        // kind 0: random; 1: all empty; 2: every component drawn from the odd values (NaN, inf, denormals ...)
        for (int kind = 0; kind < 3; kind++) {
            std::vector<float> hist(4 * n), cur(4 * n);
            std::vector<pt_denoise_guide> g(n);
            for (std::vector<float>* v : {&hist, &cur}) {
                for (size_t i = 0; i < 4 * n; i++) {
                    if (kind == 0) (*v)[i] = i % 4 == 3 ? (float)(rng() % 70) : u(rng);
                    else if (kind == 1) (*v)[i] = 0.0f;
                    else (*v)[i] = odd[rng() % (sizeof(odd) / sizeof(odd[0]))];
                }
            }
            for (size_t i = 0; i < n; i++) {
                const uint32_t pick = rng() % 8;
                g[i].shape = pick == 0 ? PT_SHAPE_INDEX_NONE : pick % 3;
                for (int k = 0; k < 3; k++)
                    g[i].normal[k] = kind == 2 ? odd[rng() % (sizeof(odd) / sizeof(odd[0]))] : (k == 2 ? 1.0f : 0.01f * (float)(rng() % 60));
                g[i].time = 1.0f;
                g[i].albedo[0] = g[i].albedo[1] = g[i].albedo[2] = 0.5f;
            }
            for (const pt_rectify_parameters& p : sets) {
                std::vector<float> out(4 * n, -7.0f), in_place(hist);
                if (ptsRectifyHistory(W, H, hist.data(), cur.data(), g.data(), &p, out.data()) != 0 ||
                    ptsRectifyHistory(W, H, in_place.data(), cur.data(), g.data(), &p, in_place.data()) != 0) {
                    std::printf("rectify: failed\n");
                    return 1;
                }
                bad += std::memcmp(out.data(), in_place.data(), 4 * n * sizeof(float)) != 0;
                size_t kept = 0, cut = 0, none = 0;
                for (size_t i = 0; i < n; i++) {
                    const float* h = &hist[4 * i];
                    const float* o = &out[4 * i];
                    const bool usable = std::isfinite(h[0]) && std::isfinite(h[1]) && std::isfinite(h[2]) &&
                                        std::isfinite(h[3]) && h[3] > 0.0f;
                    if (!usable) { none++; bad += o[0] != 0.0f || o[1] != 0.0f || o[2] != 0.0f || o[3] != 0.0f; continue; }
                    if (std::memcmp(h, o, 4 * sizeof(float)) == 0) { kept++; continue; }
                    cut++;
                    bad += !(o[3] <= h[3] && o[3] <= p.ClampedHistory && o[3] > 0.0f);
                }
                std::printf("rectify %ux%u kind %d radius %u min %u sigma %g clamp %g: kept %zu cut %zu none %zu\n", W, H, kind,
                            p.Radius, p.MinNeighbours, (double)p.Sigma, (double)p.ClampedHistory, kept, cut, none);
            }
        }
    }
    // rejected arguments leave `out` untouched
    float hist[4] = {1, 1, 1, 1}, cur[4] = {1, 2, 1, 1}, out[4], before[4];
    std::memset(out, 0x55, sizeof(out));
    std::memcpy(before, out, sizeof(out));
    pt_denoise_guide g;
    std::memset(&g, 0, sizeof(g));
    const pt_rectify_parameters ok = {3, 9, 1.0f, 8.0f, 0.9f};
    bad += ptsRectifyHistory(1, 1, nullptr, cur, &g, &ok, out) == 0;
    bad += ptsRectifyHistory(1, 1, hist, nullptr, &g, &ok, out) == 0;
    bad += ptsRectifyHistory(1, 1, hist, cur, nullptr, &ok, out) == 0;
    bad += ptsRectifyHistory(1, 1, hist, cur, &g, nullptr, out) == 0;
    bad += ptsRectifyHistory(1, 1, hist, cur, &g, &ok, nullptr) == 0;
    bad += ptsRectifyHistory(0, 1, hist, cur, &g, &ok, out) == 0;
    bad += ptsRectifyHistory(1, 0, hist, cur, &g, &ok, out) == 0;
    bad += ptsRectifyHistory(1, 1, cur, cur, &g, &ok, out) == 0;
    const pt_rectify_parameters wrong[] = {{0, 9, 1.0f, 8.0f, 0.9f}, {4, 9, 1.0f, 8.0f, 0.9f}, {3, 0, 1.0f, 8.0f, 0.9f},
                                           {3, 50, 1.0f, 8.0f, 0.9f}, {3, 9, -1.0f, 8.0f, 0.9f}, {3, 9, inf, 8.0f, 0.9f},
                                           {3, 9, nan, 8.0f, 0.9f}, {3, 9, 1.0f, 0.0f, 0.9f}, {3, 9, 1.0f, nan, 0.9f},
                                           {3, 9, 1.0f, 8.0f, -1.0f}, {3, 9, 1.0f, 8.0f, 1.5f}, {3, 9, 1.0f, 8.0f, nan}};
    for (const pt_rectify_parameters& p : wrong) bad += ptsRectifyHistory(1, 1, hist, cur, &g, &p, out) == 0;
    bad += std::memcmp(out, before, sizeof(out)) != 0;
    bad += ptsRectifyHistory(1, 1, hist, cur, &g, &ok, cur) == 0;          // out is current
    bad += cur[1] != 2.0f;
    const pt_rectify_parameters one = {1, 1, 0.0f, 8.0f, 0.9f};
    g.normal[2] = 1.0f;                                                    // the centre is its own window
    bad += ptsRectifyHistory(1, 1, hist, cur, &g, &one, out) != 0 || out[0] != 1.0f || out[1] != 2.0f || out[3] != 1.0f;
    std::printf("rectify: %d checks wrong\n", bad);
    return bad != 0;
}

// ptsDespike: the image lies in arrays of exactly
// 4 * W * H floats and W * H guide records, so a window tap past an edge is
// ASan's.  A count keeps its bits; a pixel keeps all its bits or is usable and
// no component grows.
static int Despike()
{
    std::mt19937 rng(19);
    std::uniform_real_distribution<float> u(0.0f, 4.0f);
    const float nan = std::nanf(""), inf = HUGE_VALF;
    const float odd[] = {0.0f, -0.0f, -1.0f, nan, inf, -inf, 1e-45f, 1e-38f, 3e38f, 1.0f, 4294967296.0f, 2.3283064e-10f};
    const uint32_t sizes[][2] = {{1, 1}, {1, 7}, {3, 2}, {5, 3}, {15, 15}, {16, 16}, {17, 16}, {16, 17}, {33, 18}, {67, 45}};
    int bad = 0;
    for (auto& wh : sizes) {
        const uint32_t W = wh[0], H = wh[1];
        const size_t n = (size_t)W * H;
        // kind 0: random with spikes; 1: all empty; 2: every component drawn from the odd values (NaN, inf, denormals ...)
        for (int kind = 0; kind < 3; kind++) {
            std::vector<float> src(4 * n);
            std::vector<pt_denoise_guide> g(n);
            for (size_t i = 0; i < 4 * n; i++) {
                if (kind == 0) src[i] = i % 4 == 3 ? (float)(rng() % 70) : u(rng) * (rng() % 16 == 0 ? 50.0f : 1.0f);
                else if (kind == 1) src[i] = 0.0f;
                else src[i] = odd[rng() % (sizeof(odd) / sizeof(odd[0]))];
            }
            for (size_t i = 0; i < n; i++) {
                const uint32_t pick = rng() % 8;
                g[i].shape = pick == 0 ? PT_SHAPE_INDEX_NONE : pick % 3;
                for (int k = 0; k < 3; k++)
                    g[i].normal[k] = kind == 2 ? odd[rng() % (sizeof(odd) / sizeof(odd[0]))] : (k == 2 ? 1.0f : 0.01f * (float)(rng() % 60));
                g[i].time = 1.0f;
                g[i].albedo[0] = g[i].albedo[1] = g[i].albedo[2] = 0.5f;
            }
            for (uint32_t radius = 1; radius <= 3; radius++) {
                const uint32_t all = (2 * radius + 1) * (2 * radius + 1) - 1;
                size_t kept = 0, clamped = 0;              // over every Rank and setting
                for (uint32_t rank = 1; rank <= 4; rank++) {
                    const pt_despike_parameters sets[] = {{radius, rank, rank, 2.0f, 0.0f, 0.9f}, {radius, rank, all, 0.0f, 0.0f, 1.0f},
                                                          {radius, rank, 8, 1.5f, 0.25f, -0.999f}};
                    for (const pt_despike_parameters& p : sets) {
                        std::vector<float> out(4 * n, -7.0f);
                        if (ptsDespike(W, H, src.data(), g.data(), &p, out.data()) != 0) {
                            std::printf("despike: failed\n");
                            return 1;
                        }
                        for (size_t i = 0; i < n; i++) {
                            const float* s = &src[4 * i];
                            const float* o = &out[4 * i];
                            if (std::memcmp(s, o, 4 * sizeof(float)) == 0) { kept++; continue; }
                            clamped++;
                            const bool usable = std::isfinite(s[0]) && std::isfinite(s[1]) && std::isfinite(s[2]) &&
                                                std::isfinite(s[3]) && s[3] > 0.0f;
                            bad += !usable || std::memcmp(&s[3], &o[3], sizeof(float)) != 0;
                            for (int k = 0; k < 3; k++) bad += !(std::fabs(o[k]) <= std::fabs(s[k]));
                        }
                    }
                }
                std::printf("despike %ux%u kind %d radius %u, ranks 1-4 x 3 settings: kept %zu clamped %zu\n", W, H, kind, radius,
                            kept, clamped);
            }
        }
    }
    // rejected arguments leave `out` untouched
    float src[4] = {1, 2, 1, 1}, out[4], before[4];
    std::memset(out, 0x55, sizeof(out));
    std::memcpy(before, out, sizeof(out));
    pt_denoise_guide g;
    std::memset(&g, 0, sizeof(g));
    const pt_despike_parameters ok = {1, 1, 1, 2.0f, 0.0f, 0.9f};
    bad += ptsDespike(1, 1, nullptr, &g, &ok, out) == 0;
    bad += ptsDespike(1, 1, src, nullptr, &ok, out) == 0;
    bad += ptsDespike(1, 1, src, &g, nullptr, out) == 0;
    bad += ptsDespike(1, 1, src, &g, &ok, nullptr) == 0;
    bad += ptsDespike(0, 1, src, &g, &ok, out) == 0;
    bad += ptsDespike(1, 0, src, &g, &ok, out) == 0;
    bad += ptsDespike(1, 1, src, &g, &ok, src) == 0;                       // out is the input
    const pt_despike_parameters wrong[] = {{0, 1, 1, 2.0f, 0.0f, 0.9f}, {4, 1, 1, 2.0f, 0.0f, 0.9f}, {3, 0, 1, 2.0f, 0.0f, 0.9f},
                                           {3, 5, 8, 2.0f, 0.0f, 0.9f}, {3, 3, 2, 2.0f, 0.0f, 0.9f}, {3, 3, 49, 2.0f, 0.0f, 0.9f},
                                           {2, 3, 25, 2.0f, 0.0f, 0.9f}, {1, 3, 9, 2.0f, 0.0f, 0.9f}, {3, 3, 8, -1.0f, 0.0f, 0.9f},
                                           {3, 3, 8, inf, 0.0f, 0.9f}, {3, 3, 8, nan, 0.0f, 0.9f}, {3, 3, 8, 2.0f, -1.0f, 0.9f},
                                           {3, 3, 8, 2.0f, -0.0f, 0.9f}, {3, 3, 8, 2.0f, inf, 0.9f}, {3, 3, 8, 2.0f, nan, 0.9f},
                                           {3, 3, 8, 2.0f, 0.0f, -1.0f}, {3, 3, 8, 2.0f, 0.0f, 1.5f}, {3, 3, 8, 2.0f, 0.0f, nan}};
    for (const pt_despike_parameters& p : wrong) bad += ptsDespike(1, 1, src, &g, &p, out) == 0;
    bad += std::memcmp(out, before, sizeof(out)) != 0;
    bad += src[1] != 2.0f;
    bad += ptsDespike(1, 1, src, &g, &ok, out) != 0 || std::memcmp(out, src, sizeof(out)) != 0;   // no neighbour: untested
    std::printf("despike: %d checks wrong\n", bad);
    return bad != 0;
}

// include/pt_guides.h on the host: the functions the
// guide kernel's SPECULAR instantiation calls per hit.
static int Guides()
{
    const float nan = std::nanf(""), inf = INFINITY, tiny = 1e-42f;
    int bad = 0;
    size_t calls = 0, followed = 0, refracted = 0, mirrored = 0, finite = 0;
    // classification
    const uint32_t types[] = {PT_MATERIAL_TYPE_BASIC_DIFFUSE, PT_MATERIAL_TYPE_BASIC_METAL, PT_MATERIAL_TYPE_BASIC_TRANSLUCENT,
                              PT_MATERIAL_TYPE_OPENPBR, 4u, 0xFFFFFFFFu};
    const float roughs[] = {0.0f, -0.0f, tiny, 9.99e-4f, 1e-3f, 1.001e-3f, 1.0f, -1.0f, inf, -inf, nan};
    const uint32_t caps[] = {0u, 1u, 4u, PT_GUIDE_MAX_BOUNCES, PT_GUIDE_MAX_BOUNCES + 1u, 0xFFFFFFFFu};
    for (uint32_t type : types)
        for (float r : roughs)
            for (uint32_t cap : caps)
                for (uint32_t b = 0; b <= PT_GUIDE_MAX_BOUNCES + 1u; b++) {
                    const int f = pt_guide_followed(type, r, b, cap);
                    const int want = b < cap && (type == PT_MATERIAL_TYPE_BASIC_METAL || type == PT_MATERIAL_TYPE_BASIC_TRANSLUCENT) &&
                                     r < 1e-3f;
                    bad += f != want;
                    bad += pt_guide_candidate(type) != (type == 1u || type == 2u);
                    if (pt_guide_candidate(type))
                        bad += pt_guide_roughness_word(type) != (type == 1u ? (uint32_t)PT_BASIC_METAL_ROUGHNESS : (uint32_t)PT_BASIC_TRANSLUCENT_ROUGHNESS);
                    followed += f;
                    calls++;
                }
    // the tag and the shape word over the whole 16-bit range of shape indices
    for (uint32_t s = 0; s < 65536u; s += 257u) {
        const uint32_t tag = pt_guide_tag(0u, s);
        bad += tag != s + 1u || pt_guide_tag(tag, (s + 5u) & 0xFFFFu) != tag;
        bad += pt_guide_shape_word(tag, 65535u - s) != ((tag << 16) | (65535u - s)) || pt_guide_shape_word(0u, s) != s;
    }
    bad += pt_f2u(pt_guide_total(5.0f, -0.0f, 0u)) != 0x80000000u || pt_guide_total(5.0f, 2.0f, 1u) != 7.0f;
    // directions: frames and rays, well formed and not
    std::mt19937 rng(13);
    std::uniform_real_distribution<float> U(-1.0f, 1.0f);
    // A frame after its packed round trips is orthonormal to within twice the packed form's 6.5e-5, and
    // the checks below hold to a small multiple of that.
    const float tol = 1e-3f;
    struct frame { pt3 N, TX; bool unit; };
    std::vector<frame> frames = {{v3(0, 0, 1), v3(1, 0, 0), true}, {v3(0, -1, 0), v3(0, 0, -1), true},
                                 {v3(0, 0, 0), v3(1, 0, 0), false}, {v3(0, 0, 1), v3(0, 0, 0), false},
                                 {v3(nan, 0, 1), v3(1, 0, 0), false}, {v3(0, 0, 1), v3(nan, nan, nan), false},
                                 {v3(inf, 0, 0), v3(0, 1, 0), false}, {v3(tiny, tiny, tiny), v3(tiny, 0, 0), false},
                                 {v3(0, 0, 1e30f), v3(1e30f, 0, 0), false}};
    for (int i = 0; i < 40; i++) {
        pt3 N = normalize(v3(U(rng), U(rng), U(rng)));
        pt3 T = normalize(cross(pt_abs(N.x) < 0.9f ? v3(1, 0, 0) : v3(0, 1, 0), N));
        frames.push_back({pt_reproject_unpack_unit(pt_reproject_pack_unit(N)), pt_reproject_unpack_unit(pt_reproject_pack_unit(T)), true});
    }
    const float etas[] = {1.0f, 1.5f, 2.4f, 1.0003f, 0.999f, 0.5f, 0.0f, -0.0f, -1.5f, tiny, 1e30f, inf, nan};
    for (const frame& F : frames) {
        const pt3 TY = cross(F.N, F.TX);
        std::vector<pt3> rays = {F.N, -F.N, F.TX, -F.TX, TY,                               // along the normal; c = 0 exactly
                                 F.TX + 1e-8f * F.N, F.TX - 1e-8f * F.N, normalize(F.TX + 1e-4f * F.N),   // grazing
                                 normalize(F.TX - 1e-4f * F.N), v3(0, 0, 0), v3(nan, 0, 0), v3(inf, 0, 0), v3(tiny, 0, tiny)};
        for (int i = 0; i < 30; i++) rays.push_back(normalize(v3(U(rng), U(rng), U(rng))));
        for (size_t r = 0; r < rays.size(); r++) {
            const pt3 V = rays[r];
            const bool unit_ray = r < 5 || (r >= 7 && r < 9) || r >= 13;
            for (uint32_t type : types) {
                for (float eta : etas) {
                    const pt3 W = pt_guide_direction(type, eta, F.N, F.TX, V);
                    pt3 O = v3(1, 2, 3), V2 = V;
                    pt_guide_restart(&O, &V2, 2.5f, W);
                    calls++;
                    const bool ok = W.x == W.x && W.y == W.y && W.z == W.z && pt_reproject_finite(W.x) &&
                                    pt_reproject_finite(W.y) && pt_reproject_finite(W.z);
                    finite += ok;
                    if (!(F.unit && unit_ray)) continue;
                    const float c = -dot(V, F.N);
                    const pt3 Mirror = V + (2.0f * c) * F.N;
                    const bool glass = type == PT_MATERIAL_TYPE_BASIC_TRANSLUCENT;
                    const float rel = c < 0.0f ? eta : 1.0f / eta;
                    const bool bends = glass && 1.0f - (rel * rel) * (1.0f - c * c) > 0.0f;
                    (bends ? refracted : mirrored)++;
                    if (!bends) {
                        bad += !(length(W - Mirror) < tol);                          // metal, every other type, TIR, bad index
                    } else if (eta >= 0.1f && eta <= 10.0f && c != 0.0f) {
                        // (an index whose square overflows gives infinite components, and c = 0 exactly gives
                        // cr = 0 and a tangential W of length rel: both defined, both normalised or dropped by
                        // the packed round trip, neither held to the identities below)
                        bad += !(pt_abs(length(W) - 1.0f) < tol);                    // |In|^2 = rel^2 (1 - c^2) + k = 1
                        bad += !(dot(W, F.N) * dot(V, F.N) >= -tol);                  // through the surface
                        if (eta == 1.0f) bad += !(length(W - V) < tol);              // no interface: straight on
                        // Snell, on the tangential parts: |W_t| = rel |V_t|
                        const pt3 Vt = V - dot(V, F.N) * F.N, Wt = W - dot(W, F.N) * F.N;
                        bad += !(pt_abs(length(Wt) - rel * length(Vt)) < tol * (1.0f + rel));
                    }
                    if (ok && length(W) > 0.5f) bad += !(pt_abs(length(V2) - 1.0f) < 1e-5f);   // the round trip gives a unit vector
                }
            }
        }
    }
    std::printf("guides: %zu calls, %zu followed, %zu refracted, %zu mirrored, %zu finite directions: %d checks wrong\n",
                calls, followed, refracted, mirrored, finite, bad);
    return bad != 0;
}

int main(int argc, char** argv)
{
    if (argc < 2) { std::fprintf(stderr, "usage: san_driver decode|model|scene|render|bvh|denoise|stats|tile_stats|reproject|reproject_moving|rectify|despike|guides ...\n"); return 2; }
    std::string cmd = argv[1];
    if (cmd == "decode") return Decode(argc - 2, argv + 2);
    if (cmd == "model") return Model(argc - 2, argv + 2);
    if (cmd == "scene") return Scene(argc - 2, argv + 2);
    if (cmd == "render") return Render();
    if (cmd == "bvh") return Bvh(argc > 2 ? (uint32_t)std::strtoul(argv[2], nullptr, 10) : 200000u);
    if (cmd == "denoise") return Denoise();
    if (cmd == "stats") return Stats();
    if (cmd == "tile_stats") return TileStats();
    if (cmd == "reproject") return Reproject();
    if (cmd == "reproject_moving") return ReprojectMoving();
    if (cmd == "rectify") return Rectify();
    if (cmd == "despike") return Despike();
    if (cmd == "guides") return Guides();
    std::fprintf(stderr, "unknown command %s\n", cmd.c_str());
    return 2;
}
