// Stand-alone host-sanitizer check of the ray-query host code (`make -C
// ray-tracer-from-scratch_amd asan-rays` builds it with AddressSanitizer + UBSan against the
// sanitized objects of `make asan` and the C++ mirror, and runs it; CPU only, no preloaded
// runtime).  It packs scenes through the host-only rt_frame_boxes (pack_scene: spheres,
// walls, an interleaved order, a wall with a NaN basis), orders dispatch units through the
// host-only rt_order_units (rt_row_order.cpp), walks the argument checks of
// rt_trace_rays, rt_trace_rays_device, rt_occluded*, rt_render_aov*, rt_set_lights and
// rt_set_transmission (its host half, pack_transmission, directly: a set, both ways of clearing
// and every refused argument, with no device), and converts hit records to Collisions.  Where a HIP device exists it also runs the entry points on a small batch; without one
// rt_ctx_create returns RT_ERR_NO_DEVICE and the device part is skipped (and said so).
#include <algorithm>
#include <cfloat>
#include <cmath>
#include <cstdio>
#include <cstring>
#include <memory>
#include <stdexcept>
#include <vector>

#include "rt/scene.h"
#include "../ray-tracer-from-scratch_amd/csrc/rt_host.h"  // pack_scene, pack_transmission (linked in)

static int g_fail = 0;
#define EXPECT(cond)                                                      \
    do {                                                                  \
        if (!(cond)) {                                                    \
            std::printf("FAIL line %d: %s\n", __LINE__, #cond);           \
            g_fail++;                                                     \
        }                                                                 \
    } while (0)

static std::vector<rt_prim> pack(const std::vector<std::unique_ptr<SceneGeometry>>& scene) {
    std::vector<rt_prim> prims(scene.size());
    for (size_t j = 0; j < scene.size(); j++) scene[j]->pack(&prims[j]);
    return prims;
}

int main() {
    // wall, sphere, wall, sphere, plus a wall whose basis is NaN (normal along z: never hit,
    // not uploaded) and 40 more spheres (clusters are built)
    std::vector<std::unique_ptr<SceneGeometry>> scene;
    scene.push_back(std::make_unique<Wall>(Material(RGB(0, 0, 1)), point3(3.0, 2, 0), vec3(0, -1, 0), 1, 1));
    scene.push_back(std::make_unique<Sphere>(Material(RGB(0, 1, 0), 0.5), point3(1.5, 0, 0), .5));
    scene.push_back(std::make_unique<Wall>(Material(RGB(0, 1, 0)), point3(3.0, -3, 0), vec3(0, 1, 0), 2, 2));
    scene.push_back(std::make_unique<Sphere>(Material(RGB(1, 0, 0), 0.2), point3(2.5, 1, 0.2), .4));
    scene.push_back(std::make_unique<Wall>(Material(RGB(1, 1, 1)), point3(-1, -1, 3), vec3(0, 0, 1), 2, 2));
    for (int k = 0; k < 40; k++)
        scene.push_back(std::make_unique<Sphere>(Material(RGB(.5, .5, .5), 0.3),
                                                 point3(2 + 0.15 * k, -3 + 0.14 * k, -1 + 0.07 * k), .3));
    const std::vector<rt_prim> prims = pack(scene);

    Camera cam;
    cam.aspect_ratio = 64.0 / 48;
    cam.image_width = 64;
    cam.movement_speed = 0.1;
    cam.vfov = 90;
    cam.position = point3(0, 0, 0);
    cam.lookat = point3(-1, 0, 0);
    cam.vup = vec3(0, 0, -1);
    rt_camera c{};
    const double cpos[3] = {cam.position.x, cam.position.y, cam.position.z};
    const double clook[3] = {cam.lookat.x, cam.lookat.y, cam.lookat.z};
    const double cup[3] = {cam.vup.x, cam.vup.y, cam.vup.z};
    EXPECT(rt_camera_init(cpos, clook, cup, cam.vfov, cam.aspect_ratio, cam.image_width, &c) == RT_OK);
    // pack_scene + per-frame boxes, host only
    std::vector<int16_t> boxes(4 * 64 * 600);
    int32_t nbox = 0, mir = 0;
    EXPECT(rt_frame_boxes(prims.data(), (int32_t)prims.size(), &c, 0, c.height, boxes.data(),
                          (int32_t)(boxes.size() / 4), &nbox, &mir) == RT_OK);
    EXPECT(rt_frame_boxes(prims.data(), 5, &c, 0, c.height, boxes.data(), (int32_t)(boxes.size() / 4),
                          &nbox, &mir) == RT_OK);

    // the measured dispatch order (order_units, mix_units), host only: mode 0 against the
    // two-line rule — heaviest maximum first, ties keep the lower unit — and mode 1 a
    // permutation that starts with the same unit; n = 1; all units equal (both modes: index order)
    {
        const int n = 37;
        std::vector<uint32_t> umax(n), usum(n);
        for (int u = 0; u < n; u++) {
            umax[u] = (uint32_t)((u * 7919u) % 23u) * 3000u;  // ties, and values above 65535 (saturate)
            usum[u] = umax[u] * (uint32_t)(1 + u % 5) + 1u;
        }
        std::vector<int16_t> want(n);
        for (int u = 0; u < n; u++) want[u] = (int16_t)u;
        std::stable_sort(want.begin(), want.end(), [&](int16_t a, int16_t b) {
            return std::min(umax[a], 65535u) > std::min(umax[b], 65535u);
        });
        std::vector<int16_t> perm(n, -1), mix(n, -1);
        EXPECT(rt_order_units(umax.data(), usum.data(), n, 0, perm.data()) == RT_OK);
        EXPECT(perm == want);
        EXPECT(rt_order_units(umax.data(), usum.data(), n, 1, mix.data()) == RT_OK);
        std::vector<int16_t> sorted(mix);
        std::sort(sorted.begin(), sorted.end());
        for (int u = 0; u < n; u++) EXPECT(sorted[u] == u);
        EXPECT(mix[0] == want[0]);
        const uint32_t one_max = 5, one_sum = 9;
        int16_t one[2] = {-1, -1};
        EXPECT(rt_order_units(&one_max, &one_sum, 1, 0, one) == RT_OK && one[0] == 0 && one[1] == -1);
        one[0] = -1;
        EXPECT(rt_order_units(&one_max, &one_sum, 1, 1, one) == RT_OK && one[0] == 0 && one[1] == -1);
        std::fill(umax.begin(), umax.end(), 1234u);
        std::fill(usum.begin(), usum.end(), 99u);
        for (int mode = 0; mode < 2; mode++) {
            EXPECT(rt_order_units(umax.data(), usum.data(), n, mode, perm.data()) == RT_OK);
            for (int u = 0; u < n; u++) EXPECT(perm[u] == u);
        }
        EXPECT(rt_order_units(umax.data(), usum.data(), n, 2, perm.data()) == RT_ERR_INVALID_ARG);
    }

    // argument checks that need no device
    const double o[6] = {0, 0, 0, 0.1, 0.2, 0.3}, d[6] = {1, 0, 0, 1, 0.3, -0.2};
    double rgb[6];
    rt_hit hits[2];
    rt_stats st;
    EXPECT(rt_trace_rays(nullptr, o, d, 2, 4, RT_PREC_F64, 0, RT_OUT_RGB_F64, rgb, hits, 1, &st) ==
           RT_ERR_INVALID_ARG);
    EXPECT(rt_trace_rays_device(nullptr, o, d, 2, 4, RT_PREC_F64, 0, RT_OUT_RGB_F64, rgb, hits, nullptr,
                                nullptr) == RT_ERR_INVALID_ARG);
    uint8_t occ[2] = {7, 7};
    uint64_t nocc = 9;
    const double tmax[2] = {1.0, 0.5};
    EXPECT(rt_occluded(nullptr, o, d, tmax, 2, occ, &nocc, &st) == RT_ERR_INVALID_ARG);
    EXPECT(rt_occluded_device(nullptr, o, d, tmax, 2, occ, &nocc, nullptr) == RT_ERR_INVALID_ARG);
    EXPECT(occ[0] == 7 && occ[1] == 7 && nocc == 9);
    rt_light lights[RT_MAX_LIGHTS + 1] = {};
    for (rt_light& l : lights) l.color[0] = l.color[1] = l.color[2] = 0.25;
    EXPECT(rt_set_lights(nullptr, lights, 1) == RT_ERR_INVALID_ARG);
    EXPECT(rt_multi_set_lights(nullptr, lights, 1) == RT_ERR_INVALID_ARG);
    EXPECT(sizeof(rt_light) == 48);
    // rt_set_transmission: without a ctx; then its host half on the packed scene (45 objects, 44
    // material slots: the NaN wall has none): a set, the refusals (the table stays), the clears
    std::vector<rt_transmission> recs(prims.size(), rt_transmission{0.0, 1.0});
    EXPECT(rt_set_transmission(nullptr, recs.data(), (int32_t)recs.size()) == RT_ERR_INVALID_ARG);
    EXPECT(rt_multi_set_transmission(nullptr, recs.data(), (int32_t)recs.size()) == RT_ERR_INVALID_ARG);
    EXPECT(sizeof(rt_transmission) == 16);
    {
        const int32_t n = (int32_t)prims.size();
        rth::SceneHost sc;
        EXPECT(rth::pack_scene(prims.data(), n, sc) == RT_OK);
        std::vector<rt::DevGlass> tab;
        recs[0] = rt_transmission{0.6, 1.0};   // the first wall: slot nS + 0
        recs[1] = rt_transmission{0.9, 1.5};   // the first sphere: slot 0
        recs[n - 1] = rt_transmission{1.0, 4.0};
        EXPECT(rth::pack_transmission(recs.data(), n, sc, tab) == RT_OK);
        EXPECT(tab.size() == (size_t)(sc.nS + sc.nW) && sc.nS + sc.nW == n - 1);
        EXPECT(tab[0].tau == 0.9 && tab[0].ior == 1.5 && tab[0].w == 0.9 && tab[0].wf == 0.9f);
        EXPECT(tab[(size_t)sc.nS].tau == 0.6 && tab[(size_t)sc.nS].w == 0.6);
        EXPECT(tab[1].tau == 0.0 && tab[1].w == 0.2);   // opaque: the slot's metallic
        EXPECT(tab[(size_t)sc.nS - 1].tau == 1.0 && tab[(size_t)sc.nS - 1].ior == 4.0);
        const std::vector<rt::DevGlass> kept = tab;
        auto refused = [&](const rt_transmission* r, int32_t cnt) {
            return rth::pack_transmission(r, cnt, sc, tab) == RT_ERR_INVALID_ARG && tab.size() == kept.size() &&
                   std::memcmp(tab.data(), kept.data(), kept.size() * sizeof(rt::DevGlass)) == 0;
        };
        EXPECT(refused(recs.data(), n - 1));
        EXPECT(refused(recs.data(), n + 1));
        EXPECT(refused(recs.data(), -1));
        EXPECT(refused(nullptr, n));
        const rt_transmission bad[] = {{std::nan(""), 1.5}, {0.5, std::nan("")}, {0.5, INFINITY}, {-0.01, 1.5},
                                       {1.01, 1.5},         {0.5, 0.99},         {0.5, 4.01},     {0.0, 0.5}};
        for (const rt_transmission& b : bad) {
            std::vector<rt_transmission> r2 = recs;
            r2[7] = b;
            EXPECT(refused(r2.data(), n));
        }
        std::vector<rt_transmission> zeros(prims.size(), rt_transmission{0.0, 2.5});
        EXPECT(rth::pack_transmission(zeros.data(), n, sc, tab) == RT_OK && tab.empty());
        tab = kept;
        EXPECT(rth::pack_transmission(nullptr, 0, sc, tab) == RT_OK && tab.empty());
    }
    // frame AOVs: what is refused before the ctx is looked at, the buffers untouched
    EXPECT(sizeof(rt_aov_buffers) == 48);
    int32_t aov_index[2] = {7, 7};
    float aov_depth[2] = {7.f, 7.f};
    rt_aov_buffers ab{};
    ab.index = aov_index;
    ab.depth = aov_depth;
    EXPECT(rt_render_aov(nullptr, &c, 0, 1, &ab, &st) == RT_ERR_INVALID_ARG);
    EXPECT(rt_render_aov_device(nullptr, &c, 0, 1, &ab, nullptr) == RT_ERR_INVALID_ARG);
    EXPECT(aov_index[0] == 7 && aov_index[1] == 7 && aov_depth[0] == 7.f && aov_depth[1] == 7.f);

    // hit records -> Collision
    rt_hit h{};
    h.distance = 2.5;
    h.normal[0] = -1, h.normal[1] = 0.25, h.normal[2] = 0;
    h.index = 3;
    Collision col = rt_collision_from_hit(h);
    EXPECT(col.hit && col.hit_object_index == 3 && col.distance == 2.5 && col.normal.y == 0.25);
    rt_hit miss{};
    miss.distance = DBL_MAX;
    miss.index = -1;
    col = rt_collision_from_hit(miss);
    EXPECT(!col.hit && col.hit_object_index == -1 && col.distance == DBL_MAX && col.normal.x == 0);
    EXPECT(sizeof(rt_hit) == 40);

    rt_ctx* ctx = nullptr;
    const int cs = rt_ctx_create(0, &ctx);
    if (cs == RT_ERR_NO_DEVICE) {
        std::printf("no HIP device: the checks behind a ctx were not run\n");
    } else {
        EXPECT(cs == RT_OK);
        if (cs == RT_OK) {
            EXPECT(rt_trace_rays(ctx, o, d, 2, 4, RT_PREC_F64, 0, RT_OUT_RGB_F64, rgb, hits, 1, &st) ==
                   RT_ERR_NO_SCENE);
            EXPECT(rt_render_aov(ctx, &c, 0, 1, &ab, &st) == RT_ERR_NO_SCENE);
            EXPECT(rt_render_aov_device(ctx, &c, 0, 1, &ab, nullptr) == RT_ERR_NO_SCENE);
            EXPECT(rt_set_scene(ctx, prims.data(), (int32_t)prims.size()) == RT_OK);
            EXPECT(rt_trace_rays(ctx, nullptr, d, 2, 4, RT_PREC_F64, 0, RT_OUT_RGB_F64, rgb, hits, 1, &st) ==
                   RT_ERR_INVALID_ARG);
            EXPECT(rt_trace_rays(ctx, o, d, 2, 4, RT_PREC_F64, 0, RT_OUT_RGB_F64, nullptr, nullptr, 1, &st) ==
                   RT_ERR_INVALID_ARG);
            EXPECT(rt_trace_rays(ctx, o, d, -1, 4, RT_PREC_F64, 0, RT_OUT_RGB_F64, rgb, hits, 1, &st) ==
                   RT_ERR_INVALID_ARG);
            EXPECT(rt_trace_rays(ctx, o, d, 2, 4, RT_PREC_F32, 0, RT_OUT_RGB_F64, rgb, hits, 1, &st) ==
                   RT_ERR_UNSUPPORTED);
            EXPECT(rt_trace_rays(ctx, o, d, 0, 4, RT_PREC_F64, 0, RT_OUT_RGB_F64, rgb, hits, 1, &st) == RT_OK);
            EXPECT(rt_trace_rays(ctx, o, d, 2, 4, RT_PREC_F64, 0, RT_OUT_RGB_F64, rgb, hits, 1, &st) == RT_OK);
            EXPECT(hits[0].index == 1 && st.segments >= 2);
            EXPECT(rt_occluded(ctx, o, d, tmax, 2, nullptr, nullptr, &st) == RT_ERR_INVALID_ARG);
            EXPECT(rt_occluded(ctx, o, d, tmax, -1, occ, &nocc, &st) == RT_ERR_INVALID_ARG);
            EXPECT(rt_occluded(ctx, o, d, tmax, 0, occ, &nocc, &st) == RT_OK && nocc == 9);
            // ray 0 meets the sphere at parameter 1 (x = 1.5, r = .5): on the limit, blocked
            EXPECT(rt_occluded(ctx, o, d, tmax, 2, occ, &nocc, &st) == RT_OK);
            EXPECT(occ[0] == 1 && nocc == (uint64_t)(occ[0] + occ[1]) && st.segments == 2);
            EXPECT(rt_occluded(ctx, o, d, nullptr, 2, occ, nullptr, nullptr) == RT_OK && occ[0] == 1);
            // rt_set_lights: the refused arguments, the full table, back to the reference's light
            EXPECT(rt_set_lights(ctx, lights, RT_MAX_LIGHTS + 1) == RT_ERR_INVALID_ARG);
            EXPECT(rt_set_lights(ctx, lights, -1) == RT_ERR_INVALID_ARG);
            EXPECT(rt_set_lights(ctx, nullptr, 1) == RT_ERR_INVALID_ARG);
            lights[3].position[1] = std::nan("");
            EXPECT(rt_set_lights(ctx, lights, 4) == RT_ERR_INVALID_ARG);
            EXPECT(rt_set_lights(ctx, lights, 3) == RT_OK);
            lights[3].position[1] = 0;
            EXPECT(rt_set_lights(ctx, lights, RT_MAX_LIGHTS) == RT_OK);
            EXPECT(rt_trace_rays(ctx, o, d, 2, 4, RT_PREC_F64, RT_FLAG_SHADOWS, RT_OUT_RGB_F64, rgb, hits, 1,
                                 &st) == RT_OK);
            EXPECT(rt_trace_rays(ctx, o, d, 2, 4, RT_PREC_F64, RT_FLAG_SUN, RT_OUT_RGB_F64, rgb, hits, 1,
                                 &st) == RT_ERR_UNSUPPORTED);
            EXPECT(rt_set_lights(ctx, nullptr, 0) == RT_OK);
            // rt_set_transmission on the ctx: set, shade, the refusals, clear (both ways)
            EXPECT(rt_set_transmission(ctx, recs.data(), (int32_t)recs.size()) == RT_OK);
            EXPECT(rt_trace_rays(ctx, o, d, 2, 4, RT_PREC_F64, RT_FLAG_SHADOWS, RT_OUT_RGB_F64, rgb, hits, 1,
                                 &st) == RT_OK);
            EXPECT(rt_trace_rays(ctx, o, d, 2, 4, RT_PREC_F64, RT_FLAG_SUN, RT_OUT_RGB_F64, rgb, hits, 1,
                                 &st) == RT_ERR_UNSUPPORTED);
            EXPECT(rt_set_transmission(ctx, recs.data(), (int32_t)recs.size() - 1) == RT_ERR_INVALID_ARG);
            EXPECT(rt_set_transmission(ctx, nullptr, (int32_t)recs.size()) == RT_ERR_INVALID_ARG);
            {
                const std::vector<rt_transmission> zeros(recs.size(), rt_transmission{0.0, 1.0});
                EXPECT(rt_set_transmission(ctx, zeros.data(), (int32_t)zeros.size()) == RT_OK);
            }
            EXPECT(rt_trace_rays(ctx, o, d, 2, 4, RT_PREC_F64, RT_FLAG_SUN, RT_OUT_RGB_F64, rgb, hits, 1,
                                 &st) == RT_OK);
            EXPECT(rt_set_transmission(ctx, recs.data(), (int32_t)recs.size()) == RT_OK);
            EXPECT(rt_set_transmission(ctx, nullptr, 0) == RT_OK);
            // rt_render_aov: the refused arguments (statuses before any launch), then one row
            const rt_aov_buffers none{};
            rt_aov_buffers bad = ab;
            bad.reserved = aov_index;
            EXPECT(rt_render_aov(ctx, nullptr, 0, 1, &ab, &st) == RT_ERR_INVALID_ARG);
            EXPECT(rt_render_aov(ctx, &c, 0, 1, nullptr, &st) == RT_ERR_INVALID_ARG);
            EXPECT(rt_render_aov(ctx, &c, 0, 1, &none, &st) == RT_ERR_INVALID_ARG);
            EXPECT(rt_render_aov(ctx, &c, 0, 1, &bad, &st) == RT_ERR_INVALID_ARG);
            EXPECT(rt_render_aov_device(ctx, &c, 0, 1, &bad, nullptr) == RT_ERR_INVALID_ARG);
            EXPECT(rt_render_aov(ctx, &c, -1, 1, &ab, &st) == RT_ERR_OUT_OF_RANGE);
            EXPECT(rt_render_aov(ctx, &c, c.height, 1, &ab, &st) == RT_ERR_OUT_OF_RANGE);
            EXPECT(rt_render_aov(ctx, &c, 0, -1, &ab, &st) == RT_ERR_INVALID_ARG);
            EXPECT(rt_render_aov(ctx, &c, 0, 0, &ab, &st) == RT_OK && aov_index[0] == 7 && st.segments == 0);
            std::vector<int32_t> row_index(c.width, 7);
            rt_aov_buffers row{};
            row.index = row_index.data();
            EXPECT(rt_render_aov(ctx, &c, c.height / 2, 1, &row, &st) == RT_OK);
            EXPECT(st.segments == (uint64_t)c.width && row_index[0] != 7);
            rt_ctx_destroy(ctx);
        }
    }
    // the C++ mirror rejects a primitive without a GPU record before any device work
    struct Disc : SceneGeometry {
        Disc() : SceneGeometry(Material(RGB(1, 0, 0))) {}
        Collision intersect(ray) const override { return Collision(-1, vec3(0, 0, 0), false, -1); }
    };
    scene.push_back(std::make_unique<Disc>());
    bool threw = false;
    try {
        rt_closest_hits(scene, {ray(vec3(1, 0, 0), point3(0, 0, 0))});
    } catch (const std::invalid_argument&) {
        threw = true;
    }
    EXPECT(threw);
    threw = false;
    try {
        rt_occluded(scene, {ray(vec3(1, 0, 0), point3(0, 0, 0))}, {1.0});
    } catch (const std::invalid_argument&) {
        threw = true;
    }
    EXPECT(threw);
    threw = false;
    try {
        rt_scene_aov(cam.init(), scene, cam);
    } catch (const std::invalid_argument&) {
        threw = true;
    }
    EXPECT(threw);
    std::printf(g_fail ? "asan_rays: %d check(s) FAILED\n" : "asan_rays: clean\n", g_fail);
    return g_fail ? 1 : 0;
}
