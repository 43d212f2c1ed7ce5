// Check of RtSceneOptions::transmission through the C++ mirror (include/rt/scene.h), host code
// written the way the reference's main.cpp drives rt_scene, linked against librt_host.so +
// librt_amd.so.
//   glass_main render W H F   rt_scene on the GPU, F64, depth 3, scene G's records, flags = F:
//                             writes the camera rt_scene was given (12 doubles: position,
//                             image_top_left, pixel_delta_x, pixel_delta_y), then H*W*3 doubles of
//                             the frame, then the H*W*3 doubles of a second rt_scene call with the
//                             records taken away again
//   glass_main radiance F     rt_radiance of 64 fixed rays at depth 3 with the records, flags = F:
//                             one line per ray, every double as %a: ox oy oz dx dy dz r g b
//   glass_main mismatch       one record too few: rt_scene must throw (exit status 0 if it did)
// Scene G and its records are tests/glass_fixture.py's.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <memory>
#include <stdexcept>
#include <string>
#include <vector>

#include "rt/scene.h"

static Material mat(RGB c, double metallic) { return Material(c, metallic); }

static std::vector<std::unique_ptr<SceneGeometry>> scene_g() {
    std::vector<std::unique_ptr<SceneGeometry>> s = {};
    s.push_back(std::make_unique<Sphere>(mat(RGB(.9, .95, 1), .3), point3(2.0, -.5, 0), 1.0));
    s.push_back(std::make_unique<Sphere>(mat(RGB(.6, 1, .7), .5), point3(1.6, 1.0, .3), .5));
    s.push_back(std::make_unique<Sphere>(mat(RGB(1, .3, .2), .6), point3(6, -1, .5), .8));
    s.push_back(std::make_unique<Sphere>(mat(RGB(.2, .4, 1), .2), point3(5.5, 1.5, -.3), .6));
    s.push_back(std::make_unique<Sphere>(mat(RGB(1, .9, .2), 0.0), point3(7, .3, 1.2), .5));
    s.push_back(std::make_unique<Wall>(Material(RGB(.7, .7, .7)), point3(3, 4, -1), vec3(0, -1, 0), 8, 4));
    s.push_back(std::make_unique<Wall>(Material(RGB(.5, .5, .5)), point3(3, -4, -1), vec3(0, 1, 0), 8, 4));
    s.push_back(std::make_unique<Wall>(Material(RGB(.4, .4, .4)), point3(10, -4, -1), vec3(-1, 0, 0), 8, 4));
    s.push_back(std::make_unique<Wall>(Material(RGB(.8, .9, 1)), point3(1.0, .3, -.8), vec3(-1, 0, 0), 1.5, 1.5));
    return s;
}

static std::vector<RtTransmission> trans_g() {
    std::vector<RtTransmission> t(9);
    t[0] = RtTransmission{.9, 1.5};
    t[1] = RtTransmission{.7, 1.33};
    t[8] = RtTransmission{.6, 1};
    return t;
}

static uint64_t g_state = 20261021;
static double U() {
    uint64_t z = (g_state += 0x9E3779B97F4A7C15ull);
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    z ^= z >> 31;
    return (double)(z >> 40) * (1.0 / 16777216.0);
}

static void write_frame(const std::vector<std::vector<RGB>>& fb, int W, int H) {
    for (int i = 0; i < H; i++)
        for (int j = 0; j < W; j++) {
            const double v[3] = {fb[i][j].x, fb[i][j].y, fb[i][j].z};
            std::fwrite(v, sizeof v, 1, stdout);
        }
}

int main(int argc, char** argv) {
    if (argc < 2) return 2;
    const std::string mode = argv[1];
    RtSceneOptions o = rt_scene_get_options();
    o.precision = RT_PREC_F64;
    o.depth = 3;
    o.transmission = trans_g();
    auto scene = scene_g();
    Camera cam;
    auto init_camera = [&](int W, int H) {
        cam.aspect_ratio = (double)W / H;
        cam.image_width = W;
        cam.movement_speed = 0.1;
        cam.vfov = 90;
        cam.position = point3(0, 0, 0);  // main.cpp:150-151
        cam.lookat = point3(-1, 0, 0);
        cam.vup = vec3(0, 0, -1);
        return cam.init();
    };
    if (mode == "render" && argc >= 5) {
        const int W = std::atoi(argv[2]), H = std::atoi(argv[3]);
        o.flags = (unsigned)std::atoi(argv[4]);
        rt_scene_set_options(o);
        auto u = init_camera(W, H);
        std::vector<std::vector<RGB>> frame_buffer(H, std::vector<RGB>(W, RGB(0, 0, 0)));
        rt_scene(u, scene, cam, frame_buffer);
        rt_scene(u, scene, cam, frame_buffer);  // (the records stay in force frame after frame)
        const vec3 c[4] = {cam.position, cam.image_top_left, u.at(0), u.at(1)};
        for (const vec3& v : c) {
            const double d[3] = {v.x, v.y, v.z};
            std::fwrite(d, sizeof d, 1, stdout);
        }
        write_frame(frame_buffer, W, H);
        o.transmission.clear();
        rt_scene_set_options(o);
        rt_scene(u, scene, cam, frame_buffer);
        write_frame(frame_buffer, W, H);
        return 0;
    }
    if (mode == "radiance" && argc >= 3) {
        o.flags = (unsigned)std::atoi(argv[2]);
        rt_scene_set_options(o);
        std::vector<ray> rays;
        for (int k = 0; k < 64; k++) {
            const point3 org(-1 + U(), -0.5 + U(), -0.25 + 0.5 * U());
            const double s = 0.25 + 2 * U();
            const vec3 d(s * (0.5 + U()), s * (-1.0 + 2.0 * U()), s * (-0.4 + 0.8 * U()));
            rays.push_back(ray(d, org));
        }
        const std::vector<RGB> rgb = rt_radiance(scene, rays, 3);
        if (rgb.size() != rays.size()) return 3;
        for (size_t k = 0; k < rays.size(); k++) {
            const point3 p = rays[k].get_origin();
            const vec3 d = rays[k].get_direction();
            std::printf("%a %a %a %a %a %a %a %a %a\n", p.x, p.y, p.z, d.x, d.y, d.z, rgb[k].x,
                        rgb[k].y, rgb[k].z);
        }
        return 0;
    }
    if (mode == "mismatch") {
        o.transmission.pop_back();
        rt_scene_set_options(o);
        auto u = init_camera(16, 8);
        std::vector<std::vector<RGB>> frame_buffer(8, std::vector<RGB>(16, RGB(0, 0, 0)));
        try {
            rt_scene(u, scene, cam, frame_buffer);
        } catch (const std::runtime_error&) {
            return 0;
        }
        return 4;
    }
    return 2;
}
