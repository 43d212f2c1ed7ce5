// Check of RtSceneOptions::lights through the C++ mirror (include/rt/scene.h), host code written
// the way the reference's main.cpp drives rt_scene, linked against librt_host.so + librt_amd.so.
//   lights_main render W H F   rt_scene on the GPU, F64, depth 3, lights K2, flags = F: writes the
//                              camera rt_scene was given (12 doubles: position, image_top_left,
//                              pixel_delta_x, pixel_delta_y) and then H*W*3 doubles to stdout
//   lights_main radiance F     rt_radiance of 64 fixed rays at depth 3, lights K2, flags = F: one
//                              line per ray, every double as %a: ox oy oz dx dy dz r g b
// Scene: test_shadows_cpp's (the default scene, main.cpp:160-163, and a large sphere).  K2 is
// tests/lights_fixture.py's light set.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <memory>
#include <string>
#include <vector>

#include "rt/scene.h"

static std::vector<std::unique_ptr<SceneGeometry>> lit_scene() {
    std::vector<std::unique_ptr<SceneGeometry>> scene = {};
    scene.push_back(std::make_unique<Sphere>(Material(RGB(0, 1, 0), 0.5), point3(1.5, 0, 0), .5));
    scene.push_back(std::make_unique<Wall>(Material(RGB(0, 0, 1)), point3(3.0, 2, 0), vec3(0, -1, 0), 1, 1));
    scene.push_back(std::make_unique<Wall>(Material(RGB(0, 1, 0)), point3(3.0, -3, 0), vec3(0, 1, 0), 2, 2));
    scene.push_back(std::make_unique<Sphere>(Material(RGB(1, 0, 0), 0.25), point3(2.0, -1.5, 0.5), .6));
    return scene;
}

static std::vector<RtLight> k2() {
    return {RtLight{point3(1, -2, 2.5), RGB(1, .8, .6)}, RtLight{point3(6, 1.5, 3), RGB(.3, .5, 1)}};
}

static uint64_t g_state = 20261021;
static double U() {
    uint64_t z = (g_state += 0x9E3779B97F4A7C15ull);
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    z ^= z >> 31;
    return (double)(z >> 40) * (1.0 / 16777216.0);
}

int main(int argc, char** argv) {
    if (argc < 2) return 2;
    const std::string mode = argv[1];
    RtSceneOptions o = rt_scene_get_options();
    o.precision = RT_PREC_F64;
    o.depth = 3;
    o.lights = k2();
    auto scene = lit_scene();
    if (mode == "render" && argc >= 5) {
        const int W = std::atoi(argv[2]), H = std::atoi(argv[3]);
        o.flags = (unsigned)std::atoi(argv[4]);
        rt_scene_set_options(o);
        Camera cam;
        cam.aspect_ratio = (double)W / H;
        cam.image_width = W;
        cam.movement_speed = 0.1;
        cam.vfov = 90;
        cam.position = point3(0, 0, 0);  // main.cpp:150-151
        cam.lookat = point3(-1, 0, 0);
        cam.vup = vec3(0, 0, -1);
        auto u = cam.init();
        std::vector<std::vector<RGB>> frame_buffer(H, std::vector<RGB>(W, RGB(0, 0, 0)));
        rt_scene(u, scene, cam, frame_buffer);
        const vec3 c[4] = {cam.position, cam.image_top_left, u.at(0), u.at(1)};
        for (const vec3& v : c) {
            const double d[3] = {v.x, v.y, v.z};
            std::fwrite(d, sizeof d, 1, stdout);
        }
        for (int i = 0; i < H; i++)
            for (int j = 0; j < W; j++) {
                const double v[3] = {frame_buffer[i][j].x, frame_buffer[i][j].y, frame_buffer[i][j].z};
                std::fwrite(v, sizeof v, 1, stdout);
            }
        return 0;
    }
    if (mode == "radiance" && argc >= 3) {
        o.flags = (unsigned)std::atoi(argv[2]);
        rt_scene_set_options(o);
        std::vector<ray> rays;
        for (int k = 0; k < 64; k++) {
            const point3 org(-1 + U(), -0.5 + U(), -0.25 + 0.5 * U());
            const double s = 0.25 + 2 * U();
            const vec3 d(s * (0.5 + U()), s * (-1.4 + 2.0 * U()), s * (-0.4 + 0.8 * U()));
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
    return 2;
}
