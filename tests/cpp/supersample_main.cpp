// Check of RtSceneOptions::supersample (include/rt/scene.h), host code written the way the
// reference's main.cpp drives rt_scene, linked against librt_host.so + librt_amd.so.
//   supersample_main render W H S   rt_scene on the GPU, F64, depth 10, S x S rays per pixel:
//                                   writes the camera rt_scene was given (12 doubles: position,
//                                   image_top_left, pixel_delta_x, pixel_delta_y) and then
//                                   H*W*3 doubles to stdout
//   supersample_main tiled S N      supersample = S with N devices listed: prints "1 <what>" if
//                                   rt_scene throws std::invalid_argument (no device needed)
#include <cstdio>
#include <cstdlib>
#include <memory>
#include <stdexcept>
#include <string>
#include <vector>

#include "rt/scene.h"

static std::vector<std::unique_ptr<SceneGeometry>> default_scene() {
    std::vector<std::unique_ptr<SceneGeometry>> scene = {};
    scene.push_back(std::make_unique<Sphere>(Material(RGB(0, 1, 0), 0.5), point3(1.5, 0, 0), .5));
    scene.push_back(std::make_unique<Wall>(Material(RGB(0, 0, 1)), point3(3.0, 2, 0), vec3(0, -1, 0), 1, 1));
    scene.push_back(std::make_unique<Wall>(Material(RGB(0, 1, 0)), point3(3.0, -3, 0), vec3(0, 1, 0), 2, 2));
    return scene;
}

static Camera make_camera(int w, int h) {
    Camera cam;
    cam.aspect_ratio = (double)w / h;
    cam.image_width = w;
    cam.movement_speed = 0.1;
    cam.vfov = 90;
    cam.position = point3(0, 0, 0);
    cam.lookat = point3(-1, 0, 0);
    cam.vup = vec3(0, 0, -1);
    return cam;
}

int main(int argc, char** argv) {
    if (argc < 2) return 2;
    const std::string mode = argv[1];
    if (mode == "render" && argc >= 5) {
        const int W = std::atoi(argv[2]), H = std::atoi(argv[3]);
        RtSceneOptions o = rt_scene_get_options();
        o.precision = RT_PREC_F64;
        o.supersample = std::atoi(argv[4]);
        rt_scene_set_options(o);
        auto scene = default_scene();
        Camera cam = make_camera(W, H);
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
    if (mode == "tiled" && argc >= 4) {
        RtSceneOptions o = rt_scene_get_options();
        o.supersample = std::atoi(argv[2]);
        o.devices.assign(std::atoi(argv[3]), 0);
        o.transport = RT_TRANSPORT_COPY;
        rt_scene_set_options(o);
        auto scene = default_scene();
        Camera cam = make_camera(32, 32);
        auto u = cam.init();
        std::vector<std::vector<RGB>> frame_buffer(32, std::vector<RGB>(32, RGB(0, 0, 0)));
        try {
            rt_scene(u, scene, cam, frame_buffer);
        } catch (const std::invalid_argument& e) {
            std::printf("1 %s\n", e.what());
            return 0;
        }
        std::printf("0\n");
        return 0;
    }
    return 2;
}
