// Check of the C++ mirror's ambient occlusion frames (include/rt/scene.h: rt_scene_ao), linked
// against librt_host.so + librt_amd.so.
//   ao_main frame K R  the default scene (main.cpp:160-163) from main.cpp:146-153's camera at
//                      16 x 12, the K directions of rt_ao_direction_set, radius R ("inf" allowed).
//                      First line: the camera, every double as %a, then the size:
//                        px py pz  tlx tly tlz  dxx dxy dxz  dyx dyy dyz  width height
//                      then K lines "wx wy wz" (%a), then one line per pixel, row-major:
//                        count ao(%a, the float widened exactly)
//   ao_main refuse     invalid probes: prints one line "1 <what>" per case that throws
//                      std::runtime_error or std::invalid_argument before any device work
//                      (no directions, 65 directions, a zero direction, radius 0; a
//                      SceneGeometry subclass without a GPU record)
#include <cmath>
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

class Disc : public SceneGeometry {
public:
    Disc() : SceneGeometry(Material(RGB(1, 0, 0))) {}
    Collision intersect(ray) const override { return Collision(-1, vec3(0, 0, 0), false, -1); }
};

static Camera small_camera() {
    Camera cam;
    cam.aspect_ratio = 16.0 / 12;
    cam.image_width = 16;
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
    if (mode == "frame" && argc == 4) {
        auto scene = default_scene();
        Camera cam = small_camera();
        const std::vector<vec3> u = cam.init();
        const std::vector<vec3> dirs = rt_ao_direction_set(std::atoi(argv[2]));
        const double radius = std::string(argv[3]) == "inf" ? INFINITY : std::atof(argv[3]);
        const RtAo a = rt_scene_ao(u, scene, cam, dirs, radius);
        const size_t n = (size_t)a.width * a.height;
        if (a.count.size() != n || a.ao.size() != n) return 3;
        const vec3 v[4] = {cam.position, cam.image_top_left, u.at(0), u.at(1)};
        for (const vec3& w : v) std::printf("%a %a %a ", w.x, w.y, w.z);
        std::printf("%d %d\n", a.width, a.height);
        for (const vec3& w : dirs) std::printf("%a %a %a\n", w.x, w.y, w.z);
        for (size_t k = 0; k < n; k++) std::printf("%d %a\n", (int)a.count[k], (double)a.ao[k]);
        return 0;
    }
    if (mode == "refuse") {
        Camera cam = small_camera();
        const std::vector<vec3> u = cam.init();
        const std::vector<vec3> four = rt_ao_direction_set(4);
        std::vector<vec3> zero = four;
        zero[2] = vec3(0, 0, 0);
        struct Case {
            std::vector<vec3> dirs;
            double radius;
            bool disc;
        };
        const Case cases[] = {{{}, 1.0, false},
                              {std::vector<vec3>(65, vec3(1, 0, 0)), 1.0, false},
                              {zero, 1.0, false},
                              {four, 0.0, false},
                              {four, 1.0, true}};
        for (const Case& c : cases) {
            auto scene = default_scene();
            if (c.disc) scene.push_back(std::make_unique<Disc>());
            try {
                rt_scene_ao(u, scene, cam, c.dirs, c.radius);
                std::printf("0\n");
            } catch (const std::invalid_argument& e) {
                std::printf("1 invalid_argument %s\n", e.what());
            } catch (const std::runtime_error& e) {
                std::printf("1 runtime_error %s\n", e.what());
            }
        }
        try {
            rt_ao_direction_set(65);
            std::printf("0\n");
        } catch (const std::runtime_error& e) {
            std::printf("1 runtime_error %s\n", e.what());
        }
        return 0;
    }
    return 2;
}
