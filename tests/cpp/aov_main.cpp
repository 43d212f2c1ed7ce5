// Check of the C++ mirror's frame AOVs (include/rt/scene.h: rt_scene_aov), linked against
// librt_host.so + librt_amd.so.
//   aov_main frame     the default scene (main.cpp:160-163) from main.cpp:146-153's camera at
//                      16 x 12.  First line: the camera, every double as %a, then the size:
//                        px py pz  tlx tly tlz  dxx dxy dxz  dyx dyy dyz  width height
//                      then one line per pixel, row-major, every value as %a (floats widen
//                      exactly):
//                        index distance nx ny nz  depth  n0 n1 n2  a0 a1 a2
//   aov_main plugin    a SceneGeometry subclass without a GPU record: prints "1 <what>" when
//                      the call throws std::invalid_argument (no device needed)
#include <cstdio>
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
    if (mode == "frame") {
        auto scene = default_scene();
        Camera cam = small_camera();
        const std::vector<vec3> u = cam.init();
        const RtAov a = rt_scene_aov(u, scene, cam);
        const size_t n = (size_t)a.width * a.height;
        if (a.hits.size() != n || a.depth.size() != n || a.normal.size() != 3 * n || a.albedo.size() != 3 * n)
            return 3;
        const vec3 v[4] = {cam.position, cam.image_top_left, u.at(0), u.at(1)};
        for (const vec3& w : v) std::printf("%a %a %a ", w.x, w.y, w.z);
        std::printf("%d %d\n", a.width, a.height);
        for (size_t k = 0; k < n; k++) {
            const Collision& c = a.hits[k];
            std::printf("%d %a %a %a %a %a %a %a %a %a %a %a\n", c.hit_object_index, c.distance, c.normal.x,
                        c.normal.y, c.normal.z, (double)a.depth[k], (double)a.normal[3 * k],
                        (double)a.normal[3 * k + 1], (double)a.normal[3 * k + 2], (double)a.albedo[3 * k],
                        (double)a.albedo[3 * k + 1], (double)a.albedo[3 * k + 2]);
        }
        return 0;
    }
    if (mode == "plugin") {
        auto scene = default_scene();
        scene.push_back(std::make_unique<Disc>());
        Camera cam = small_camera();
        try {
            rt_scene_aov(cam.init(), scene, cam);
            std::printf("0\n");
        } catch (const std::invalid_argument& e) {
            std::printf("1 %s\n", e.what());
        }
        return 0;
    }
    return 2;
}
