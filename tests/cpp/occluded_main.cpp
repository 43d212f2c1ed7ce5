// Check of the C++ mirror's occlusion query (include/rt/scene.h: rt_occluded), linked against
// librt_host.so + librt_amd.so.
//   occluded_main query    100 fixed rays on the default scene (main.cpp:160-163) with a limit
//                          each; one line per ray, every double as %a:
//                          ox oy oz dx dy dz tmax occluded
//   occluded_main plugin   a SceneGeometry subclass without a GPU record: prints "1 <what>"
//                          when the call throws std::invalid_argument (no device needed)
#include <cstdint>
#include <cstdio>
#include <limits>
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

// SplitMix64, U in [0, 1) from the top 24 bits (exact in binary, so %a round-trips trivially)
static uint64_t g_state = 20261020;
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
    if (mode == "query") {
        auto scene = default_scene();
        std::vector<ray> rays;
        std::vector<double> tmax;
        const double limits[4] = {0.5, 1.0, 3.0, std::numeric_limits<double>::infinity()};
        for (int k = 0; k < 100; k++) {
            // origins around the camera, directions into the half space of the scene (most
            // rays meet the sphere or a wall), lengths 0.25 .. 2.25 (not normalised); the
            // limits cut some of those hits off
            double u[7];
            for (double& x : u) x = U();
            const point3 o(-1 + 2 * u[0], -1 + 2 * u[1], -0.5 + u[2]);
            const double s = 0.25 + 2 * u[3];
            const vec3 d(s * (0.5 + u[4]), s * (-0.6 + 1.2 * u[5]), s * (-0.4 + 0.8 * u[6]));
            rays.push_back(ray(d, o));
            tmax.push_back(limits[k & 3]);
        }
        const std::vector<unsigned char> occ = rt_occluded(scene, rays, tmax);
        if (occ.size() != rays.size()) return 3;
        for (size_t k = 0; k < rays.size(); k++) {
            const point3 o = rays[k].get_origin();
            const vec3 d = rays[k].get_direction();
            std::printf("%a %a %a %a %a %a %a %d\n", o.x, o.y, o.z, d.x, d.y, d.z, tmax[k], (int)occ[k]);
        }
        return 0;
    }
    if (mode == "plugin") {
        auto scene = default_scene();
        scene.push_back(std::make_unique<Disc>());
        const std::vector<ray> rays = {ray(vec3(1, 0, 0), point3(0, 0, 0))};
        try {
            rt_occluded(scene, rays);
            std::printf("0\n");
        } catch (const std::invalid_argument& e) {
            std::printf("1 %s\n", e.what());
        }
        return 0;
    }
    return 2;
}
