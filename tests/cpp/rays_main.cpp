// Check of the C++ mirror's batch ray queries (include/rt/scene.h: rt_closest_hits,
// rt_radiance), written the way a host of the reference calls find_closest_hit and
// recursive_ray_tracing (main.cpp:67-119), linked against librt_host.so + librt_amd.so.
//   rays_main trace [depth]   100 fixed rays on the default scene (main.cpp:160-163) through
//                             both calls; one line per ray, every double as %a:
//                             ox oy oz dx dy dz index hit distance nx ny nz r g b
//   rays_main plugin          a SceneGeometry subclass without a GPU record: prints "1 <what>"
//                             for each of the two calls that throws std::invalid_argument
//                             (no device needed)
#include <cstdint>
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
    if (mode == "trace") {
        const int depth = argc >= 3 ? std::atoi(argv[2]) : 10;
        auto scene = default_scene();
        std::vector<ray> rays;
        for (int k = 0; k < 100; k++) {
            // origins around the camera, directions into the half space of the scene (most
            // rays meet the sphere or a wall), lengths 0.25 .. 2.25 (not normalised)
            const point3 o(-1 + 2 * U(), -1 + 2 * U(), -0.5 + U());
            const double s = 0.25 + 2 * U();
            const vec3 d(s * (0.5 + U()), s * (-1.2 + 2.4 * U()), s * (-0.4 + 0.8 * U()));
            rays.push_back(ray(d, o));
        }
        const std::vector<Collision> hits = rt_closest_hits(scene, rays);
        const std::vector<RGB> rgb = rt_radiance(scene, rays, depth);
        if (hits.size() != rays.size() || rgb.size() != rays.size()) return 3;
        for (size_t k = 0; k < rays.size(); k++) {
            const point3 o = rays[k].get_origin();
            const vec3 d = rays[k].get_direction();
            const Collision& c = hits[k];
            std::printf("%a %a %a %a %a %a %d %d %a %a %a %a %a %a %a\n", o.x, o.y, o.z, d.x, d.y, d.z,
                        c.hit_object_index, (int)c.hit, c.distance, c.normal.x, c.normal.y, c.normal.z,
                        rgb[k].x, rgb[k].y, rgb[k].z);
        }
        return 0;
    }
    if (mode == "plugin") {
        auto scene = default_scene();
        scene.push_back(std::make_unique<Disc>());
        const std::vector<ray> rays = {ray(vec3(1, 0, 0), point3(0, 0, 0))};
        try {
            rt_closest_hits(scene, rays);
            std::printf("0\n");
        } catch (const std::invalid_argument& e) {
            std::printf("1 %s\n", e.what());
        }
        try {
            rt_radiance(scene, rays);
            std::printf("0\n");
        } catch (const std::invalid_argument& e) {
            std::printf("1 %s\n", e.what());
        }
        return 0;
    }
    return 2;
}
