/*
 * host/rt_scene.cpp — the drop-in frame operator (main.cpp:124-139) on the GPU path.
 *
 * Same signature and observable behaviour as the reference: fills
 * frame_buffer.at(i).at(j) for every row i < image_height and column j < image_width,
 * with RGB values of recursive_ray_tracing at depth 10.  Underneath, the scene is
 * flattened through SceneGeometry::pack() and rendered by the HIP kernel through the
 * C-ABI with fp64 output (RT_OUT_RGB_F64), so the values are the fp64 path's.
 *
 * The reference has no context argument, so a process-wide renderer is created on first
 * use (device/precision from rt_scene_set_options; with several devices a row-tiled
 * rt_multi whose bands are gathered into the first); like the reference, rt_scene is
 * meant to be called from one thread.  A primitive without a GPU record (a SceneGeometry
 * subclass that does not override pack()) throws std::invalid_argument before any device
 * work.
 */
#include <cstdlib>
#include <cstring>
#include <memory>
#include <mutex>
#include <stdexcept>
#include <string>
#include <vector>

#include "../../include/rt/scene.h"

namespace {

struct Global {
    std::mutex mu;
    RtSceneOptions opts;
    rt_ctx* ctx = nullptr;
    int ctx_device = -1;
    rt_multi* multi = nullptr;       // opts.devices.size() > 1: row-tiled across GPUs
    std::vector<int> multi_devices;
    int multi_transport = -1;
    std::vector<double> staging;
    std::vector<rt_prim> uploaded;  // the scene on the device (re-uploaded only on change)
    bool uploaded_tiled = false;    // ... of the tiled (rt_multi) or the one-GPU renderer
    std::vector<rt_prim> ctx_prims;  // the scene on `ctx` itself (the ray queries always use it)
    // the transmission records in force on `ctx` / `multi` (set only on change: a set uploads a
    // table); emptied wherever the renderer or its scene is replaced, which clears the records
    std::vector<rt_transmission> ctx_glass, multi_glass;
    bool atexit_set = false;
    // no destructor: a function-static's destructor runs in an order unspecified relative
    // to the HIP and RCCL runtimes' own teardown; rt_scene_shutdown (atexit) releases
    void release() {
        if (ctx) rt_ctx_destroy(ctx);
        if (multi) rt_multi_destroy(multi);
        ctx = nullptr;
        multi = nullptr;
        ctx_device = -1;
        multi_devices.clear();
        multi_transport = -1;
        uploaded.clear();
        ctx_prims.clear();
        ctx_glass.clear();
        multi_glass.clear();
    }
};

Global& global() {
    static Global* g = new Global();  // never destroyed (see Global::release)
    return *g;
}

/* After the first renderer exists (the HIP runtime — and RCCL for a tiled renderer — is
 * initialised by then), so the handler runs before their exit-time teardown. */
void register_shutdown(Global& g) {
    if (g.atexit_set) return;
    g.atexit_set = true;
    std::atexit([] { rt_scene_shutdown(); });
}

void check(int st, rt_ctx* ctx, const char* what) {
    if (st != RT_OK)
        throw std::runtime_error(std::string(what) + ": " + rt_strerror(st) + " " +
                                 rt_last_hip_error(ctx));
}

void check_multi(int st, rt_multi* m, const char* what) {
    if (st != RT_OK)
        throw std::runtime_error(std::string(what) + ": " + rt_strerror(st) + " " +
                                 rt_multi_last_error(m));
}

/* RtSceneOptions::lights as the C-ABI's records (empty: n == 0, the reference's light). */
std::vector<rt_light> light_records(const RtSceneOptions& o) {
    std::vector<rt_light> ls(o.lights.size());
    for (size_t l = 0; l < ls.size(); l++) {
        const RtLight& s = o.lights[l];
        ls[l] = rt_light{{s.position.x, s.position.y, s.position.z}, {s.color.x, s.color.y, s.color.z}};
    }
    return ls;
}

/* RtSceneOptions::transmission in force on the one-GPU renderer (tiled == false) or the
 * row-tiled one: rt_set_transmission / rt_multi_set_transmission when the records differ from
 * those set last (an empty vector: none). */
void apply_transmission(Global& g, bool tiled) {
    std::vector<rt_transmission> want(g.opts.transmission.size());
    for (size_t j = 0; j < want.size(); j++)
        want[j] = rt_transmission{g.opts.transmission[j].transmission, g.opts.transmission[j].ior};
    std::vector<rt_transmission>& have = tiled ? g.multi_glass : g.ctx_glass;
    if (want.size() == have.size() &&
        (want.empty() || std::memcmp(want.data(), have.data(), want.size() * sizeof(rt_transmission)) == 0))
        return;
    if (tiled)
        check_multi(rt_multi_set_transmission(g.multi, want.data(), (int32_t)want.size()), g.multi,
                    "rt_multi_set_transmission");
    else
        check(rt_set_transmission(g.ctx, want.data(), (int32_t)want.size()), g.ctx, "rt_set_transmission");
    have.swap(want);
}

/* The frame's camera as the C-ABI takes it: position and image_top_left of cam, the pixel
 * deltas Camera::init returned (u), the frame size (main.cpp:124-134). */
rt_camera camera_record(const std::vector<vec3>& u, const Camera& cam) {
    rt_camera c{};
    const vec3* v[4] = {&cam.position, &cam.image_top_left, &u.at(0), &u.at(1)};
    double* dst[4] = {c.position, c.image_top_left, c.pixel_delta_x, c.pixel_delta_y};
    for (int k = 0; k < 4; k++) {
        dst[k][0] = v[k]->x;
        dst[k][1] = v[k]->y;
        dst[k][2] = v[k]->z;
    }
    c.width = (int)cam.image_width;
    c.height = (int)cam.image_height;
    return c;
}

}  // namespace

void rt_scene_shutdown() {
    Global& g = global();
    std::lock_guard<std::mutex> lk(g.mu);
    g.release();
}

void rt_scene_set_options(const RtSceneOptions& opts) {
    Global& g = global();
    std::lock_guard<std::mutex> lk(g.mu);
    g.opts = opts;
}

RtSceneOptions rt_scene_get_options() {
    Global& g = global();
    std::lock_guard<std::mutex> lk(g.mu);
    return g.opts;
}

void rt_scene(std::vector<vec3> u, const std::vector<std::unique_ptr<SceneGeometry>>& scene,
              const Camera& cam, std::vector<std::vector<RGB>>& frame_buffer) {
    Global& g = global();
    std::lock_guard<std::mutex> lk(g.mu);
    // flatten first: a primitive the GPU path does not know throws before any device work
    std::vector<rt_prim> prims(scene.size());
    for (size_t j = 0; j < scene.size(); j++) scene[j]->pack(&prims[j]);
    // several devices, or one with the loopback transport (the gather's RCCL calls on one GPU)
    const bool tiled = g.opts.devices.size() > 1 ||
                       (g.opts.devices.size() == 1 && g.opts.transport == RT_TRANSPORT_RCCL_LOOPBACK);
    // supersampling is the one-GPU renderer's (rt_multi refuses RT_OPT_SUPERSAMPLE): refused
    // here, before any device work
    const int ss = g.opts.supersample;
    if (ss != 1 && ss != 2 && ss != 4 && ss != 8)
        throw std::invalid_argument("RtSceneOptions::supersample must be 1, 2, 4 or 8");
    if (ss != 1 && tiled)
        throw std::invalid_argument("RtSceneOptions::supersample > 1 needs the one-GPU renderer");
    if (tiled && (!g.multi || g.multi_devices != g.opts.devices ||
                  g.multi_transport != g.opts.transport)) {
        if (g.multi) rt_multi_destroy(g.multi);
        g.multi = nullptr;
        const int n = (int)g.opts.devices.size();
        const int st = rt_multi_create(g.opts.devices.data(), n, n, 0, nullptr, g.opts.transport,
                                       &g.multi);
        if (st != RT_OK) throw std::runtime_error(std::string("rt_multi_create: ") + rt_strerror(st));
        g.multi_devices = g.opts.devices;
        g.multi_transport = g.opts.transport;
        g.uploaded.clear();
        g.multi_glass.clear();
    } else if (!tiled && (!g.ctx || g.ctx_device != g.opts.device)) {
        if (g.ctx) rt_ctx_destroy(g.ctx);
        g.ctx = nullptr;
        check(rt_ctx_create(g.opts.device, &g.ctx), nullptr, "rt_ctx_create");
        g.ctx_device = g.opts.device;
        g.uploaded.clear();
        g.ctx_prims.clear();
        g.ctx_glass.clear();
    }
    register_shutdown(g);
    if (tiled != g.uploaded_tiled) g.uploaded.clear();
    g.uploaded_tiled = tiled;
    // the interactive loop renders the same scene frame after frame (main.cpp:329): keep it
    // resident on the device and upload only when the packed records change
    if (g.uploaded.empty() || prims.size() != g.uploaded.size() ||
        std::memcmp(prims.data(), g.uploaded.data(), prims.size() * sizeof(rt_prim)) != 0) {
        g.uploaded.clear();
        (tiled ? g.multi_glass : g.ctx_glass).clear();  // rt_set_scene clears the records
        if (tiled)
            check_multi(rt_multi_set_scene(g.multi, prims.data(), (int32_t)prims.size()), g.multi,
                        "rt_multi_set_scene");
        else
            check(rt_set_scene(g.ctx, prims.data(), (int32_t)prims.size()), g.ctx, "rt_set_scene");
        g.uploaded = prims;
        if (!tiled) g.ctx_prims = prims;
    }

    const rt_camera c = camera_record(u, cam);
    const int W = c.width, H = c.height;
    g.staging.resize((size_t)W * H * 3);
    // (no device work: the records travel with every launch)
    const std::vector<rt_light> ls = light_records(g.opts);
    if (tiled)
        check_multi(rt_multi_set_lights(g.multi, ls.data(), (int32_t)ls.size()), g.multi,
                    "rt_multi_set_lights");
    else
        check(rt_set_lights(g.ctx, ls.data(), (int32_t)ls.size()), g.ctx, "rt_set_lights");
    apply_transmission(g, tiled);
    if (tiled)
        check_multi(rt_multi_render(g.multi, &c, g.opts.depth, g.opts.precision, g.opts.flags,
                                    RT_OUT_RGB_F64, g.staging.data(), nullptr),
                    g.multi, "rt_multi_render");
    else {
        check(rt_set_option(g.ctx, RT_OPT_SUPERSAMPLE, ss), g.ctx, "rt_set_option");
        check(rt_render(g.ctx, &c, 0, H, g.opts.depth, g.opts.precision, g.opts.flags,
                        RT_OUT_RGB_F64, g.staging.data(), 0, nullptr),
              g.ctx, "rt_render");
    }
    for (int i = 0; i < H; i++)
        for (int j = 0; j < W; j++) {
            const double* p = &g.staging[((size_t)i * W + j) * 3];
            frame_buffer.at(i).at(j) = RGB(p[0], p[1], p[2]);  // main.cpp:136 indexing
        }
}

/* ---- ray queries: find_closest_hit / recursive_ray_tracing for a batch of rays ----------
 * The one-GPU renderer of rt_scene (RtSceneOptions::device), its scene kept resident the
 * same way; a row-tiled rt_scene keeps its own renderer beside it. */
namespace {

/* Flattens the scene (throws for a primitive without a GPU record, before any device work)
 * and makes it the scene of g.ctx. */
void ray_scene(Global& g, const std::vector<std::unique_ptr<SceneGeometry>>& scene) {
    std::vector<rt_prim> prims(scene.size());
    for (size_t j = 0; j < scene.size(); j++) scene[j]->pack(&prims[j]);
    if (!g.ctx || g.ctx_device != g.opts.device) {
        if (g.ctx) rt_ctx_destroy(g.ctx);
        g.ctx = nullptr;
        g.ctx_prims.clear();
        g.ctx_glass.clear();
        if (!g.uploaded_tiled) g.uploaded.clear();
        check(rt_ctx_create(g.opts.device, &g.ctx), nullptr, "rt_ctx_create");
        g.ctx_device = g.opts.device;
    }
    register_shutdown(g);
    // ctx_prims is empty both before the first upload and after an empty scene: upload then
    if (g.ctx_prims.empty() || prims.size() != g.ctx_prims.size() ||
        std::memcmp(prims.data(), g.ctx_prims.data(), prims.size() * sizeof(rt_prim)) != 0) {
        g.ctx_prims.clear();
        g.ctx_glass.clear();  // rt_set_scene clears the records
        if (!g.uploaded_tiled) g.uploaded.clear();
        check(rt_set_scene(g.ctx, prims.data(), (int32_t)prims.size()), g.ctx, "rt_set_scene");
        g.ctx_prims = prims;
        if (!g.uploaded_tiled) g.uploaded = prims;
    }
}

void flatten_rays(const std::vector<ray>& rays, std::vector<double>& o, std::vector<double>& d) {
    o.resize(rays.size() * 3);
    d.resize(rays.size() * 3);
    for (size_t k = 0; k < rays.size(); k++) {
        const vec3 ro = rays[k].get_origin(), rd = rays[k].get_direction();
        o[3 * k] = ro.x, o[3 * k + 1] = ro.y, o[3 * k + 2] = ro.z;
        d[3 * k] = rd.x, d[3 * k + 1] = rd.y, d[3 * k + 2] = rd.z;
    }
}

}  // namespace

Collision rt_collision_from_hit(const rt_hit& h) {
    return Collision(h.distance, vec3(h.normal[0], h.normal[1], h.normal[2]), h.index >= 0,
                     (int)h.index);
}

std::vector<Collision> rt_closest_hits(const std::vector<std::unique_ptr<SceneGeometry>>& scene,
                                       const std::vector<ray>& rays) {
    Global& g = global();
    std::lock_guard<std::mutex> lk(g.mu);
    ray_scene(g, scene);
    std::vector<double> o, d;
    flatten_rays(rays, o, d);
    std::vector<rt_hit> hits(rays.size());
    // the hit record does not depend on the precision (F64 and PATH64 share the exact path)
    check(rt_trace_rays(g.ctx, o.data(), d.data(), (int64_t)rays.size(), 0, RT_PREC_F64, 0,
                        RT_OUT_RGB_F64, nullptr, hits.data(), 0, nullptr),
          g.ctx, "rt_trace_rays");
    std::vector<Collision> out;
    out.reserve(rays.size());
    for (const rt_hit& h : hits) out.push_back(rt_collision_from_hit(h));
    return out;
}

std::vector<unsigned char> rt_occluded(const std::vector<std::unique_ptr<SceneGeometry>>& scene,
                                       const std::vector<ray>& rays,
                                       const std::vector<double>& tmax) {
    if (!tmax.empty() && tmax.size() != rays.size())
        throw std::invalid_argument("rt_occluded: tmax holds neither 0 nor one limit per ray");
    Global& g = global();
    std::lock_guard<std::mutex> lk(g.mu);
    ray_scene(g, scene);
    std::vector<double> o, d;
    flatten_rays(rays, o, d);
    std::vector<unsigned char> out(rays.size());
    if (rays.empty()) return out;
    check(rt_occluded(g.ctx, o.data(), d.data(), tmax.empty() ? nullptr : tmax.data(),
                      (int64_t)rays.size(), out.data(), nullptr, nullptr),
          g.ctx, "rt_occluded");
    return out;
}

RtAov rt_scene_aov(std::vector<vec3> u, const std::vector<std::unique_ptr<SceneGeometry>>& scene,
                   const Camera& cam) {
    Global& g = global();
    std::lock_guard<std::mutex> lk(g.mu);
    ray_scene(g, scene);
    const rt_camera c = camera_record(u, cam);
    RtAov a;
    a.width = c.width;
    a.height = c.height;
    const size_t n = (size_t)(c.width > 0 ? c.width : 0) * (size_t)(c.height > 0 ? c.height : 0);
    if (n == 0) return a;
    std::vector<rt_hit> hits(n);
    a.depth.resize(n);
    a.normal.resize(n * 3);
    a.albedo.resize(n * 3);
    rt_aov_buffers b{};
    b.hit = hits.data();
    b.depth = a.depth.data();
    b.normal = a.normal.data();
    b.albedo = a.albedo.data();
    check(rt_render_aov(g.ctx, &c, 0, c.height, &b, nullptr), g.ctx, "rt_render_aov");
    a.hits.reserve(n);
    for (const rt_hit& h : hits) a.hits.push_back(rt_collision_from_hit(h));
    return a;
}

RtAo rt_scene_ao(std::vector<vec3> u, const std::vector<std::unique_ptr<SceneGeometry>>& scene,
                 const Camera& cam, const std::vector<vec3>& dirs, double radius) {
    Global& g = global();
    std::lock_guard<std::mutex> lk(g.mu);
    ray_scene(g, scene);
    const rt_camera c = camera_record(u, cam);
    RtAo a;
    a.width = c.width;
    a.height = c.height;
    const size_t n = (size_t)(c.width > 0 ? c.width : 0) * (size_t)(c.height > 0 ? c.height : 0);
    std::vector<double> w;
    w.reserve(dirs.size() * 3);
    for (const vec3& v : dirs) {
        w.push_back(v.x);
        w.push_back(v.y);
        w.push_back(v.z);
    }
    a.count.resize(n);
    a.ao.resize(n);
    rt_ao_params q{};
    q.dirs = w.data();
    q.ndirs = dirs.size() > (size_t)RT_AO_MAX_DIRS ? RT_AO_MAX_DIRS + 1 : (int32_t)dirs.size();
    q.radius = radius;
    rt_ao_buffers b{};
    b.count = a.count.data();
    b.ao = a.ao.data();
    // (an empty frame still has its arguments checked: the buffers are not read then)
    uint8_t none_c = 0;
    float none_a = 0;
    if (n == 0) {
        b.count = &none_c;
        b.ao = &none_a;
    }
    check(rt_render_ao(g.ctx, &c, 0, c.height > 0 ? c.height : 0, &q, &b, nullptr), g.ctx, "rt_render_ao");
    return a;
}

std::vector<vec3> rt_ao_direction_set(int n) {
    std::vector<double> w(n > 0 ? (size_t)n * 3 : 0);
    check(rt_ao_directions(n, w.data()), nullptr, "rt_ao_directions");
    std::vector<vec3> out;
    out.reserve((size_t)n);
    for (int k = 0; k < n; k++) out.emplace_back(w[3 * k], w[3 * k + 1], w[3 * k + 2]);
    return out;
}

std::vector<RGB> rt_radiance(const std::vector<std::unique_ptr<SceneGeometry>>& scene,
                             const std::vector<ray>& rays, int remaining_iterations) {
    Global& g = global();
    std::lock_guard<std::mutex> lk(g.mu);
    ray_scene(g, scene);
    std::vector<double> o, d;
    flatten_rays(rays, o, d);
    const int prec = g.opts.precision == RT_PREC_MIXED ? RT_PREC_F64 : g.opts.precision;
    const std::vector<rt_light> ls = light_records(g.opts);
    check(rt_set_lights(g.ctx, ls.data(), (int32_t)ls.size()), g.ctx, "rt_set_lights");
    apply_transmission(g, false);
    std::vector<double> rgb(rays.size() * 3);
    check(rt_trace_rays(g.ctx, o.data(), d.data(), (int64_t)rays.size(), remaining_iterations, prec,
                        g.opts.flags, RT_OUT_RGB_F64, rgb.data(), nullptr, 0, nullptr),
          g.ctx, "rt_trace_rays");
    std::vector<RGB> out;
    out.reserve(rays.size());
    for (size_t k = 0; k < rays.size(); k++) out.emplace_back(rgb[3 * k], rgb[3 * k + 1], rgb[3 * k + 2]);
    return out;
}
