/*
 * rt_capi.cpp — implementation of include/rt_capi.h: the context's lifecycle (the device
 * scene, one HBM allocation in the layout of rt_device.h; a stream; the staging buffers of
 * the host-output entry points), the options, the small pure entry points and the host-only
 * diagnostics, which are thin wrappers over the pure units (rt_host.h).  The frame entry
 * points are in rt_render.cpp, the ray queries in rt_queries.cpp, the row feedback in
 * rt_feedback.cpp.  No exception crosses the boundary; every entry point returns an
 * rt_status.
 */
#include <algorithm>
#include <chrono>
#include <cmath>
#include <cstring>
#include <memory>
#include <new>
#include <vector>

#include "rt_ctx.h"

namespace rth __attribute__((visibility("hidden"))) {

int hip_fail(rt_ctx* ctx, hipError_t e, const char* what) {
    if (ctx)
        std::snprintf(ctx->last_err, sizeof ctx->last_err, "%s: %s", what, hipGetErrorString(e));
    return e == hipErrorOutOfMemory ? RT_ERR_OUT_OF_MEMORY : RT_ERR_HIP;
}

int launch_event(rt_ctx* ctx, hipStream_t st, hipEvent_t* ev) {
    *ev = nullptr;
    if (st == ctx->stream) return RT_OK;  // rt_set_scene syncs ctx->stream
    for (auto& f : ctx->inflight)
        if (f.stream == st) {
            *ev = f.ev;
            return RT_OK;
        }
    constexpr size_t kMaxStreams = 16;
    if (ctx->inflight.size() >= kMaxStreams) {
        // many distinct streams: retire the oldest entry (wait for its frame) and reuse it
        Inflight f = ctx->inflight.front();
        RT_HIP(ctx, hipEventSynchronize(f.ev));
        ctx->inflight.erase(ctx->inflight.begin());
        f.stream = st;
        ctx->inflight.push_back(f);
        *ev = f.ev;
        return RT_OK;
    }
    Inflight f{st, nullptr};
    RT_HIP(ctx, hipEventCreate(&f.ev));
    ctx->inflight.push_back(f);
    *ev = f.ev;
    return RT_OK;
}

int wait_inflight(rt_ctx* ctx) {
    if (ctx->stream) RT_HIP(ctx, hipStreamSynchronize(ctx->stream));
    for (auto& f : ctx->inflight) RT_HIP(ctx, hipEventSynchronize(f.ev));
    for (int s = 0; s < FrameTable::SLOTS; s++)  // batched launches (RT_OPT_FRAME_BATCH)
        if (ctx->tab.busy[s]) {
            RT_HIP(ctx, hipEventSynchronize(ctx->tab.ev[s]));
            ctx->tab.busy[s] = false;
        }
    return RT_OK;
}

int bytes_per_pixel(int32_t f) {
    switch (f) {
        case RT_OUT_RGB_F32: return 12;
        case RT_OUT_RGB_F64: return 24;
        case RT_OUT_RGBA8: return 4;
        case RT_OUT_RGBA8_WRAP: return 4;
        default: return 0;
    }
}

int grow(rt_ctx* ctx, void** buf, size_t* cap, size_t bytes) {
    if (bytes <= *cap) return RT_OK;
    RT_HIP(ctx, hipStreamSynchronize(ctx->stream));
    if (*buf) RT_HIP(ctx, hipFree(*buf));
    *buf = nullptr;
    *cap = 0;
    RT_HIP(ctx, hipMalloc(buf, bytes));
    *cap = bytes;
    return RT_OK;
}

int staged_begin(rt_ctx* ctx, unsigned long long* counter) {
    if (counter) RT_HIP(ctx, hipMemsetAsync(counter, 0, sizeof *counter, ctx->stream));
    RT_HIP(ctx, hipEventRecord(ctx->stg.ev0, ctx->stream));
    return RT_OK;
}

int staged_finish(rt_ctx* ctx, unsigned long long* counter, uint64_t* value, rt_stats* stats) {
    unsigned long long h = 0;
    if (counter) RT_HIP(ctx, hipMemcpyAsync(&h, counter, sizeof h, hipMemcpyDeviceToHost, ctx->stream));
    RT_HIP(ctx, hipStreamSynchronize(ctx->stream));
    if (value) *value = h;
    if (stats) {
        float ms = 0.f;
        RT_HIP(ctx, hipEventElapsedTime(&ms, ctx->stg.ev0, ctx->stg.ev1));
        stats->ms = ms;
        stats->segments = h;
    }
    return RT_OK;
}

}  // namespace rth

using namespace rth;

namespace {
/* Replaced transmission tables, once nothing in flight can read them (hipFree waits for the
 * device besides). */
void free_retired_glass(rt_ctx* ctx) {
    for (rt::DevGlass* t : ctx->glass_retired) (void)hipFree(t);
    ctx->glass_retired.clear();
}
}  // namespace

extern "C" {

int rt_capi_version(void) { return RT_CAPI_VERSION; }

const char* rt_strerror(int status) {
    switch (status) {
        case RT_OK: return "ok";
        case RT_ERR_INVALID_ARG: return "invalid argument";
        case RT_ERR_NO_DEVICE: return "no HIP device";
        case RT_ERR_HIP: return "HIP runtime error";
        case RT_ERR_OUT_OF_MEMORY: return "out of device memory";
        case RT_ERR_NO_SCENE: return "no scene uploaded";
        case RT_ERR_UNSUPPORTED: return "unsupported depth/flags";
        case RT_ERR_OUT_OF_RANGE: return "row band out of range";
        case RT_ERR_COMM: return "RCCL communication error";
        default: return "unknown status";
    }
}

const char* rt_last_hip_error(const rt_ctx* ctx) { return ctx ? ctx->last_err : ""; }

int32_t rt_out_bytes_per_pixel(int32_t out_format) { return bytes_per_pixel(out_format); }

int rt_supersample_camera(const rt_camera* cam, int32_t s, rt_camera* out) {
    return supersample_camera(cam, s, out);
}

int32_t rt_max_depth(void) { return rt::max_depth(); }

int32_t rt_tile_rows(void) { return rt::TILE_H; }

int rt_band_rows(int32_t height, int32_t nranks, int32_t rank, int32_t* row0, int32_t* nrows) {
    if (!row0 || !nrows || height < 0 || nranks <= 0 || rank < 0 || rank >= nranks)
        return RT_ERR_INVALID_ARG;
    // contiguous blocks, the first (height % nranks) ranks take one extra row
    const int32_t base = height / nranks, extra = height % nranks;
    *row0 = rank * base + (rank < extra ? rank : extra);
    *nrows = base + (rank < extra ? 1 : 0);
    return RT_OK;
}

int rt_camera_init(const double position[3], const double lookat[3], const double vup[3],
                   double vfov, double aspect_ratio, double image_width, rt_camera* cam) {
    /* Camera::init, scene.cpp:80-106, op for op (3.14 for pi kept). */
    if (!position || !lookat || !vup || !cam) return RT_ERR_INVALID_ARG;
    const hv3 pos{position[0], position[1], position[2]};
    const hv3 look{lookat[0], lookat[1], lookat[2]};
    const hv3 up{vup[0], vup[1], vup[2]};
    const double image_height = static_cast<int>(image_width / aspect_ratio);
    const hv3 pl{pos.x - look.x, pos.y - look.y, pos.z - look.z};
    const double focal_length = std::sqrt(pl.x * pl.x + pl.y * pl.y + pl.z * pl.z);
    const double theta = vfov * 3.14 / 180.0;
    const double h = std::tan(theta / 2);
    const double fov_height = 2 * h * focal_length;
    const double fov_width = fov_height * (static_cast<double>(image_width) / image_height);
    const hv3 w = hnormalize(pl);
    const hv3 u = hnormalize(hcross(up, w));
    const hv3 v = hcross(w, u);
    const hv3 fx{u.x * fov_width, u.y * fov_width, u.z * fov_width};
    const double nfh = -fov_height;
    const hv3 fy{v.x * nfh, v.y * nfh, v.z * nfh};
    const hv3 pdx{fx.x / image_width, fx.y / image_width, fx.z / image_width};
    const hv3 pdy{fy.x / image_height, fy.y / image_height, fy.z / image_height};
    const hv3 wf{w.x * focal_length, w.y * focal_length, w.z * focal_length};
    const hv3 ftl{((pos.x - wf.x) - fx.x / 2) - fy.x / 2, ((pos.y - wf.y) - fx.y / 2) - fy.y / 2,
                  ((pos.z - wf.z) - fx.z / 2) - fy.z / 2};
    const hv3 s{pdx.x + pdy.x, pdx.y + pdy.y, pdx.z + pdy.z};
    const hv3 itl{ftl.x + s.x * 0.5, ftl.y + s.y * 0.5, ftl.z + s.z * 0.5};
    const double p3[4][3] = {{pos.x, pos.y, pos.z}, {itl.x, itl.y, itl.z},
                             {pdx.x, pdx.y, pdx.z}, {pdy.x, pdy.y, pdy.z}};
    std::memcpy(cam->position, p3[0], sizeof p3[0]);
    std::memcpy(cam->image_top_left, p3[1], sizeof p3[1]);
    std::memcpy(cam->pixel_delta_x, p3[2], sizeof p3[2]);
    std::memcpy(cam->pixel_delta_y, p3[3], sizeof p3[3]);
    cam->width = static_cast<int32_t>(image_width);
    cam->height = static_cast<int32_t>(image_height);
    return RT_OK;
}

int rt_ctx_create(int device, rt_ctx** out) {
    if (!out) return RT_ERR_INVALID_ARG;
    *out = nullptr;
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess || n <= 0) return RT_ERR_NO_DEVICE;
    if (device < 0 || device >= n) return RT_ERR_NO_DEVICE;
    rt_ctx* ctx = new (std::nothrow) rt_ctx();
    if (!ctx) return RT_ERR_OUT_OF_MEMORY;
    ctx->device = device;
    int st = RT_OK;
    DeviceGuard dg(device);
    do {
        hipError_t e;
        if ((e = dg.err) != hipSuccess) { st = hip_fail(ctx, e, "hipSetDevice"); break; }
        if ((e = hipStreamCreateWithFlags(&ctx->stream, hipStreamNonBlocking)) != hipSuccess) {
            st = hip_fail(ctx, e, "hipStreamCreate"); break;
        }
        if ((e = hipEventCreate(&ctx->stg.ev0)) != hipSuccess) { st = hip_fail(ctx, e, "hipEventCreate"); break; }
        if ((e = hipEventCreate(&ctx->stg.ev1)) != hipSuccess) { st = hip_fail(ctx, e, "hipEventCreate"); break; }
        if ((e = hipEventCreateWithFlags(&ctx->rf.ev_cost, hipEventDisableTiming)) != hipSuccess) {
            st = hip_fail(ctx, e, "hipEventCreate"); break;
        }
        if ((e = hipEventCreateWithFlags(&ctx->rf.ev_iso, hipEventDisableTiming)) != hipSuccess) {
            st = hip_fail(ctx, e, "hipEventCreate"); break;
        }
        if ((e = hipMalloc(&ctx->stg.d_segs, sizeof(unsigned long long))) != hipSuccess) {
            st = hip_fail(ctx, e, "hipMalloc(segs)"); break;
        }
    } while (0);
    if (st != RT_OK) {
        rt_ctx_destroy(ctx);
        return st;
    }
    *out = ctx;
    return RT_OK;
}

int rt_ctx_destroy(rt_ctx* ctx) {
    if (!ctx) return RT_ERR_INVALID_ARG;
    render_shutdown(ctx);
    DeviceGuard dg(ctx->device);
    (void)wait_inflight(ctx);  // frames in flight on caller streams still read the scene
    for (auto& f : ctx->inflight) (void)hipEventDestroy(f.ev);
    ctx->inflight.clear();
    frame_table_release(ctx);
    if (ctx->d_scene) (void)hipFree(ctx->d_scene);
    if (ctx->d_glass) (void)hipFree(ctx->d_glass);
    free_retired_glass(ctx);
    Staging& g = ctx->stg;
    if (g.d_out) (void)hipFree(g.d_out);
    if (g.d_rays) (void)hipFree(g.d_rays);
    if (g.d_hits) (void)hipFree(g.d_hits);
    if (g.d_segs) (void)hipFree(g.d_segs);
    feedback_release(ctx);
    if (g.ev0) (void)hipEventDestroy(g.ev0);
    if (g.ev1) (void)hipEventDestroy(g.ev1);
    if (ctx->stream) (void)hipStreamDestroy(ctx->stream);
    delete ctx;
    return RT_OK;
}

int rt_set_scene(rt_ctx* ctx, const rt_prim* prims, int32_t n) {
    if (!ctx || n < 0 || (n > 0 && !prims)) return RT_ERR_INVALID_ARG;
    SceneHost sc;
    const int st = pack_scene(prims, n, sc);
    if (st != RT_OK) return st;
    DeviceGuard dg(ctx->device);
    RT_HIP(ctx, dg.err);
    // no render of the old scene may still be running, on the ctx's stream or a caller's
    const int ws = wait_inflight(ctx);
    if (ws != RT_OK) return ws;
    if (sc.total > ctx->scene_bytes) {
        if (ctx->d_scene) RT_HIP(ctx, hipFree(ctx->d_scene));
        ctx->d_scene = nullptr;
        ctx->scene_bytes = 0;
        RT_HIP(ctx, hipMalloc(&ctx->d_scene, sc.total));
        ctx->scene_bytes = sc.total;
    }
    RT_HIP(ctx, hipMemcpy(ctx->d_scene, sc.image(), sc.total, hipMemcpyHostToDevice));
    // the transmission records belonged to the old scene's objects (nothing is in flight)
    if (ctx->d_glass) ctx->glass_retired.push_back(ctx->d_glass);
    ctx->d_glass = nullptr;
    ctx->opt.glass = false;
    free_retired_glass(ctx);
    ctx->sc = std::move(sc);
    ctx->have_scene = true;
    ctx->scene_gen++;
    return RT_OK;
}

/* No device work: the records travel by value in the arguments of every later launch of the
 * lights kernels, so frames in flight keep the lights they were enqueued with. */
int rt_set_lights(rt_ctx* ctx, const rt_light* lights, int32_t n) {
    if (!ctx) return RT_ERR_INVALID_ARG;
    const int st = pack_lights(lights, n, ctx->lights);  // (leaves ctx->lights alone on failure)
    if (st != RT_OK) return st;
    ctx->opt.lights = ctx->lights.n > 0;
    return RT_OK;
}

/* The records go to a device table of their own per set (rt_ctx.h d_glass): no launch in flight
 * sees another set's records, and nothing is waited for unless many sets pile up. */
int rt_set_transmission(rt_ctx* ctx, const rt_transmission* recs, int32_t n) {
    if (!ctx) return RT_ERR_INVALID_ARG;
    if (n > 0 && !ctx->have_scene) return RT_ERR_NO_SCENE;
    std::vector<rt::DevGlass> tab;
    const int st = pack_transmission(recs, n, ctx->sc, tab);  // (nothing changes on failure)
    if (st != RT_OK) return st;
    DeviceGuard dg(ctx->device);
    RT_HIP(ctx, dg.err);
    rt::DevGlass* d_new = nullptr;
    if (!tab.empty()) {
        const size_t bytes = tab.size() * sizeof(rt::DevGlass);
        RT_HIP(ctx, hipMalloc(reinterpret_cast<void**>(&d_new), bytes));
        const hipError_t e = hipMemcpy(d_new, tab.data(), bytes, hipMemcpyHostToDevice);
        if (e != hipSuccess) {
            (void)hipFree(d_new);
            return hip_fail(ctx, e, "hipMemcpy(transmission)");
        }
    }
    if (ctx->d_glass) ctx->glass_retired.push_back(ctx->d_glass);
    ctx->d_glass = d_new;
    ctx->opt.glass = d_new != nullptr;
    if (ctx->glass_retired.size() >= 16) {
        const int ws = wait_inflight(ctx);
        if (ws != RT_OK) return ws;
        free_retired_glass(ctx);
    }
    return RT_OK;
}

/* Host-only: no ctx, no device. */
int rt_frame_boxes(const rt_prim* prims, int32_t n, const rt_camera* cam, int32_t row0,
                   int32_t nrows, int16_t* out, int32_t cap, int32_t* nbox, int32_t* mir_depth) {
    if (!cam || !nbox || !mir_depth || cap < 0 || (cap > 0 && !out)) return RT_ERR_INVALID_ARG;
    if (row0 < 0 || nrows < 0 || row0 + nrows > cam->height) return RT_ERR_OUT_OF_RANGE;
    SceneHost sc;
    const int st = pack_scene(prims, n, sc);
    if (st != RT_OK) return st;
    FrameOptions opt;
    opt.wave_cull_min = 0x7fffffff;  // as the linear-scan kernels see the scene
    std::unique_ptr<rt::KParams> p(new (std::nothrow) rt::KParams);
    if (!p) return RT_ERR_OUT_OF_MEMORY;
    *p = make_params(FrameScene{sc, opt, nullptr, 0}, nullptr, cam, row0, nrows,
                     FrameReq{0, RT_PREC_F64, 0, RT_OUT_RGB_F32}, nullptr, nullptr);
    long total = p->nbox;
    for (long L = 1, lvl = 1; L <= p->mir_depth; L++) {
        lvl *= sc.nW;
        total += lvl * p->nbox;
    }
    *nbox = p->nbox;
    *mir_depth = p->mir_depth;
    if (total > cap) return RT_ERR_INVALID_ARG;
    for (int j = 0; j < p->nbox; j++) std::memcpy(out + 4 * j, &p->box[j], sizeof(rt::PrimBox));
    for (long j = p->nbox; j < total; j++)
        std::memcpy(out + 4 * j, &p->mbox[j - p->nbox], sizeof(rt::PrimBox));
    return RT_OK;
}

int rt_set_option(rt_ctx* ctx, int32_t option, int64_t value) {
    if (!ctx) return RT_ERR_INVALID_ARG;
    FrameOptions& o = ctx->opt;
    RowFeedback& rf = ctx->rf;
    switch (option) {
        case RT_OPT_WAVE_CULL_MIN_SPHERES:
            if (value < 0) return RT_ERR_INVALID_ARG;
            o.wave_cull_min = value > 0x7fffffff ? 0x7fffffff : (int)value;
            return RT_OK;
        case RT_OPT_STATS_DEVICE_PTR:
            o.d_stats = reinterpret_cast<unsigned long long*>(static_cast<intptr_t>(value));
            return RT_OK;
        case RT_OPT_CLUSTER_COS:
            if (value < -2000 || value > 2000) return RT_ERR_INVALID_ARG;
            o.clu_cos = (float)value / 1000.0f;
            return RT_OK;
        case RT_OPT_WALL_ORDER:
            if (value != 0 && value != 1) return RT_ERR_INVALID_ARG;
            o.wall_order = value == 1;
            return RT_OK;
        case RT_OPT_EYE_TABLES:
            if (value != 0 && value != 1) return RT_ERR_INVALID_ARG;
            o.eye_tables = value == 1;
            return RT_OK;
        case RT_OPT_TILE_BINS:
            if (value != 0 && value != 1) return RT_ERR_INVALID_ARG;
            o.tile_bins = value == 1;
            return RT_OK;
        case RT_OPT_BOX_CACHE:
            if (value != 0 && value != 1) return RT_ERR_INVALID_ARG;
            o.box_cache_on = value == 1;
            return RT_OK;
        case RT_OPT_MIRROR_BINS:
            if (value != 0 && value != 1) return RT_ERR_INVALID_ARG;
            o.mirror_bins = value == 1;
            return RT_OK;
        case RT_OPT_ROW_ORDER:
            if (value != 0 && value != 1) return RT_ERR_INVALID_ARG;
            o.row_order = value == 1;
            return RT_OK;
        case RT_OPT_PIXEL_PAIRS:
            if (value != 0 && value != 1) return RT_ERR_INVALID_ARG;
            o.pixel_pairs = value == 1;
            return RT_OK;
        case RT_OPT_SUPERSAMPLE:
            if (value != 1 && value != 2 && value != 4 && value != 8) return RT_ERR_INVALID_ARG;
            o.ss_log2 = value == 8 ? 3 : (value == 4 ? 2 : (value == 2 ? 1 : 0));
            return RT_OK;
        case RT_OPT_ROW_FEEDBACK_EMA:
            if (value < 0 || value > 95) return RT_ERR_INVALID_ARG;
            rf.fb_ema = (int)value;
            return RT_OK;
        case RT_OPT_HOST_PIPELINE:
            if (value != 0 && value != 1) return RT_ERR_INVALID_ARG;
            ctx->host_pipeline = value == 1;
            return RT_OK;
        case RT_OPT_FRAME_BATCH:
            if (value < 1 || value > RT_MULTI_BATCH_MAX) return RT_ERR_INVALID_ARG;
            ctx->tab.frame_batch = (int)value;
            return RT_OK;
        case RT_OPT_ROW_FEEDBACK_ISOLATE:
            if (value != 0 && value != 1) return RT_ERR_INVALID_ARG;
            rf.fb_isolate = value == 1;
            return RT_OK;
        case RT_OPT_ROW_MIX:
            if (value < 0 || value > 2) return RT_ERR_INVALID_ARG;
            ctx->row_mix = (int)value;
            return RT_OK;
        case RT_OPT_ROW_FEEDBACK_WARM:
            if (value < 0 || value > 1000) return RT_ERR_INVALID_ARG;
            rf.fb_warm = (int)value;
            return RT_OK;
        case RT_OPT_ROW_FEEDBACK:
            if (value < 0 || value > 1000000) return RT_ERR_INVALID_ARG;
            rf.feedback = (int)value;
            rf.fb_epoch++;  // orders and snapshots taken so far belong to the old setting
            if (value == 0) {
                rf.fb.perm.clear();
                rf.fb.mix.clear();
                rf.fb_band = RowFeedback::Band{};
            }
            return RT_OK;
        default:
            return RT_ERR_INVALID_ARG;
    }
}

int rt_selftest(rt_ctx* ctx, int32_t test, uint64_t n, uint64_t seed, uint64_t* mismatches) {
    if (!ctx || !mismatches || test < 0 || test > 2) return RT_ERR_INVALID_ARG;
    DeviceGuard dg(ctx->device);
    RT_HIP(ctx, dg.err);
    unsigned long long* d_bad = ctx->stg.d_segs;
    RT_HIP(ctx, hipMemsetAsync(d_bad, 0, sizeof(unsigned long long), ctx->stream));
    const int e = rt::launch_selftest(test, n, seed, d_bad, ctx->stream);
    if (e != (int)hipSuccess) return hip_fail(ctx, (hipError_t)e, "launch k_selftest");
    unsigned long long h = 0;
    RT_HIP(ctx, hipMemcpyAsync(&h, d_bad, sizeof h, hipMemcpyDeviceToHost, ctx->stream));
    RT_HIP(ctx, hipStreamSynchronize(ctx->stream));
    *mismatches = h;
    return RT_OK;
}

/* Explicit tile-row dispatch order (a permutation of 0 .. n-1), used by renders whose grid
 * has exactly n tile rows; n == 0 clears it. */
int rt_set_row_order(rt_ctx* ctx, const int16_t* perm, int32_t n) {
    if (!ctx || n < 0 || n > rt::ROW_PERM_MAX || (n > 0 && !perm)) return RT_ERR_INVALID_ARG;
    std::vector<char> seen(n, 0);
    for (int j = 0; j < n; j++) {
        if (perm[j] < 0 || perm[j] >= n || seen[perm[j]]) return RT_ERR_INVALID_ARG;
        seen[perm[j]] = 1;
    }
    ctx->rf.row_perm.assign(perm, perm + n);
    return RT_OK;
}

/* Host-only diagnostic: the dispatch order order_units gives for these per-unit maxima and
 * sums (mode 0: heaviest first, 1: the mixed order). */
int rt_order_units(const uint32_t* unit_max, const uint32_t* unit_sum, int32_t n, int32_t mode,
                   int16_t* perm) {
    if (n < 0 || n > rt::ROW_PERM_MAX || !unit_max || !unit_sum || !perm || (mode != 0 && mode != 1))
        return RT_ERR_INVALID_ARG;
    UnitOrder o;
    order_units(unit_max, unit_sum, n, o, false, 0);
    const std::vector<int16_t>& r = mode == 1 ? o.mix : o.perm;
    std::copy(r.begin(), r.end(), perm);
    return RT_OK;
}

/* Diagnostic: k_unit_max_sum on the caller's wave costs (buffers of its own, synchronous). */
int rt_unit_costs(rt_ctx* ctx, const uint16_t* cost, int32_t gy, int32_t gx, int32_t units_log2,
                  uint32_t* unit_max, uint32_t* unit_sum) {
    if (!ctx || !cost || !unit_max || !unit_sum || gy < 1 || gy > 65535 || gx < 1 || gx > 65535 ||
        units_log2 < 0 || units_log2 > 3)
        return RT_ERR_INVALID_ARG;
    DeviceGuard dg(ctx->device);
    RT_HIP(ctx, dg.err);
    const size_t nc = (size_t)gy * gx, nu = (size_t)gy << units_log2;
    uint16_t* d_cost = nullptr;
    uint32_t* d_stat = nullptr;
    hipError_t e = hipMalloc(&d_cost, nc * sizeof(uint16_t));
    if (e == hipSuccess) e = hipMalloc(&d_stat, 2 * nu * sizeof(uint32_t));
    if (e == hipSuccess) e = hipMemcpyAsync(d_cost, cost, nc * sizeof(uint16_t), hipMemcpyHostToDevice, ctx->stream);
    if (e == hipSuccess) e = (hipError_t)rt::launch_unit_max_sum(d_cost, gy, gx, units_log2, d_stat, ctx->stream);
    if (e == hipSuccess) e = hipMemcpyAsync(unit_max, d_stat, nu * sizeof(uint32_t), hipMemcpyDeviceToHost, ctx->stream);
    if (e == hipSuccess) e = hipMemcpyAsync(unit_sum, d_stat + nu, nu * sizeof(uint32_t), hipMemcpyDeviceToHost, ctx->stream);
    const hipError_t es = hipStreamSynchronize(ctx->stream);
    if (d_cost) (void)hipFree(d_cost);
    if (d_stat) (void)hipFree(d_stat);
    RT_HIP(ctx, e);
    RT_HIP(ctx, es);
    return RT_OK;
}

#if RT_HOST_BENCH
/* Diagnostic build only (-DRT_HOST_BENCH=1, tools/host_bench.py): the per-frame host work of
 * a render, timed on the CPU with no device — out_us[0] = make_params (everything the host
 * computes per frame, with a box cache as a ctx has), [1] = frame_boxes alone, [2] = the
 * KParams value-init + copy. */
int rt_host_bench(const rt_prim* prims, int32_t n, const rt_camera* cam, int32_t row0,
                  int32_t nrows, int32_t iters, double* out_us) {
    SceneHost sc;
    const int st = pack_scene(prims, n, sc);
    if (st != RT_OK) return st;
    FrameOptions opt;
    opt.wave_cull_min = 0x7fffffff;
    const FrameScene fs{sc, opt, nullptr, 0};
    std::unique_ptr<BoxCache> bc(new BoxCache);
    std::unique_ptr<rt::KParams> p(new rt::KParams);
    using clk = std::chrono::steady_clock;
    auto us = [](clk::time_point a, clk::time_point b) {
        return std::chrono::duration<double, std::micro>(b - a).count();
    };
    volatile int sink = 0;
    auto t0 = clk::now();
    for (int k = 0; k < iters; k++) {
        *p = make_params(fs, bc.get(), cam, row0, nrows, FrameReq{4, RT_PREC_PATH64, 0, RT_OUT_RGB_F32},
                         nullptr, nullptr);
        sink += p->nbox;
    }
    auto t1 = clk::now();
    for (int k = 0; k < iters; k++) {
        frame_boxes(sc, opt, cam, row0, nrows, *p);
        sink += p->nbox;
    }
    auto t2 = clk::now();
    for (int k = 0; k < iters; k++) {
        rt::KParams q{};
        q.nbox = k;
        *p = q;
        sink += p->nbox;
    }
    auto t3 = clk::now();
    out_us[0] = us(t0, t1) / iters;
    out_us[1] = us(t1, t2) / iters;
    out_us[2] = us(t2, t3) / iters;
    (void)sink;
    return RT_OK;
}
#endif

}  // extern "C"
