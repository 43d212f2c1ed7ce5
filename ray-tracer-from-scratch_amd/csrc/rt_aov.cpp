/*
 * rt_aov.cpp — frame AOVs (rt_render_aov*), kernel in rt_trace_aov.hip: the primary segment of
 * a camera's frame, written as per-pixel layers (hit record, index, depth, normal, albedo).
 * The frame's arguments come from make_params like a colour frame's — camera, band, eye tables,
 * wall order, primary pixel boxes — with the options that have no meaning here switched off (no
 * supersampling, lights, pixel pairs or mirror chains) and a box cache of its own, so the colour
 * frames' cache is neither read nor written.  Nothing of the row feedback takes part: no
 * prepare_rows, no cost snapshot, no explicit or measured order.
 */
#include <cstddef>

#include "rt_ctx.h"

using namespace rth;

namespace {

constexpr size_t kLayerBytes[5] = {sizeof(rt_hit), sizeof(int32_t), sizeof(float), 3 * sizeof(float),
                                   3 * sizeof(float)};

int check_aov_args(const rt_ctx* ctx, const rt_camera* cam, int32_t row0, int32_t nrows,
                   const rt_aov_buffers* b) {
    if (!ctx || !cam || !b) return RT_ERR_INVALID_ARG;
    if (b->reserved) return RT_ERR_INVALID_ARG;
    if (!b->hit && !b->index && !b->depth && !b->normal && !b->albedo) return RT_ERR_INVALID_ARG;
    // scene and band: rt_render's checks for the same cam, row0 and nrows
    return check_render_args(ctx, cam, row0, nrows, FrameReq{0, RT_PREC_F64, 0u, RT_OUT_RGB_F32});
}

/* The launch of one band (nrows, width > 0, arguments checked, the ctx's device current). */
int launch_aov_band(rt_ctx* ctx, const rt_camera* cam, int32_t row0, int32_t nrows,
                    const rt_aov_buffers& d, hipStream_t hs, hipEvent_t done) {
    const rt::KParams p = primary_params(ctx, cam, row0, nrows);
    rt::AovArgs a{};
    a.hit = reinterpret_cast<rt::DevHit*>(d.hit);
    a.index = d.index;
    a.depth = d.depth;
    a.normal = d.normal;
    a.albedo = d.albedo;
    const int e = rt::launch_aov(p, a, hs, done);
    if (e != (int)hipSuccess) return hip_fail(ctx, (hipError_t)e, "launch k_aov");
    return RT_OK;
}

}  // namespace

namespace rth {

rt::KParams primary_params(rt_ctx* ctx, const rt_camera* cam, int32_t row0, int32_t nrows) {
    FrameOptions opt = ctx->opt;
    opt.ss_log2 = 0;
    opt.lights = false;
    opt.glass = false;
    opt.pixel_pairs = false;
    opt.mirror_bins = false;  // the primary boxes only
    const FrameReq rq{0, RT_PREC_F64, 0u, RT_OUT_RGB_F32};
    return make_params(FrameScene{ctx->sc, opt, ctx->d_scene, ctx->scene_gen}, &ctx->aov_box_cache, cam,
                       row0, nrows, rq, nullptr, nullptr);
}

}  // namespace rth

extern "C" {

int rt_render_aov_device(rt_ctx* ctx, const rt_camera* cam, int32_t row0, int32_t nrows,
                         const rt_aov_buffers* d_out, void* stream) {
    int st = check_aov_args(ctx, cam, row0, nrows, d_out);
    if (st != RT_OK || nrows == 0 || cam->width == 0) return st;
    DeviceGuard dg(ctx->device);
    RT_HIP(ctx, dg.err);
    hipStream_t hs = stream ? static_cast<hipStream_t>(stream) : ctx->stream;
    hipEvent_t done = nullptr;
    st = launch_event(ctx, hs, &done);
    if (st != RT_OK) return st;
    return launch_aov_band(ctx, cam, row0, nrows, *d_out, hs, done);
}

int rt_render_aov(rt_ctx* ctx, const rt_camera* cam, int32_t row0, int32_t nrows,
                  const rt_aov_buffers* out, rt_stats* stats) {
    int st = check_aov_args(ctx, cam, row0, nrows, out);
    if (st != RT_OK) return st;
    const size_t npx = (size_t)nrows * (size_t)cam->width;
    if (npx == 0) {
        if (stats) {
            stats->ms = 0.0;
            stats->segments = 0;
        }
        return RT_OK;
    }
    DeviceGuard dg(ctx->device);
    RT_HIP(ctx, dg.err);
    Staging& g = ctx->stg;
    // the requested layers back to back in the ctx's output buffer (records first: 8-byte words)
    void* const host[5] = {out->hit, out->index, out->depth, out->normal, out->albedo};
    size_t off[5], total = 0;
    for (int k = 0; k < 5; k++) {
        off[k] = total;
        if (host[k]) total += npx * kLayerBytes[k];
    }
    if ((st = grow(ctx, &g.d_out, &g.d_out_cap, total)) != RT_OK) return st;
    char* base = static_cast<char*>(g.d_out);
    auto dev = [&](int k) -> void* { return host[k] ? base + off[k] : nullptr; };
    rt_aov_buffers d{};
    d.hit = static_cast<rt_hit*>(dev(0));
    d.index = static_cast<int32_t*>(dev(1));
    d.depth = static_cast<float*>(dev(2));
    d.normal = static_cast<float*>(dev(3));
    d.albedo = static_cast<float*>(dev(4));
    if ((st = staged_begin(ctx, nullptr)) != RT_OK) return st;
    st = launch_aov_band(ctx, cam, row0, nrows, d, ctx->stream, nullptr);
    if (st != RT_OK) return st;
    RT_HIP(ctx, hipEventRecord(g.ev1, ctx->stream));
    for (int k = 0; k < 5; k++)
        if (host[k])
            RT_HIP(ctx, hipMemcpyAsync(host[k], base + off[k], npx * kLayerBytes[k], hipMemcpyDeviceToHost,
                                       ctx->stream));
    st = staged_finish(ctx, nullptr, nullptr, stats);
    if (st == RT_OK && stats) stats->segments = (uint64_t)npx;
    return st;
}

}  // extern "C"
