/*
 * rt_ao.cpp — ambient occlusion frames (rt_render_ao*), kernel in rt_trace_ao.hip: the primary
 * segment of a camera's frame, then ndirs any-hit probes of the hemisphere above every hit,
 * written as the number of occluded probes and / or the open fraction per pixel.  The frame's
 * arguments are the AOV path's (primary_params, rt_aov.cpp): the colour frames' box cache and
 * the row feedback take no part.  The directions travel by value in the kernel's arguments, so
 * the caller's array is consumed before an entry point returns and a launch keeps the set it
 * was enqueued with.  rt_ao_directions is pure host code.
 */
#include <cmath>
#include <cstddef>

#include "rt_ctx.h"

using namespace rth;

namespace {

int check_ao_args(const rt_ctx* ctx, const rt_camera* cam, int32_t row0, int32_t nrows,
                  const rt_ao_params* q, const rt_ao_buffers* b) {
    if (!ctx || !cam || !q || !b) return RT_ERR_INVALID_ARG;
    if (b->reserved || q->reserved != 0 || q->reserved2) return RT_ERR_INVALID_ARG;
    if (!b->count && !b->ao) return RT_ERR_INVALID_ARG;
    if (!q->dirs || q->ndirs < 1 || q->ndirs > RT_AO_MAX_DIRS) return RT_ERR_INVALID_ARG;
    if (!(q->radius > 0)) return RT_ERR_INVALID_ARG;  // NaN too
    for (int k = 0; k < q->ndirs; k++) {
        const double* w = q->dirs + 3 * k;
        if (!std::isfinite(w[0]) || !std::isfinite(w[1]) || !std::isfinite(w[2])) return RT_ERR_INVALID_ARG;
        if (w[0] == 0 && w[1] == 0 && w[2] == 0) return RT_ERR_INVALID_ARG;
    }
    // scene and band: rt_render's checks for the same cam, row0 and nrows
    return check_render_args(ctx, cam, row0, nrows, FrameReq{0, RT_PREC_F64, 0u, RT_OUT_RGB_F32});
}

/* The launch of one band (nrows, width > 0, arguments checked, the ctx's device current). */
int launch_ao_band(rt_ctx* ctx, const rt_camera* cam, int32_t row0, int32_t nrows, const rt_ao_params& q,
                   uint8_t* d_count, float* d_ao, hipStream_t hs, hipEvent_t done) {
    const rt::KParams p = primary_params(ctx, cam, row0, nrows);
    rt::AoArgs a{};
    a.count = d_count;
    a.ao = d_ao;
    a.radius = q.radius;
    a.ndirs = q.ndirs;
    for (int k = 0; k < q.ndirs; k++)
        for (int c = 0; c < 3; c++) a.dirs[k][c] = q.dirs[3 * k + c];
    const int e = rt::launch_ao(p, a, hs, done);
    if (e != (int)hipSuccess) return hip_fail(ctx, (hipError_t)e, "launch k_ao");
    return RT_OK;
}

}  // namespace

extern "C" {

int rt_ao_directions(int32_t n, double* out) {
    if (n < 1 || n > RT_AO_MAX_DIRS || !out) return RT_ERR_INVALID_ARG;
    const double pi = 3.14159265358979323846;
    const double golden = pi * (3.0 - std::sqrt(5.0));
    for (int32_t k = 0; k < n; k++) {
        const double z = 1.0 - (double)(2 * k + 1) / (double)n;
        const double r = std::sqrt(1.0 - z * z);
        const double phi = (double)k * golden;
        out[3 * k + 0] = r * std::cos(phi);
        out[3 * k + 1] = r * std::sin(phi);
        out[3 * k + 2] = z;
    }
    return RT_OK;
}

int rt_render_ao_device(rt_ctx* ctx, const rt_camera* cam, int32_t row0, int32_t nrows,
                        const rt_ao_params* params, const rt_ao_buffers* d_out, void* stream) {
    int st = check_ao_args(ctx, cam, row0, nrows, params, d_out);
    if (st != RT_OK || nrows == 0 || cam->width == 0) return st;
    DeviceGuard dg(ctx->device);
    RT_HIP(ctx, dg.err);
    hipStream_t hs = stream ? static_cast<hipStream_t>(stream) : ctx->stream;
    hipEvent_t done = nullptr;
    st = launch_event(ctx, hs, &done);
    if (st != RT_OK) return st;
    return launch_ao_band(ctx, cam, row0, nrows, *params, d_out->count, d_out->ao, hs, done);
}

int rt_render_ao(rt_ctx* ctx, const rt_camera* cam, int32_t row0, int32_t nrows,
                 const rt_ao_params* params, const rt_ao_buffers* out, rt_stats* stats) {
    int st = check_ao_args(ctx, cam, row0, nrows, params, out);
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
    // the requested layers back to back in the ctx's output buffer (floats first: 4-byte words)
    const size_t ao_bytes = out->ao ? npx * sizeof(float) : 0;
    const size_t count_bytes = out->count ? npx : 0;
    if ((st = grow(ctx, &g.d_out, &g.d_out_cap, ao_bytes + count_bytes)) != RT_OK) return st;
    char* base = static_cast<char*>(g.d_out);
    float* d_ao = out->ao ? reinterpret_cast<float*>(base) : nullptr;
    uint8_t* d_count = out->count ? reinterpret_cast<uint8_t*>(base + ao_bytes) : nullptr;
    if ((st = staged_begin(ctx, nullptr)) != RT_OK) return st;
    st = launch_ao_band(ctx, cam, row0, nrows, *params, d_count, d_ao, ctx->stream, nullptr);
    if (st != RT_OK) return st;
    RT_HIP(ctx, hipEventRecord(g.ev1, ctx->stream));
    if (out->ao) RT_HIP(ctx, hipMemcpyAsync(out->ao, d_ao, ao_bytes, hipMemcpyDeviceToHost, ctx->stream));
    if (out->count)
        RT_HIP(ctx, hipMemcpyAsync(out->count, d_count, count_bytes, hipMemcpyDeviceToHost, ctx->stream));
    st = staged_finish(ctx, nullptr, nullptr, stats);
    if (st == RT_OK && stats) stats->segments = (uint64_t)npx;
    return st;
}

}  // extern "C"
