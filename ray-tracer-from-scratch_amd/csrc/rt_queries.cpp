/*
 * rt_queries.cpp — caller rays: ray batches (rt_trace_rays*) and occlusion queries
 * (rt_occluded*), kernels in rt_rays.hip.  Nothing of a frame takes part: no camera, pixel
 * boxes, mirror chains, eye tables, row order or row feedback, so the box cache, the
 * feedback state and the frame-only options (RT_OPT_SUPERSAMPLE among them) are neither
 * read nor written; of the kernel arguments only scene_params' part is used.
 */
#include <cstddef>

#include "rt_ctx.h"

static_assert(sizeof(rt_hit) == sizeof(rt::DevHit) && offsetof(rt_hit, normal) == offsetof(rt::DevHit, normal) &&
                  offsetof(rt_hit, index) == offsetof(rt::DevHit, index),
              "rt_hit is the kernels' record");

using namespace rth;

namespace {

/* ---- ray batches: find_closest_hit / recursive_ray_tracing for caller rays -------------- */

int check_ray_args(const rt_ctx* ctx, const double* origins, const double* directions, int64_t n,
                   const FrameReq& rq, const void* out, const void* hits) {
    if (!ctx) return RT_ERR_INVALID_ARG;
    if (n < 0 || n > INT32_MAX) return RT_ERR_INVALID_ARG;
    if (!out && !hits) return RT_ERR_INVALID_ARG;
    if (n > 0 && (!origins || !directions)) return RT_ERR_INVALID_ARG;
    if (rq.depth < 0) return RT_ERR_INVALID_ARG;
    if (rq.precision < RT_PREC_F64 || rq.precision > RT_PREC_PATH64) return RT_ERR_INVALID_ARG;
    if (bytes_per_pixel(rq.out_format) == 0) return RT_ERR_INVALID_ARG;
    if (!ctx->have_scene) return RT_ERR_NO_SCENE;
    if (rq.depth > rt::max_depth()) return RT_ERR_UNSUPPORTED;
    if (rq.precision == RT_PREC_F32) return RT_ERR_UNSUPPORTED;  // no fp32 ray kernels yet
    return RT_OK;
}

/* The launch of one batch (n > 0, arguments checked, the ctx's device current). */
int launch_ray_batch(rt_ctx* ctx, const double* d_origins, const double* d_directions, int64_t n,
                     const FrameReq& rq, void* d_out, rt_hit* d_hits, unsigned long long* d_segs,
                     hipStream_t hs, hipEvent_t done) {
    // MIXED's contract is "output == F64": the F64 kernels serve it
    const int32_t prec = rq.precision == RT_PREC_MIXED ? RT_PREC_F64 : rq.precision;
    rt::KParams p{};
    scene_params(ctx->frame_scene(), prec, p);
    p.depth = rq.depth;
    p.flags = rq.flags;
    p.outf = rq.out_format;
    p.out = d_out;
    p.segs = d_segs;
    rt::RayArgs ra{};
    ra.org = d_origins;
    ra.dir = d_directions;
    ra.hits = reinterpret_cast<rt::DevHit*>(d_hits);
    ra.n = (int32_t)n;
    ra.shade = d_out ? 1 : 0;
    // RT_FLAG_SHADOWS: the shadow kernels (rt_rays_shadow.hip) shade; scene lights: the lights
    // kernels (rt_rays_lights.hip), with or without the flag; a hits-only call ignores both
    // transmission records: the glass kernels (rt_rays_glass.hip), lights or not
    const bool glass = d_out && ctx->d_glass;
    const bool lights = d_out && ctx->lights.n > 0;
    const bool shadows = d_out && (rq.flags & RT_FLAG_SHADOWS);
    if ((shadows || lights || glass) && (rq.flags & RT_FLAG_SUN)) return RT_ERR_UNSUPPORTED;
    const int e = glass     ? rt::launch_rays_glass(p, ra, glass_lights(ctx), rt::GlassArgs{ctx->d_glass}, prec, hs,
                                                    done)
                  : lights  ? rt::launch_rays_lights(p, ra, ctx->lights, prec, hs, done)
                  : shadows ? rt::launch_rays_shadow(p, ra, prec, hs, done)
                            : rt::launch_rays(p, ra, prec, hs, done);
    if (e != (int)hipSuccess) return hip_fail(ctx, (hipError_t)e, "launch k_rays");
    return RT_OK;
}

/* ---- occlusion queries: k_ray_occluded --------------------------------------------------- */

int check_occluded_args(const rt_ctx* ctx, const double* origins, const double* directions,
                        int64_t n, const void* out, const void* count) {
    if (!ctx) return RT_ERR_INVALID_ARG;
    if (n < 0 || n > INT32_MAX) return RT_ERR_INVALID_ARG;
    if (!out && !count) return RT_ERR_INVALID_ARG;
    if (n > 0 && (!origins || !directions)) return RT_ERR_INVALID_ARG;
    if (!ctx->have_scene) return RT_ERR_NO_SCENE;
    return RT_OK;
}

int launch_occluded_batch(rt_ctx* ctx, const double* d_origins, const double* d_directions,
                          const double* d_tmax, int64_t n, uint8_t* d_out,
                          unsigned long long* d_count, hipStream_t hs, hipEvent_t done) {
    rt::KParams p{};
    scene_params(ctx->frame_scene(), RT_PREC_F64, p);  // the fp64 kernels' cluster set
    rt::OccArgs oa{};
    oa.org = d_origins;
    oa.dir = d_directions;
    oa.tmax = d_tmax;
    oa.out = d_out;
    oa.count = d_count;
    oa.n = (int32_t)n;
    const int e = rt::launch_occluded(p, oa, hs, done);
    if (e != (int)hipSuccess) return hip_fail(ctx, (hipError_t)e, "launch k_ray_occluded");
    return RT_OK;
}

/* A host-staged call without rays: nothing runs. */
int no_rays(rt_stats* stats) {
    if (stats) {
        stats->ms = 0.0;
        stats->segments = 0;
    }
    return RT_OK;
}

}  // namespace

extern "C" {

int rt_trace_rays_device(rt_ctx* ctx, const double* d_origins, const double* d_directions,
                         int64_t n, int32_t depth, int32_t precision, uint32_t flags,
                         int32_t out_format, void* d_out, rt_hit* d_hits, uint64_t* d_segments,
                         void* stream) {
    const FrameReq rq{depth, precision, flags, out_format};
    int st = check_ray_args(ctx, d_origins, d_directions, n, rq, d_out, d_hits);
    if (st != RT_OK || n == 0) return st;
    DeviceGuard dg(ctx->device);
    RT_HIP(ctx, dg.err);
    hipStream_t hs = stream ? static_cast<hipStream_t>(stream) : ctx->stream;
    hipEvent_t done = nullptr;
    st = launch_event(ctx, hs, &done);
    if (st != RT_OK) return st;
    return launch_ray_batch(ctx, d_origins, d_directions, n, rq, d_out, d_hits,
                            reinterpret_cast<unsigned long long*>(d_segments), hs, done);
}

int rt_trace_rays(rt_ctx* ctx, const double* origins, const double* directions, int64_t n,
                  int32_t depth, int32_t precision, uint32_t flags, int32_t out_format, void* out,
                  rt_hit* hits, int32_t count_segments, rt_stats* stats) {
    const FrameReq rq{depth, precision, flags, out_format};
    int st = check_ray_args(ctx, origins, directions, n, rq, out, hits);
    if (st == RT_OK && out) st = check_shadow_flags(precision, flags, own_kernels(ctx));
    if (st != RT_OK) return st;
    if (n == 0) return no_rays(stats);
    DeviceGuard dg(ctx->device);
    RT_HIP(ctx, dg.err);
    Staging& g = ctx->stg;
    const size_t in_bytes = (size_t)n * 3 * sizeof(double);
    const size_t out_bytes = out ? (size_t)n * (size_t)bytes_per_pixel(out_format) : 0;
    const size_t hit_bytes = hits ? (size_t)n * sizeof(rt_hit) : 0;
    if ((st = grow(ctx, &g.d_rays, &g.d_rays_cap, 2 * in_bytes)) != RT_OK) return st;
    if ((st = grow(ctx, &g.d_out, &g.d_out_cap, out_bytes)) != RT_OK) return st;
    if ((st = grow(ctx, &g.d_hits, &g.d_hits_cap, hit_bytes)) != RT_OK) return st;
    double* d_o = static_cast<double*>(g.d_rays);
    double* d_d = d_o + (size_t)n * 3;
    RT_HIP(ctx, hipMemcpyAsync(d_o, origins, in_bytes, hipMemcpyHostToDevice, ctx->stream));
    RT_HIP(ctx, hipMemcpyAsync(d_d, directions, in_bytes, hipMemcpyHostToDevice, ctx->stream));
    unsigned long long* segs = count_segments ? g.d_segs : nullptr;
    if ((st = staged_begin(ctx, segs)) != RT_OK) return st;
    st = launch_ray_batch(ctx, d_o, d_d, n, rq, out ? g.d_out : nullptr,
                          hits ? static_cast<rt_hit*>(g.d_hits) : nullptr, segs, ctx->stream, nullptr);
    if (st != RT_OK) return st;
    RT_HIP(ctx, hipEventRecord(g.ev1, ctx->stream));
    if (out) RT_HIP(ctx, hipMemcpyAsync(out, g.d_out, out_bytes, hipMemcpyDeviceToHost, ctx->stream));
    if (hits) RT_HIP(ctx, hipMemcpyAsync(hits, g.d_hits, hit_bytes, hipMemcpyDeviceToHost, ctx->stream));
    return staged_finish(ctx, segs, nullptr, stats);
}

int rt_occluded_device(rt_ctx* ctx, const double* d_origins, const double* d_directions,
                       const double* d_tmax, int64_t n, uint8_t* d_out, uint64_t* d_count,
                       void* stream) {
    int st = check_occluded_args(ctx, d_origins, d_directions, n, d_out, d_count);
    if (st != RT_OK || n == 0) return st;
    DeviceGuard dg(ctx->device);
    RT_HIP(ctx, dg.err);
    hipStream_t hs = stream ? static_cast<hipStream_t>(stream) : ctx->stream;
    hipEvent_t done = nullptr;
    st = launch_event(ctx, hs, &done);
    if (st != RT_OK) return st;
    return launch_occluded_batch(ctx, d_origins, d_directions, d_tmax, n, d_out,
                                 reinterpret_cast<unsigned long long*>(d_count), hs, done);
}

int rt_occluded(rt_ctx* ctx, const double* origins, const double* directions, const double* tmax,
                int64_t n, uint8_t* out, uint64_t* count, rt_stats* stats) {
    int st = check_occluded_args(ctx, origins, directions, n, out, count);
    if (st != RT_OK) return st;
    if (n == 0) return no_rays(stats);
    DeviceGuard dg(ctx->device);
    RT_HIP(ctx, dg.err);
    Staging& g = ctx->stg;
    const size_t in_bytes = (size_t)n * 3 * sizeof(double);
    const size_t t_bytes = tmax ? (size_t)n * sizeof(double) : 0;
    if ((st = grow(ctx, &g.d_rays, &g.d_rays_cap, 2 * in_bytes + t_bytes)) != RT_OK) return st;
    if ((st = grow(ctx, &g.d_hits, &g.d_hits_cap, out ? (size_t)n : 0)) != RT_OK) return st;
    double* d_o = static_cast<double*>(g.d_rays);
    double* d_d = d_o + (size_t)n * 3;
    double* d_t = tmax ? d_d + (size_t)n * 3 : nullptr;
    RT_HIP(ctx, hipMemcpyAsync(d_o, origins, in_bytes, hipMemcpyHostToDevice, ctx->stream));
    RT_HIP(ctx, hipMemcpyAsync(d_d, directions, in_bytes, hipMemcpyHostToDevice, ctx->stream));
    if (tmax) RT_HIP(ctx, hipMemcpyAsync(d_t, tmax, t_bytes, hipMemcpyHostToDevice, ctx->stream));
    unsigned long long* d_cnt = count ? g.d_segs : nullptr;
    if ((st = staged_begin(ctx, d_cnt)) != RT_OK) return st;
    st = launch_occluded_batch(ctx, d_o, d_d, d_t, n, out ? static_cast<uint8_t*>(g.d_hits) : nullptr,
                               d_cnt, ctx->stream, nullptr);
    if (st != RT_OK) return st;
    RT_HIP(ctx, hipEventRecord(g.ev1, ctx->stream));
    if (out) RT_HIP(ctx, hipMemcpyAsync(out, g.d_hits, (size_t)n, hipMemcpyDeviceToHost, ctx->stream));
    st = staged_finish(ctx, d_cnt, count, stats);
    if (st == RT_OK && stats) stats->segments = (uint64_t)n;
    return st;
}

}  // extern "C"
