/*
 * rt_feedback.cpp — the row feedback's device bookkeeping (RowFeedback, rt_ctx.h): which
 * frames are sampled, the cost snapshot behind a sampled frame, the order installed once it
 * has landed (rt_row_order.cpp computes it), the isolation of sampled frames, and
 * rt_tile_row_costs.  Launching thread only.
 */
#include <algorithm>
#include <cstring>
#include <vector>

#include "rt_ctx.h"

namespace rth __attribute__((visibility("hidden"))) {

namespace {

/* The grid of p's band: tile rows, and waves per tile row. */
int grid_rows(const rt::KParams& p) { return (p.nrows + rt::TILE_H - 1) / rt::TILE_H; }
int grid_waves(const rt::KParams& p) { return ((p.W + rt::TILE_W - 1) / rt::TILE_W) * (rt::BLOCK / 64); }

RowFeedback::Band band_of(const rt_ctx* ctx, const rt::KParams& p) {
    return {p.W, p.row0, p.nrows, ctx->scene_gen, ctx->rf.fb_epoch, p.tstride, p.tphase};
}

}  // namespace

int prepare_rows(rt_ctx* ctx, hipStream_t st, rt::KParams& p) {
    RowFeedback& rf = ctx->rf;
    const int gy = grid_rows(p);
    const int per_row = grid_waves(p);
    const RowFeedback::Band band = band_of(ctx, p);
    if (rf.cost_pending && hipEventQuery(rf.ev_cost) == hipSuccess) {
        rf.cost_pending = false;
        rf.iso_pending = false;  // the sampled frame has finished: nothing left to order
        const RowFeedback::Band& b = rf.cost_band;
        const int bgy = (b.nrows + rt::TILE_H - 1) / rt::TILE_H;
        const int ul = rf.cost_ul;
        const bool same = rf.fb_band == b && rf.fb_units_log2 == ul;  // keep smoothing
        rf.fb_units_log2 = ul;
        const int bnu = bgy << ul;
        order_units(rf.h_umax, rf.h_umax + bnu, bnu, rf.fb, same, rf.fb_ema);
        rf.fb_band = b;
    }
    p.row_units_log2 = 0;
    if (!rf.row_perm.empty()) {
        if ((int)rf.row_perm.size() == gy && gy <= rt::ROW_PERM_MAX) {
            p.row_perm_n = gy;
            std::memcpy(p.row_perm, rf.row_perm.data(), gy * sizeof(int16_t));
        }
    } else if (rf.feedback > 0 && !p.ss_log2 && !(p.flags & (rt::FLAG_SHADOWS | rt::FLAG_LIGHTS | rt::FLAG_GLASS)) && rf.fb_band == band &&
               !rf.fb.perm.empty()) {
        const int nu = gy << rf.fb_units_log2;
        const bool mix = ctx->row_mix == 2 || (ctx->row_mix == 1 && ctx->frames_overlap && !ctx->last_of_call);
        const std::vector<int16_t>& perm = mix && rf.fb.mix.size() == rf.fb.perm.size() ? rf.fb.mix : rf.fb.perm;
        if ((int)perm.size() == nu && nu <= rt::ROW_PERM_MAX) {
            p.row_units_log2 = rf.fb_units_log2;
            p.row_perm_n = nu;
            std::memcpy(p.row_perm, perm.data(), nu * sizeof(int16_t));
        }
    }
    // sample this frame's costs when a snapshot is due (snapshot_costs copies them)
    p.tile_cost = nullptr;
    if (rf.feedback <= 0 || !rf.row_perm.empty() || gy > rt::ROW_PERM_MAX || rf.cost_pending)
        return RT_OK;
    // supersampled, shadowed, lit (rt_set_lights) and transmissive (rt_set_transmission) frames
    // are never sampled (no stamped kernels)
    if (p.ss_log2 || (p.flags & (rt::FLAG_SHADOWS | rt::FLAG_LIGHTS | rt::FLAG_GLASS))) return RT_OK;
    if (!(rf.fb_band == band)) {
        rf.warm_left = rf.fb_warm;  // a new band or scene: the first snapshot, then the warm ones
    } else if (rf.warm_left > 0) {
        rf.warm_left--;
    } else if (++rf.since_snapshot < rf.feedback) {
        return RT_OK;
    }
    const size_t need = (size_t)gy * per_row;
    const size_t nu = (size_t)gy << units_log2(gy, per_row);
    if (need > rf.d_cost_cap || nu > rf.umax_cap) {
        // grow (rare): nothing in flight may still use the old buffers
        RT_HIP(ctx, hipStreamSynchronize(st));
        const int ws = wait_inflight(ctx);
        if (ws != RT_OK) return ws;
        if (rf.cost_pending) RT_HIP(ctx, hipEventSynchronize(rf.ev_cost));
        rf.cost_pending = false;
        const size_t cap = std::max(need, rf.d_cost_cap), ucap = std::max<size_t>({nu, rf.umax_cap, 64});
        if (rf.d_cost) RT_HIP(ctx, hipFree(rf.d_cost));
        if (rf.d_umax) RT_HIP(ctx, hipFree(rf.d_umax));
        if (rf.h_umax) RT_HIP(ctx, hipHostFree(rf.h_umax));
        rf.d_cost = nullptr;
        rf.d_umax = nullptr;
        rf.h_umax = nullptr;
        rf.d_cost_cap = 0;
        rf.umax_cap = 0;
        RT_HIP(ctx, hipMalloc(&rf.d_cost, cap * sizeof(uint16_t)));
        RT_HIP(ctx, hipMalloc(&rf.d_umax, 2 * ucap * sizeof(uint32_t)));
        RT_HIP(ctx, hipHostMalloc(&rf.h_umax, 2 * ucap * sizeof(uint32_t), hipHostMallocDefault));
        rf.d_cost_cap = cap;
        rf.umax_cap = ucap;
    }
    p.tile_cost = rf.d_cost;
    return RT_OK;
}

/* After a launch that sampled its costs (every `feedback` frames, or at once for a band the
 * order does not cover yet): copy them back behind the kernel. */
int snapshot_costs(rt_ctx* ctx, hipStream_t st, const rt::KParams& p) {
    if (!p.tile_cost) return RT_OK;
    RowFeedback& rf = ctx->rf;
    const int gy = grid_rows(p), gx = grid_waves(p);
    const int ul = units_log2(gy, gx);
    // per-unit maxima and sums on the device, then 2 nu words back (not every wave's cost)
    const int e = rt::launch_unit_max_sum(rf.d_cost, gy, gx, ul, rf.d_umax, st);
    if (e != (int)hipSuccess) return hip_fail(ctx, (hipError_t)e, "launch k_unit_max_sum");
    RT_HIP(ctx, hipMemcpyAsync(rf.h_umax, rf.d_umax, 2 * ((size_t)gy << ul) * sizeof(uint32_t),
                               hipMemcpyDeviceToHost, st));
    RT_HIP(ctx, hipEventRecord(rf.ev_cost, st));
    rf.cost_pending = true;
    rf.cost_band = band_of(ctx, p);
    rf.cost_ul = ul;
    rf.since_snapshot = 0;
    return RT_OK;
}

/* RT_OPT_ROW_FEEDBACK_ISOLATE: before a launch on `st` — a sampled frame first waits for
 * this ctx's latest frame on every other stream; any other frame whose stream has not yet
 * been ordered behind the pending sampled frame waits for it once.  Device-side waits only
 * (the host never blocks); streams are the ones launch_event tracks. */
int isolate_before(rt_ctx* ctx, hipStream_t st, bool sampled) {
    RowFeedback& rf = ctx->rf;
    if (!rf.fb_isolate) return RT_OK;
    if (sampled) {
        // (ctx->stream is not tracked: rt_render synchronises it before returning)
        for (const auto& f : ctx->inflight)
            if (f.stream != st) RT_HIP(ctx, hipStreamWaitEvent(st, f.ev, 0));
        return RT_OK;
    }
    if (!rf.iso_pending) return RT_OK;
    for (hipStream_t s : rf.iso_seen)
        if (s == st) return RT_OK;
    RT_HIP(ctx, hipStreamWaitEvent(st, rf.ev_iso, 0));
    rf.iso_seen.push_back(st);
    return RT_OK;
}
int isolate_after(rt_ctx* ctx, hipStream_t st, bool sampled) {
    RowFeedback& rf = ctx->rf;
    if (!rf.fb_isolate || !sampled) return RT_OK;
    RT_HIP(ctx, hipEventRecord(rf.ev_iso, st));
    rf.iso_pending = true;
    rf.iso_seen.assign(1, st);
    return RT_OK;
}

void feedback_release(rt_ctx* ctx) {
    RowFeedback& rf = ctx->rf;
    if (rf.ev_cost) (void)hipEventSynchronize(rf.ev_cost);
    if (rf.d_cost) (void)hipFree(rf.d_cost);
    if (rf.d_umax) (void)hipFree(rf.d_umax);
    if (rf.h_umax) (void)hipHostFree(rf.h_umax);
    if (rf.ev_cost) (void)hipEventDestroy(rf.ev_cost);
    if (rf.ev_iso) (void)hipEventDestroy(rf.ev_iso);
}

}  // namespace rth

using namespace rth;

extern "C" int rt_tile_row_costs(rt_ctx* ctx, const rt_camera* cam, int32_t depth, int32_t precision,
                                 uint32_t flags, float* costs, int32_t n) {
    const int32_t H = cam ? cam->height : 0;
    const FrameReq rq{depth, precision, flags, RT_OUT_RGB_F32};
    int st = check_render_args(ctx, cam, 0, H, rq);
    if (st != RT_OK) return st;
    if (flags & RT_FLAG_SHADOWS) return RT_ERR_UNSUPPORTED;  // no stamped shadow kernels
    if (ctx && ctx->lights.n > 0) return RT_ERR_UNSUPPORTED;  // nor stamped lights kernels
    if (ctx && ctx->d_glass) return RT_ERR_UNSUPPORTED;       // nor stamped glass kernels
    const int gy = (H + rt::TILE_H - 1) / rt::TILE_H;
    if (!costs || n != gy) return RT_ERR_INVALID_ARG;
    if (gy == 0 || cam->width == 0) {
        for (int t = 0; t < n; t++) costs[t] = 0.0f;
        return RT_OK;
    }
    DeviceGuard dg(ctx->device);
    RT_HIP(ctx, dg.err);
    const int per_row = ((cam->width + rt::TILE_W - 1) / rt::TILE_W) * (rt::BLOCK / 64);
    const size_t nw = (size_t)gy * per_row;
    const size_t out_bytes = (size_t)H * cam->width * 12;
    // scratch for this call only (the frame's pixels and every wave's cost)
    void* d_img = nullptr;
    uint16_t* d_c = nullptr;
    std::vector<uint16_t> h_c(nw);
    auto release = [&] {
        if (d_img) (void)hipFree(d_img);
        if (d_c) (void)hipFree(d_c);
    };
    hipError_t e = hipMalloc(&d_img, out_bytes);
    if (e == hipSuccess) e = hipMalloc(reinterpret_cast<void**>(&d_c), nw * sizeof(uint16_t));
    if (e == hipSuccess) e = hipMemsetAsync(d_c, 0, nw * sizeof(uint16_t), ctx->stream);
    if (e != hipSuccess) {
        release();
        return hip_fail(ctx, e, "rt_tile_row_costs buffers");
    }
    FrameOptions opt = ctx->opt;
    opt.ss_log2 = 0;  // the caller's frame as it is (rt_capi.h: RT_OPT_SUPERSAMPLE is ignored)
    rt::KParams p = make_params(FrameScene{ctx->sc, opt, ctx->d_scene, ctx->scene_gen}, &ctx->box_cache,
                                cam, 0, H, rq, d_img, nullptr);
    p.pairs = 0;        // one tile per wave: costs[t] sums tile row t's waves
    p.tile_cost = d_c;  // the stamped kernels
    const int le = rt::launch_trace(p, precision, ctx->stream);
    if (le == (int)hipSuccess) e = hipMemcpyAsync(h_c.data(), d_c, nw * sizeof(uint16_t), hipMemcpyDeviceToHost, ctx->stream);
    if (le == (int)hipSuccess && e == hipSuccess) e = hipStreamSynchronize(ctx->stream);
    release();
    if (le != (int)hipSuccess) return hip_fail(ctx, (hipError_t)le, "launch k_trace (stamped)");
    if (e != hipSuccess) return hip_fail(ctx, e, "rt_tile_row_costs copy");
    for (int t = 0; t < gy; t++) {
        double s = 0.0;
        for (int k = 0; k < per_row; k++) s += h_c[(size_t)t * per_row + k];
        costs[t] = (float)s;
    }
    return RT_OK;
}
