/*
 * rt_ctx.h — struct rt_ctx and what the HIP-runtime host units share (internal; not ABI).
 *
 *   rt_capi.cpp      context lifecycle, scene upload, options, the small pure entry points
 *   rt_feedback.cpp  the row feedback's device bookkeeping (RowFeedback)
 *   rt_render.cpp    the frame entry points, the helper thread, the frame table
 *   rt_queries.cpp   ray batches and occlusion queries
 *   rt_aov.cpp       frame AOVs (the primary hits' layers)
 *   rt_ao.cpp        ambient occlusion frames (probes at the primary hits)
 *
 * A ctx belongs to one caller thread at a time (rt_capi.h).  The only other thread is
 * rt_render.cpp's helper (RT_OPT_HOST_PIPELINE), alive inside rt_render_device_frames: it
 * reads the SceneHost, the FrameOptions, d_scene and scene_gen, and reads and writes the
 * BoxCache, which the launching thread leaves alone while a batch runs.  Everything else —
 * RowFeedback, FrameTable, Staging, the in-flight list — is the launching thread's.
 */
#ifndef RT_CTX_H
#define RT_CTX_H

#include <hip/hip_runtime.h>

#include <cstdio>
#include <vector>

#include "rt_host.h"

#ifndef RT_ROW_MIX_DEFAULT      // build-time default of RT_OPT_ROW_MIX (A/B builds)
#define RT_ROW_MIX_DEFAULT 1
#endif

namespace rth __attribute__((visibility("hidden"))) {

/* Row feedback (RT_OPT_ROW_FEEDBACK): every render records each wave's cost
 * (KParams::tile_cost); every `feedback` frames a snapshot is copied to pinned host
 * memory behind the kernel and, once it has landed, the tile rows are ordered by their
 * most expensive tile (heaviest first) for the following renders of the same band.
 * Only the dispatch order changes: every tile is traced once per frame either way.
 * Launching thread only (rt_feedback.cpp; rt_set_option and rt_set_row_order write the
 * settings). */
struct RowFeedback {
    std::vector<int16_t> row_perm;  // rt_set_row_order: explicit tile-row dispatch order
    int feedback = 32;             // refresh interval in frames, 0 = off
    uint16_t* d_cost = nullptr;    // device, d_cost_cap entries (one per wave)
    size_t d_cost_cap = 0;
    uint32_t* d_umax = nullptr;    // device, per dispatch unit: its most expensive wave, then
                                   // (behind the nu maxima) the sum of its waves: 2 nu words
    uint32_t* h_umax = nullptr;    // pinned host snapshot of d_umax
    size_t umax_cap = 0;           // in units (the buffers hold 2 words per unit)
    int cost_ul = 0;               // units per tile row (log2) of the pending snapshot
    hipEvent_t ev_cost = nullptr;  // snapshot landed
    bool cost_pending = false;
    // RT_OPT_ROW_FEEDBACK_ISOLATE (default 0): a sampled frame runs alone on the GPU — its
    // stream waits for the other streams' latest frames, and each other stream's next frame
    // waits for it — so its wave costs are not those of two frames sharing the CUs (frames
    // in flight overlap a frame's tail with the next one's start, which inflated or hid the
    // costs of the tiles dispatched first and could install a worse order for 32 frames)
    bool fb_isolate = false;
    hipEvent_t ev_iso = nullptr;         // recorded behind the sampled frame
    bool iso_pending = false;
    std::vector<hipStream_t> iso_seen;   // streams already ordered behind ev_iso
    struct Band {
        int32_t W = -1, row0 = -1, nrows = -1;
        unsigned long long scene_gen = 0;
        unsigned fb_epoch = 0;  // rt_set_option(RT_OPT_ROW_FEEDBACK) starts a new epoch
        int32_t tstride = 0, tphase = 0;  // interleaved parts (KParams::tstride)
        bool operator==(const Band& o) const {
            return W == o.W && row0 == o.row0 && nrows == o.nrows && scene_gen == o.scene_gen &&
                   fb_epoch == o.fb_epoch && tstride == o.tstride && tphase == o.tphase;
        }
    };
    unsigned fb_epoch = 0;  // a snapshot still in flight from an older epoch is not used
    Band cost_band;                // band of the pending snapshot
    Band fb_band;                  // band fb.perm was computed for
    UnitOrder fb;                  // (rt_row_order.cpp) fb.acc, fb.work: of fb_band
    int fb_units_log2 = 0;         // dispatch units per tile row (log2) of fb.perm
    // RT_OPT_ROW_FEEDBACK_EMA: per-unit cost smoothed over the snapshots of one band
    // (acc = w*acc + (1-w)*new), so one noisy snapshot (tile costs measured while another
    // frame's waves shared the GPU) does not reorder the rows on its own; 0 = off
    int fb_ema = 0;                // w in percent
    int since_snapshot = 0;
    // RT_OPT_ROW_FEEDBACK_WARM: after a new band or scene, this many further snapshots are
    // taken back to back (each as soon as the previous one has landed) before the interval
    // applies, so the order settles within a few frames instead of a few intervals
    int fb_warm = 0;
    int warm_left = 0;
};

/* RT_OPT_FRAME_BATCH: the pipelined frame loop launches up to frame_batch consecutive
 * frames that share a stream as ONE grid (frame = blockIdx.z, rt::launch_trace_batch),
 * their kernel arguments in a device table copied from pinned memory in front of the
 * launch.  SLOTS groups may be in flight; a slot is reused once its launch (whose stop
 * event is ev[slot]) has completed.  Launching thread only (rt_render.cpp; wait_inflight
 * retires the busy slots). */
struct FrameTable {
    int frame_batch = 1;
    static constexpr int SLOTS = 64;
    rt::KParams* h_tab = nullptr;  // pinned, SLOTS x RT_MULTI_BATCH_MAX
    rt::KParams* d_tab = nullptr;  // device, the same
    hipEvent_t ev[SLOTS] = {};
    bool busy[SLOTS] = {};
    int next = 0;
};

/* The host-staged entry points' buffers (rt_render, rt_trace_rays, rt_occluded; all on
 * ctx->stream, idle between calls).  Launching thread only. */
struct Staging {
    void* d_out = nullptr;   // pixels / colours
    size_t d_out_cap = 0;
    void* d_rays = nullptr;  // origins then directions (rt_occluded: then the limits)
    size_t d_rays_cap = 0;
    void* d_hits = nullptr;  // hit records (rt_occluded: the mask bytes)
    size_t d_hits_cap = 0;
    unsigned long long* d_segs = nullptr;  // the optional counter (segments, occluded rays)
    hipEvent_t ev0 = nullptr, ev1 = nullptr;  // around the launch: rt_stats::ms
};

/* Renders enqueued on caller streams (rt_render_device): per stream, an event recorded
 * behind its latest launch.  rt_set_scene and rt_ctx_destroy wait on every one of them
 * before they overwrite or free the device scene, so a frame still in flight on a
 * non-blocking stream never reads a half-replaced scene. */
struct Inflight {
    hipStream_t stream;
    hipEvent_t ev;
};

struct Prep;  // rt_render.cpp: RT_OPT_HOST_PIPELINE's helper thread and its ring

}  // namespace rth

struct rt_ctx {
    int device = 0;
    hipStream_t stream = nullptr;
    void* d_scene = nullptr;
    size_t scene_bytes = 0;
    bool have_scene = false;
    unsigned long long scene_gen = 0;  // bumped by every rt_set_scene
    rth::SceneHost sc;
    rt::LightArgs lights{};  // rt_set_lights: n == 0 = the reference's light (plain kernels)
    // rt_set_transmission: the device table of the records in force (null = none: the kernels a
    // ctx without records launches).  A set allocates a new table, so launches in flight keep
    // reading theirs; replaced tables wait in glass_retired until nothing can read them
    // (wait_inflight: rt_set_scene, rt_ctx_destroy, or a full list).
    rt::DevGlass* d_glass = nullptr;
    std::vector<rt::DevGlass*> glass_retired;
    rth::FrameOptions opt;
    rth::BoxCache box_cache;
    rth::BoxCache aov_box_cache;  // rt_render_aov* / rt_render_ao*'s own (rt_aov.cpp primary_params):
                                  // the colour frames' stays as it was
    rth::RowFeedback rf;
    rth::FrameTable tab;
    rth::Staging stg;
    std::vector<rth::Inflight> inflight;
    // RT_OPT_HOST_PIPELINE: rt_render_device_frames computes frame f+1's kernel arguments
    // (pixel boxes, mirror chains, eye tables: make_params) on a helper thread while this
    // thread launches frame f (rt_render.cpp render_frames_pipelined)
    bool host_pipeline = true;
    rth::Prep* prep = nullptr;
    // RT_OPT_ROW_MIX: 0 = heaviest first; 1 (default) = the mixed order for the frames of an
    // rt_render_device_frames call spread over several streams (frames_overlap), whose tail
    // the next frame fills; 2 = the mixed order for every frame
    int row_mix = RT_ROW_MIX_DEFAULT;
    bool frames_overlap = false;   // inside rt_render_device_frames with >= 2 distinct streams
    bool last_of_call = false;     // ... and this frame is the call's last: nothing is known to
                                   // follow it, so its tail counts as exposed (heaviest first)
    char last_err[256] = {0};

    rth::FrameScene frame_scene() const { return {sc, opt, d_scene, scene_gen}; }
};

namespace rth __attribute__((visibility("hidden"))) {

/* ---- rt_capi.cpp ---------------------------------------------------------------------- */

int hip_fail(rt_ctx* ctx, hipError_t e, const char* what);

#define RT_HIP(ctx, call)                                   \
    do {                                                    \
        hipError_t e_ = (call);                             \
        if (e_ != hipSuccess) return rth::hip_fail(ctx, e_, #call); \
    } while (0)

/* Makes the ctx's device current for the duration of an entry point and restores the
 * caller's current device on every return path (the boundary must not change it). */
struct DeviceGuard {
    int prev = -1;
    hipError_t err = hipSuccess;
    explicit DeviceGuard(int device) {
        if (hipGetDevice(&prev) != hipSuccess) prev = -1;
        if (prev != device) err = hipSetDevice(device);
    }
    ~DeviceGuard() {
        int cur = -1;
        if (prev >= 0 && hipGetDevice(&cur) == hipSuccess && cur != prev) (void)hipSetDevice(prev);
    }
    DeviceGuard(const DeviceGuard&) = delete;
    DeviceGuard& operator=(const DeviceGuard&) = delete;
};

/* Before a launch on `st` (a caller stream): the stream's in-flight event, which the
 * launch signals on completion (rt::launch_trace's done_event); null for ctx->stream. */
int launch_event(rt_ctx* ctx, hipStream_t st, hipEvent_t* ev);

/* Every render this ctx has enqueued, on any stream, has finished. */
int wait_inflight(rt_ctx* ctx);

int bytes_per_pixel(int32_t out_format);

/* The host-staged entry points (rt_render, rt_trace_rays, rt_occluded) stage through the
 * ctx's buffers on ctx->stream: grow() a buffer on demand (the stream idle while it moves);
 * staged_begin zeroes the optional counter and records ev0 in front of the launch; the
 * caller launches, records ev1 directly behind it and enqueues its copies back; then
 * staged_finish copies the counter back (*value, may be null), synchronises and fills the
 * stats (segments = the counter). */
int grow(rt_ctx* ctx, void** buf, size_t* cap, size_t bytes);
int staged_begin(rt_ctx* ctx, unsigned long long* counter);
int staged_finish(rt_ctx* ctx, unsigned long long* counter, uint64_t* value, rt_stats* stats);

/* ---- rt_feedback.cpp ------------------------------------------------------------------ */

/* Before a launch on st: the row order (explicit, else the feedback's for p's band) and,
 * when a snapshot is due, the cost buffer (p.tile_cost: the frame is "sampled"). */
int prepare_rows(rt_ctx* ctx, hipStream_t st, rt::KParams& p);
/* Behind the launch of a sampled frame: its costs copied back. */
int snapshot_costs(rt_ctx* ctx, hipStream_t st, const rt::KParams& p);
/* RT_OPT_ROW_FEEDBACK_ISOLATE: around a launch on st. */
int isolate_before(rt_ctx* ctx, hipStream_t st, bool sampled);
int isolate_after(rt_ctx* ctx, hipStream_t st, bool sampled);
void feedback_release(rt_ctx* ctx);  // rt_ctx_destroy

/* ---- rt_render.cpp -------------------------------------------------------------------- */

int check_render_args(const rt_ctx* ctx, const rt_camera* cam, int32_t row0, int32_t nrows,
                      const FrameReq& rq);
/* RT_FLAG_SHADOWS and scene lights (rt_capi.h): the shadow and lights kernels exist for the
 * fp64-path precisions without the sun term; checked before anything is launched.  lights: the
 * ctx has lights (rt_set_lights) or transmission records (rt_set_transmission) set. */
/* The ctx launches kernels of its own for every shaded frame or batch: lights or transmission
 * records are set. */
inline bool own_kernels(const rt_ctx* ctx) { return ctx->lights.n > 0 || ctx->d_glass != nullptr; }
/* What the glass kernels take as lights: the ctx's, or the reference's one white light at the
 * origin, which gives the plain kernels' bits (rt_capi.h "Lights"). */
inline rt::LightArgs glass_lights(const rt_ctx* ctx) {
    if (ctx->lights.n > 0) return ctx->lights;
    rt::LightArgs la{};
    for (int k = 0; k < 3; k++) la.l[0].col[k] = 1.0, la.l[0].colf[k] = 1.0f;
    la.n = 1;
    return la;
}
inline int check_shadow_flags(int32_t precision, uint32_t flags, bool lights = false) {
    if (!(flags & RT_FLAG_SHADOWS) && !lights) return RT_OK;
    if (precision == RT_PREC_F32 || (flags & RT_FLAG_SUN)) return RT_ERR_UNSUPPORTED;
    return RT_OK;
}
void render_shutdown(rt_ctx* ctx);       // rt_ctx_destroy, first: joins the helper thread
void frame_table_release(rt_ctx* ctx);   // rt_ctx_destroy, with nothing in flight

/* ---- rt_aov.cpp ----------------------------------------------------------------------- */

/* The kernel arguments of a frame's PRIMARY segment alone (rt_render_aov*, rt_render_ao*): the
 * camera, the band, eye tables, wall order, primary pixel boxes and cull choice of make_params,
 * with the options that have no meaning there switched off (supersampling, lights, pixel pairs,
 * mirror chains), through the ctx's aov_box_cache.  Nothing of the row feedback takes part. */
rt::KParams primary_params(rt_ctx* ctx, const rt_camera* cam, int32_t row0, int32_t nrows);

}  // namespace rth

#endif
