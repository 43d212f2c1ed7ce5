/*
 * rt_render.cpp — the frame entry points (rt_render, rt_render_device*, the pipelined and
 * batched frame loop of rt_render_device_frames).  A frame is: the argument checks, the
 * kernel arguments (make_params, rt_frame_args.cpp — on this thread, or ahead of it on the
 * helper thread), the row order (prepare_rows, rt_feedback.cpp), the launch, the cost
 * snapshot of a sampled frame.
 */
#include <algorithm>
#include <atomic>
#include <chrono>
#include <condition_variable>
#include <mutex>
#include <new>
#include <thread>

#include "rt_ctx.h"

#ifndef RT_DRY_LAUNCH     // diagnostic build: 1 = no kernel launch in rt_render_device*,
#define RT_DRY_LAUNCH 0   // 2 = nor rt_multi's per-frame runtime calls (never in the product)
#endif
#ifndef RT_HOST_PROFILE   // diagnostic build: per-phase host time of rt_render_device, printed
#define RT_HOST_PROFILE 0 // to stderr by rt_ctx_destroy (never in the product)
#endif
#if RT_HOST_PROFILE
static double g_hp[5], g_hp_t;  // per-phase sums; the running phase's start (launching thread)
static long g_hn;
static inline double hp_now() {
    return std::chrono::duration<double, std::micro>(
               std::chrono::steady_clock::now().time_since_epoch()).count();
}
#define HP_START() (g_hp_t = hp_now())
#define HP(i) (g_hp[(i)] += (g_hn > 50 ? hp_now() - g_hp_t : 0.0), g_hp_t = hp_now())  // warm calls only
#else
#define HP_START() ((void)0)
#define HP(i) ((void)0)
#endif

namespace rth __attribute__((visibility("hidden"))) {

/* The frames of one rt_render_device_frames call: frame f renders cams[f % ncams] into
 * d_outs[f % nouts] on streams[f % nstreams] (nstreams 0: the ctx's stream). */
struct FrameBatch {
    const rt_camera* cams;
    int32_t ncams, row0, nrows;
    void* const* d_outs;
    int32_t nouts;
    void* const* streams;
    int32_t nstreams, nframes;
    void* stream(int32_t f) const { return nstreams > 0 ? streams[f % nstreams] : nullptr; }
};

/* RT_OPT_HOST_PIPELINE's helper thread.  A batch (rt_render_device_frames) posts its frames;
 * the helper computes each frame's make_params into a ring of RING slots, at most RING frames
 * ahead of the launching thread, which takes a slot, finishes the frame (row order, launch,
 * cost snapshot) and releases it.  make_params only reads the scene and the options and
 * uses the ctx's box cache, which no other code touches while a batch runs; everything that
 * changes ctx state (the row feedback) stays on the launching thread. */
struct Prep {
    static constexpr int RING = 3;
    std::thread th;
    std::mutex mu;
    std::condition_variable cv;
    bool quit = false;
    // the posted batch: read by the helper only
    FrameBatch b{};
    FrameReq rq{};
    std::atomic<uint64_t> posted{0}, done{0};  // batches posted / finished by the helper
    std::atomic<int> produced{0}, consumed{0};
    std::atomic<bool> stop{false};             // the launching thread gave up on the batch
    rt::KParams slot[RING];
};

namespace {

void prep_main(rt_ctx* ctx) {
    Prep& q = *ctx->prep;
    uint64_t seen = 0;
    for (;;) {
        uint64_t g = q.posted.load(std::memory_order_acquire);
        for (int it = 0; g == seen && it < 2048; it++) {
            std::this_thread::yield();
            g = q.posted.load(std::memory_order_acquire);
        }
        if (g == seen) {
            std::unique_lock<std::mutex> lk(q.mu);
            q.cv.wait(lk, [&] { return q.quit || q.posted.load(std::memory_order_acquire) != seen; });
            if (q.quit) return;
            g = q.posted.load(std::memory_order_acquire);
        }
        seen = g;
        const FrameBatch& b = q.b;
        for (int f = 0; f < b.nframes; f++) {
            while (f - q.consumed.load(std::memory_order_acquire) >= Prep::RING &&
                   !q.stop.load(std::memory_order_acquire))
                std::this_thread::yield();
            if (q.stop.load(std::memory_order_acquire)) break;
            VirtFrame v;  // (cannot fail: the batch's frames were checked before it was posted)
            if (virt_frame(ctx->opt.ss_log2, &b.cams[f % b.ncams], b.row0, b.nrows, v) != RT_OK) v.nrows = 0;
            q.slot[f % Prep::RING] = make_params(ctx->frame_scene(), &ctx->box_cache, v.cam, v.row0,
                                                 v.nrows, q.rq, b.d_outs[f % b.nouts], nullptr);
            q.produced.store(f + 1, std::memory_order_release);
        }
        q.done.store(seen, std::memory_order_release);
    }
}

/* The frame launch: the lights kernels (rt_trace_lights.hip) for a frame prepared while the ctx
 * had lights set (they take RT_FLAG_SHADOWS at run time), with the ctx's current records; the
 * shadow kernels (rt_trace_shadow.hip) for a flagged frame without lights. */
int launch_frame(const rt_ctx* ctx, const rt::KParams& p, int32_t precision, void* stream,
                 void* done_event = nullptr) {
    if (p.flags & rt::FLAG_GLASS) {  // rt_set_transmission: the glass kernels, lights or not
        if (!ctx->d_glass) return (int)hipErrorInvalidValue;
        return rt::launch_trace_glass(p, glass_lights(ctx), rt::GlassArgs{ctx->d_glass}, precision, stream,
                                      done_event);
    }
    if (p.flags & rt::FLAG_LIGHTS)
        return rt::launch_trace_lights(p, ctx->lights, precision, stream, done_event);
    if (p.flags & rt::FLAG_SHADOWS) return rt::launch_trace_shadow(p, precision, stream, done_event);
    return rt::launch_trace(p, precision, stream, done_event);
}

/* Pixel rows of interleaved part `part` of `nparts` (tile rows part, part + nparts, ...). */
int32_t interleaved_rows(int32_t height, int32_t nparts, int32_t part) {
    const int32_t T = (height + rt::TILE_H - 1) / rt::TILE_H;
    int32_t n = 0;
    for (int32_t t = part; t < T; t += nparts) n += std::min(rt::TILE_H, height - t * rt::TILE_H);
    return n;
}

/* One frame whose arguments are complete (prepare_rows done): the stream's in-flight event,
 * the isolation waits, the launch, the cost snapshot of a sampled frame. */
int launch_prepared(rt_ctx* ctx, const rt::KParams& p, int32_t precision, hipStream_t hs) {
    hipEvent_t done = nullptr;
    int st = launch_event(ctx, hs, &done);
    if (st != RT_OK) return st;
    const bool sampled = p.tile_cost != nullptr;
    st = isolate_before(ctx, hs, sampled);
    if (st != RT_OK) return st;
    HP(2);
    // RT_DRY_LAUNCH (diagnostic builds, tools/multi_host_cost.py): every host step of the
    // frame but the kernel launch, to separate the host's own work from the runtime's
    const int e = RT_DRY_LAUNCH ? (int)hipSuccess : launch_frame(ctx, p, precision, hs, done);
    if (e != (int)hipSuccess) return hip_fail(ctx, (hipError_t)e, "launch k_trace");
    if (RT_DRY_LAUNCH) return RT_OK;
    st = isolate_after(ctx, hs, sampled);
    if (st != RT_OK) return st;
    HP(3);
    st = snapshot_costs(ctx, hs, p);
    HP(4);
    return st;
}

/* rt_render_device_interleaved's band: part `part` of `nparts` >= 2 (nrows = its pixel rows). */
struct Interleave {
    int32_t nparts, part, out_frame;
};

/* rt_render_device and rt_render_device_interleaved: a contiguous band [row0, row0 + nrows)
 * (il null) or an interleaved part.  pre: the frame's arguments, computed by the host
 * pipeline's helper thread (contiguous bands only). */
int render_device_impl(rt_ctx* ctx, const rt_camera* cam, int32_t row0, int32_t nrows,
                       const FrameReq& rq, void* d_out, uint64_t* d_segments, void* stream,
                       const rt::KParams* pre = nullptr, const Interleave* il = nullptr) {
#if RT_HOST_PROFILE
    g_hn++;
#endif
    HP_START();
    int st = check_render_args(ctx, cam, row0, nrows, rq);
    if (st == RT_OK) st = check_shadow_flags(rq.precision, rq.flags, own_kernels(ctx));
    if (st != RT_OK) return st;
    if (!d_out && nrows > 0 && cam->width > 0) return RT_ERR_INVALID_ARG;
    if (ctx->opt.ss_log2 && il) return RT_ERR_UNSUPPORTED;  // contiguous bands only
    // from here on: the frame the kernels trace (RT_OPT_SUPERSAMPLE: S times larger)
    VirtFrame vf;
    st = virt_frame(ctx->opt.ss_log2, cam, row0, nrows, vf);
    if (st != RT_OK) return st;
    cam = vf.cam;
    row0 = vf.row0;
    nrows = vf.nrows;
    // the ctx's buffers (row feedback) and the launch belong to ctx->device, whatever
    // device the caller has current
    DeviceGuard dg(ctx->device);
    RT_HIP(ctx, dg.err);
    HP(0);
    // an interleaved part's tile rows span the frame: its pixel boxes are the whole frame's
    rt::KParams p = pre ? *pre
                        : make_params(ctx->frame_scene(), &ctx->box_cache, cam, il ? 0 : row0,
                                      il ? cam->height : nrows, rq, d_out,
                                      reinterpret_cast<unsigned long long*>(d_segments));
    if (il) {
        p.row0 = 0;
        p.nrows = nrows;
        p.tstride = il->nparts;
        p.tphase = il->part;
        p.frame_h = cam->height;
        p.out_frame = il->out_frame ? 1 : 0;
        p.pairs = 0;  // the two-pixel kernel is contiguous-only
        // centre-out dispatch from the part's tile row nearest the frame's heavy row
        const int nt = (nrows + rt::TILE_H - 1) / rt::TILE_H;
        p.row_center = std::max(0, std::min(nt - 1, (p.row_center - il->part) / il->nparts));
    }
    HP(1);
    hipStream_t hs = stream ? static_cast<hipStream_t>(stream) : ctx->stream;
    st = prepare_rows(ctx, hs, p);
    if (st != RT_OK) return st;
    return launch_prepared(ctx, p, rq.precision, hs);
}

/* RT_OPT_FRAME_BATCH: a group of n >= 2 prepared frames of one stream (their arguments in
 * the pinned table slot s) as one launch — the slot copied into the device table behind the
 * stream's earlier work, then one grid of n frames whose stop event marks the slot free
 * again; n == 1 is an ordinary launch. */
int launch_group(rt_ctx* ctx, int s, int n, int32_t precision, hipStream_t hs) {
    if (n <= 0) return RT_OK;
    FrameTable& t = ctx->tab;
    rt::KParams* grp = t.h_tab + (size_t)s * RT_MULTI_BATCH_MAX;
    HP_START();
    if (n == 1) return launch_prepared(ctx, grp[0], precision, hs);
    int st = isolate_before(ctx, hs, false);
    if (st != RT_OK) return st;
    rt::KParams* dst = t.d_tab + (size_t)s * RT_MULTI_BATCH_MAX;
    RT_HIP(ctx, hipMemcpyAsync(dst, grp, (size_t)n * sizeof(rt::KParams), hipMemcpyHostToDevice, hs));
    const int e = RT_DRY_LAUNCH ? (int)hipSuccess
                                : rt::launch_trace_batch(dst, grp[0], n, precision, hs, t.ev[s]);
    if (e != (int)hipSuccess) return hip_fail(ctx, (hipError_t)e, "launch k_trace_tab");
    t.busy[s] = !RT_DRY_LAUNCH;
    t.next = (s + 1) % FrameTable::SLOTS;
    return RT_OK;
}

/* The pipelined frame loop with RT_OPT_FRAME_BATCH: consecutive frames are grouped while they
 * share a stream (frames on one stream run in order anyway), write distinct buffers, have
 * the same grid (a row order change between them starts a new group) and are not sampled by
 * the row feedback (a sampled frame runs alone, through the stamped kernels, then its cost
 * snapshot); each group is one launch.  Every frame's arguments, row order and feedback
 * bookkeeping are the per-frame loop's, so the output is identical. */
int launch_frame_groups(rt_ctx* ctx, const FrameBatch& b, const FrameReq& rq) {
    Prep& q = *ctx->prep;
    FrameTable& t = ctx->tab;
    DeviceGuard dg(ctx->device);
    RT_HIP(ctx, dg.err);
    if (!t.d_tab) {
        const size_t n = (size_t)FrameTable::SLOTS * RT_MULTI_BATCH_MAX;
        for (auto& e : t.ev)
            if (!e) RT_HIP(ctx, hipEventCreateWithFlags(&e, hipEventDisableTiming));
        if (!t.h_tab) RT_HIP(ctx, hipHostMalloc(&t.h_tab, n * sizeof(rt::KParams), hipHostMallocDefault));
        RT_HIP(ctx, hipMalloc(&t.d_tab, n * sizeof(rt::KParams)));
    }
    int st = RT_OK;
    int32_t f = 0;
    while (f < b.nframes && st == RT_OK) {
        void* const stf = b.stream(f);
        hipStream_t hs = stf ? static_cast<hipStream_t>(stf) : ctx->stream;
        const int s = t.next;  // this group's table slot: free once its last launch ended
        if (t.busy[s]) {
            RT_HIP(ctx, hipEventSynchronize(t.ev[s]));
            t.busy[s] = false;
        }
        rt::KParams* grp = t.h_tab + (size_t)s * RT_MULTI_BATCH_MAX;
        const void* outs[RT_MULTI_BATCH_MAX];
        int n = 0;
        while (f < b.nframes && n < t.frame_batch) {
            void* const out = b.d_outs[f % b.nouts];
            if (n > 0 && (b.stream(f) != stf || std::find(outs, outs + n, out) != outs + n)) break;
            while (q.produced.load(std::memory_order_acquire) <= f) std::this_thread::yield();
            rt::KParams& p = grp[n];
            p = q.slot[f % Prep::RING];
            q.consumed.store(f + 1, std::memory_order_release);
            ctx->last_of_call = f + 1 == b.nframes;
            st = prepare_rows(ctx, hs, p);
            if (st != RT_OK) break;
            const bool other_grid = n > 0 && (p.W != grp[0].W || p.nrows != grp[0].nrows ||
                                              p.row_units_log2 != grp[0].row_units_log2);
            // (no table kernels for the cull, pair, supersample, shadow, lights and glass paths: one
            // launch each)
            if (p.tile_cost || other_grid || p.wave_cull || p.pairs || p.ss_log2 ||
                (p.flags & (rt::FLAG_SHADOWS | rt::FLAG_LIGHTS | rt::FLAG_GLASS))) {
                // this frame alone (after the frames grouped so far), through the per-frame path
                const rt::KParams one = p;
                st = launch_group(ctx, s, n, rq.precision, hs);
                HP_START();
                if (st == RT_OK) st = launch_prepared(ctx, one, rq.precision, hs);
                n = 0;
                f++;
                break;
            }
            outs[n++] = out;
            f++;
        }
        if (st == RT_OK) st = launch_group(ctx, s, n, rq.precision, hs);
    }
    // the helper thread must not wait for a consumer that stopped early
    q.consumed.store(b.nframes, std::memory_order_release);
    return st;
}

/* rt_render_device_frames with the host pipeline (RT_OPT_HOST_PIPELINE): the helper thread
 * computes make_params of the next frames while this thread launches the current one, so a
 * frame costs the host max(arguments, launch) instead of their sum.  Same launches, same
 * order, same arguments as the sequential loop. */
int render_frames_pipelined(rt_ctx* ctx, const FrameBatch& b, const FrameReq& rq) {
    if (!ctx->prep) {
        ctx->prep = new (std::nothrow) Prep();
        if (!ctx->prep) return RT_ERR_OUT_OF_MEMORY;
        try {
            ctx->prep->th = std::thread(prep_main, ctx);
        } catch (...) {
            delete ctx->prep;
            ctx->prep = nullptr;
            return RT_ERR_OUT_OF_MEMORY;
        }
    }
    Prep& q = *ctx->prep;
    q.b = b;
    q.rq = rq;
    q.produced.store(0, std::memory_order_relaxed);
    q.consumed.store(0, std::memory_order_relaxed);
    q.stop.store(false, std::memory_order_relaxed);
    uint64_t g;
    {
        std::lock_guard<std::mutex> lk(q.mu);
        g = q.posted.load(std::memory_order_relaxed) + 1;
        q.posted.store(g, std::memory_order_release);
    }
    q.cv.notify_one();
    int st = RT_OK;
    if (ctx->tab.frame_batch > 1) {
        st = launch_frame_groups(ctx, b, rq);
    } else {
        for (int32_t f = 0; f < b.nframes; f++) {
            while (q.produced.load(std::memory_order_acquire) <= f) std::this_thread::yield();
            ctx->last_of_call = f + 1 == b.nframes;
            st = render_device_impl(ctx, &b.cams[f % b.ncams], b.row0, b.nrows, rq, b.d_outs[f % b.nouts],
                                    nullptr, b.stream(f), &q.slot[f % Prep::RING]);
            q.consumed.store(f + 1, std::memory_order_release);
            if (st != RT_OK) break;
        }
    }
    // the helper is done with this batch before its arguments (cams, d_outs) go out of scope
    q.stop.store(true, std::memory_order_release);
    while (q.done.load(std::memory_order_acquire) != g) std::this_thread::yield();
    return st;
}

}  // namespace

int check_render_args(const rt_ctx* ctx, const rt_camera* cam, int32_t row0, int32_t nrows,
                      const FrameReq& rq) {
    if (!ctx || !cam) return RT_ERR_INVALID_ARG;
    if (!ctx->have_scene) return RT_ERR_NO_SCENE;
    if (cam->width < 0 || cam->height < 0 || nrows < 0) return RT_ERR_INVALID_ARG;
    if (row0 < 0 || row0 + nrows > cam->height) return RT_ERR_OUT_OF_RANGE;
    if (rq.depth < 0) return RT_ERR_INVALID_ARG;
    if (rq.depth > rt::max_depth()) return RT_ERR_UNSUPPORTED;
    if (rq.precision < RT_PREC_F64 || rq.precision > RT_PREC_PATH64) return RT_ERR_INVALID_ARG;
    if (bytes_per_pixel(rq.out_format) == 0) return RT_ERR_INVALID_ARG;
    return RT_OK;
}

void render_shutdown(rt_ctx* ctx) {
#if RT_HOST_PROFILE
    if (g_hn > 50) {
        const double m = (double)(g_hn - 50);
        std::fprintf(stderr, "host profile over %ld warm renders (us): args %.2f params %.2f rows+event %.2f launch %.2f snapshot %.2f\n",
                     g_hn - 50, g_hp[0] / m, g_hp[1] / m, g_hp[2] / m, g_hp[3] / m, g_hp[4] / m);
    }
#endif
    if (!ctx->prep) return;
    {
        std::lock_guard<std::mutex> lk(ctx->prep->mu);
        ctx->prep->quit = true;
    }
    ctx->prep->cv.notify_one();
    if (ctx->prep->th.joinable()) ctx->prep->th.join();
    delete ctx->prep;
    ctx->prep = nullptr;
}

void frame_table_release(rt_ctx* ctx) {
    FrameTable& t = ctx->tab;
    for (auto& e : t.ev)
        if (e) (void)hipEventDestroy(e);
    if (t.d_tab) (void)hipFree(t.d_tab);
    if (t.h_tab) (void)hipHostFree(t.h_tab);
}

}  // namespace rth

using namespace rth;

extern "C" {

int rt_render_device(rt_ctx* ctx, const rt_camera* cam, int32_t row0, int32_t nrows,
                     int32_t depth, int32_t precision, uint32_t flags, int32_t out_format,
                     void* d_out, uint64_t* d_segments, void* stream) {
    return render_device_impl(ctx, cam, row0, nrows, FrameReq{depth, precision, flags, out_format},
                              d_out, d_segments, stream);
}

int rt_interleaved_rows(int32_t height, int32_t nparts, int32_t part, int32_t* nrows) {
    if (!nrows || height < 0 || nparts <= 0 || part < 0 || part >= nparts) return RT_ERR_INVALID_ARG;
    *nrows = interleaved_rows(height, nparts, part);
    return RT_OK;
}

int rt_render_device_interleaved(rt_ctx* ctx, const rt_camera* cam, int32_t nparts, int32_t part,
                                 int32_t depth, int32_t precision, uint32_t flags,
                                 int32_t out_format, void* d_out, int32_t out_frame_rows,
                                 uint64_t* d_segments, void* stream) {
    if (!ctx || !cam || nparts <= 0 || part < 0 || part >= nparts || cam->height < 0)
        return RT_ERR_INVALID_ARG;
    const FrameReq rq{depth, precision, flags, out_format};
    if (nparts == 1)  // the whole frame: a contiguous band, stored at its frame rows anyway
        return render_device_impl(ctx, cam, 0, cam->height, rq, d_out, d_segments, stream);
    if (rt::TILE_H != 8) return RT_ERR_UNSUPPORTED;  // parts are dealt in 8-row tile rows
    const Interleave il{nparts, part, out_frame_rows};
    return render_device_impl(ctx, cam, 0, interleaved_rows(cam->height, nparts, part), rq, d_out,
                              d_segments, stream, nullptr, &il);
}

int rt_render_device_frames(rt_ctx* ctx, const rt_camera* cams, int32_t ncams, int32_t row0,
                            int32_t nrows, int32_t depth, int32_t precision, uint32_t flags,
                            int32_t out_format, void* const* d_outs, int32_t nouts,
                            void* const* streams, int32_t nstreams, int32_t nframes) {
    if (!ctx || !cams || ncams <= 0 || !d_outs || nouts <= 0 || nframes < 0 ||
        (nstreams > 0 && !streams) || nstreams < 0)
        return RT_ERR_INVALID_ARG;
    if (nframes > 0 && check_shadow_flags(precision, flags, own_kernels(ctx)) != RT_OK)
        return RT_ERR_UNSUPPORTED;
    const FrameReq rq{depth, precision, flags, out_format};
    const FrameBatch b{cams, ncams, row0, nrows, d_outs, nouts, streams, nstreams, nframes};
    // RT_OPT_ROW_MIX 1: consecutive frames on different streams overlap on the GPU
    struct Overlap {
        bool &f, &l;
        ~Overlap() { f = l = false; }
    } overlap{ctx->frames_overlap, ctx->last_of_call};
    for (int32_t k = 1; k < nstreams && k < nframes; k++)
        if (streams[k] != streams[0]) ctx->frames_overlap = true;
    if (ctx->host_pipeline && nframes >= 2 && !RT_DRY_LAUNCH) {
        // every frame's arguments checked up front (the pipeline's helper computes them
        // unchecked); a batch with an invalid frame takes the sequential loop, which stops
        // at that frame with its status
        bool ok = true;
        for (int32_t c = 0; c < ncams && c < nframes && ok; c++)
            ok = check_render_args(ctx, &cams[c], row0, nrows, rq) == RT_OK;
        for (int32_t f = 0; f < nframes && f < nouts && ok; f++)
            ok = d_outs[f] != nullptr || nrows == 0 || cams[f % ncams].width == 0;
        if (ok) return render_frames_pipelined(ctx, b, rq);
    }
    for (int32_t f = 0; f < nframes; f++) {
        ctx->last_of_call = f + 1 == nframes;
        const int e = render_device_impl(ctx, &cams[f % ncams], row0, nrows, rq, d_outs[f % nouts],
                                         nullptr, b.stream(f));
        if (e != RT_OK) return e;
    }
    return RT_OK;
}

int rt_render(rt_ctx* ctx, const rt_camera* cam, int32_t row0, int32_t nrows, int32_t depth,
              int32_t precision, uint32_t flags, int32_t out_format, void* out,
              int32_t count_segments, rt_stats* stats) {
    const FrameReq rq{depth, precision, flags, out_format};
    int st = check_render_args(ctx, cam, row0, nrows, rq);
    if (st == RT_OK) st = check_shadow_flags(precision, flags, own_kernels(ctx));
    if (st != RT_OK) return st;
    const size_t bytes = (size_t)nrows * (size_t)cam->width * (size_t)bytes_per_pixel(out_format);
    if (!out && bytes > 0) return RT_ERR_INVALID_ARG;
    DeviceGuard dg(ctx->device);
    RT_HIP(ctx, dg.err);
    Staging& g = ctx->stg;
    if ((st = grow(ctx, &g.d_out, &g.d_out_cap, bytes)) != RT_OK) return st;
    unsigned long long* segs = count_segments ? g.d_segs : nullptr;
    // host staging above is the output frame's; the kernels trace the (RT_OPT_SUPERSAMPLE:
    // S times larger) frame below
    VirtFrame vf;
    st = virt_frame(ctx->opt.ss_log2, cam, row0, nrows, vf);
    if (st != RT_OK) return st;
    rt::KParams p = make_params(ctx->frame_scene(), &ctx->box_cache, vf.cam, vf.row0, vf.nrows, rq,
                                g.d_out, segs);
    st = prepare_rows(ctx, ctx->stream, p);
    if (st != RT_OK) return st;
    if ((st = staged_begin(ctx, segs)) != RT_OK) return st;
    const int e = launch_frame(ctx, p, precision, ctx->stream);
    if (e != (int)hipSuccess) return hip_fail(ctx, (hipError_t)e, "launch k_trace");
    RT_HIP(ctx, hipEventRecord(g.ev1, ctx->stream));
    st = snapshot_costs(ctx, ctx->stream, p);
    if (st != RT_OK) return st;
    if (bytes > 0)
        RT_HIP(ctx, hipMemcpyAsync(out, g.d_out, bytes, hipMemcpyDeviceToHost, ctx->stream));
    return staged_finish(ctx, segs, nullptr, stats);
}

}  // extern "C"
