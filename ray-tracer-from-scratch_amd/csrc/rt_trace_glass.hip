/* rt_trace_glass.hip — the frame kernels of rt_trace_lights.hip built once more (namespace
 * rt::kgl) with the passage step of rt_set_transmission: at a hit whose record has tau > 0 the
 * path goes on with the ray that passes through the object (rt_scan_dev.h glass_next: a pane
 * passes it on unbent, a sphere refracts it in, along the chord and out) and the unwind weighs
 * with tau in metallic's place.  RT_GLASS turns RT_LIGHTS on (rt_knobs.h): local colours, the
 * light loop and RT_FLAG_SHADOWS' runtime branch are the lights kernels'; without lights set the
 * host passes the reference's one light, which gives the plain kernels' bits.  Frames rendered
 * while records are set launch these (launch_trace_glass); every other frame the kernels it
 * launched before, whose code does not move.
 *
 * KParamsG = KParams + LightArgs + GlassArgs, one by-value kernel argument seen under the name
 * KParams by the shared headers (rt_trace_lights.hip has the reason).  The records themselves
 * live in a device table of the ctx, indexed by material slot like p.mat; the mirror bins are
 * not applied (mir_depth == 0: a ray that passed a pane did not reflect off it). */
#define RT_GLASS 1
#include "rt_knobs.h"

namespace rt {
namespace kgl {
struct KParamsG : rt::KParams {
    LightArgs lights;
    GlassArgs glass;
};
static_assert(sizeof(KParamsG) <= 16384, "kernel arguments over 16 KB");
#define KParams KParamsG
#include "rt_scan_dev.h"
#include "rt_frame_dev.h"

/* The glass unit's launchers — the lights unit's family: {F64, PATH64} x {linear, cull} x the
 * four depth tiers, F64 with the general pow() at the deepest tier only, each plain and
 * resolving (SS) — 36 kernels.  No sun, F32, pair, table or stamped variants. */
template <int PREC, bool INT_EXP, bool CULL, int MAXD, bool SS>
static void launch_one_gl(const KParams& p, dim3 grid, hipStream_t st, hipEvent_t done) {
    if (done)
        hipExtLaunchKernelGGL((k_trace<PREC, false, INT_EXP, CULL, MAXD, SS>), grid, dim3(BLOCK), 0, st,
                              nullptr, done, 0, p);
    else
        hipLaunchKernelGGL((k_trace<PREC, false, INT_EXP, CULL, MAXD, SS>), grid, dim3(BLOCK), 0, st, p);
}
template <int PREC, bool INT_EXP, bool CULL, bool SS>
static hipError_t launch_depth_gl(const KParams& p, dim3 grid, hipStream_t st, hipEvent_t done) {
    if constexpr (!INT_EXP) {
        launch_one_gl<PREC, false, CULL, MAXD_LARGE, SS>(p, grid, st, done);
    } else {
        if (p.depth <= MAXD_SMALL)
            launch_one_gl<PREC, true, CULL, MAXD_SMALL, SS>(p, grid, st, done);
        else if (p.depth <= MAXD_MID)
            launch_one_gl<PREC, true, CULL, MAXD_MID, SS>(p, grid, st, done);
        else if (p.depth <= MAXD_REF)
            launch_one_gl<PREC, true, CULL, MAXD_REF, SS>(p, grid, st, done);
        else
            launch_one_gl<PREC, true, CULL, MAXD_LARGE, SS>(p, grid, st, done);
    }
    return hipGetLastError();
}
template <int PREC, bool SS>
static hipError_t launch_prec_gl(const KParams& p, dim3 grid, hipStream_t st, hipEvent_t done) {
    // (PATH64's fp32 colour takes the exponent through v_log / v_exp either way)
    if (PREC == PREC_PATH64 || p.int_exp)
        return p.wave_cull ? launch_depth_gl<PREC, true, true, SS>(p, grid, st, done)
                           : launch_depth_gl<PREC, true, false, SS>(p, grid, st, done);
    if constexpr (PREC == PREC_F64)
        return p.wave_cull ? launch_depth_gl<PREC, false, true, SS>(p, grid, st, done)
                           : launch_depth_gl<PREC, false, false, SS>(p, grid, st, done);
    return hipErrorInvalidValue;
}
int launch_glass_ns(const KParams& p, int prec, void* stream, void* done_event) {
    if (p.W <= 0 || p.nrows <= 0) return (int)hipSuccess;
    if (p.depth < 0 || p.depth > MAXD_LARGE || (p.flags & FLAG_SUN)) return (int)hipErrorInvalidValue;
    if (p.lights.n < 1 || p.lights.n > MAX_LIGHTS) return (int)hipErrorInvalidValue;
    if (p.glass.rec == nullptr || p.mir_depth != 0) return (int)hipErrorInvalidValue;
    const int ul = p.row_units_log2;
    const int units = ((p.nrows + TILE_H - 1) / TILE_H) << ul;
    const dim3 grid((((p.W + TILE_W - 1) / TILE_W) + (1 << ul) - 1) >> ul, units, 1);
    hipStream_t st = static_cast<hipStream_t>(stream);
    hipEvent_t done = static_cast<hipEvent_t>(done_event);
    if (prec == PREC_MIXED) prec = PREC_F64;  // MIXED's contract is output == F64
    if (prec != PREC_F64 && prec != PREC_PATH64) return (int)hipErrorInvalidValue;
    if (p.ss_log2) {  // RT_OPT_SUPERSAMPLE: launch_trace_ns' conditions
        if (p.ss_log2 < 0 || p.ss_log2 > 3 || p.tstride > 1 || ((p.W | p.nrows) & ((1 << p.ss_log2) - 1)))
            return (int)hipErrorInvalidValue;
        return (int)(prec == PREC_F64 ? launch_prec_gl<PREC_F64, true>(p, grid, st, done)
                                      : launch_prec_gl<PREC_PATH64, true>(p, grid, st, done));
    }
    return (int)(prec == PREC_F64 ? launch_prec_gl<PREC_F64, false>(p, grid, st, done)
                                  : launch_prec_gl<PREC_PATH64, false>(p, grid, st, done));
}
#undef KParams

}  // namespace kgl

int launch_trace_glass(const KParams& p, const LightArgs& la, const GlassArgs& ga, int prec, void* stream,
                       void* done_event) {
    kgl::KParamsG pg;
    static_cast<KParams&>(pg) = p;
    pg.lights = la;
    pg.glass = ga;
    return kgl::launch_glass_ns(pg, prec, stream, done_event);
}

}  // namespace rt
