/* rt_trace_lights.hip — the frame kernels of rt_trace.hip built once more (namespace
 * rt::klt) with the scene lights of rt_set_lights: at every hit a loop over the light records
 * (rt_scan_dev.h shade_lights_d / shade_lights_f) and, with RT_FLAG_SHADOWS, one light ray per
 * light (lights_blocked, rt_anyhit.h) — the flag is a wave-uniform runtime branch, so flagged
 * and unflagged frames share these kernels.  Frames rendered while lights are set launch
 * these (launch_trace_lights); every other frame the plain or shadow kernels, whose code does
 * not move.
 *
 * The light records travel behind the frame's arguments in ONE by-value kernel argument,
 * KParamsL = KParams + LightArgs: inside this unit the shared device headers see KParamsL under
 * the name KParams, so every device function reads p.lights through the same scalar loads as
 * the rest of p and no signature in the shared headers changes. */
#define RT_LIGHTS 1
#include "rt_knobs.h"

namespace rt {
namespace klt {
struct KParamsL : rt::KParams {
    LightArgs lights;
};
static_assert(sizeof(KParamsL) <= 16384, "kernel arguments over 16 KB");
#define KParams KParamsL
#include "rt_scan_dev.h"
#include "rt_frame_dev.h"

/* The lights unit's launchers — the shadow unit's family: {F64, PATH64} x {linear, cull} x the
 * four depth tiers, F64 with the general pow() at the deepest tier only, each plain and
 * resolving (SS) — 36 kernels.  No sun, F32, pair, table or stamped variants. */
template <int PREC, bool INT_EXP, bool CULL, int MAXD, bool SS>
static void launch_one_lt(const KParams& p, dim3 grid, hipStream_t st, hipEvent_t done) {
    if (done)
        hipExtLaunchKernelGGL((k_trace<PREC, false, INT_EXP, CULL, MAXD, SS>), grid, dim3(BLOCK), 0, st,
                              nullptr, done, 0, p);
    else
        hipLaunchKernelGGL((k_trace<PREC, false, INT_EXP, CULL, MAXD, SS>), grid, dim3(BLOCK), 0, st, p);
}
template <int PREC, bool INT_EXP, bool CULL, bool SS>
static hipError_t launch_depth_lt(const KParams& p, dim3 grid, hipStream_t st, hipEvent_t done) {
    if constexpr (!INT_EXP) {
        launch_one_lt<PREC, false, CULL, MAXD_LARGE, SS>(p, grid, st, done);
    } else {
        if (p.depth <= MAXD_SMALL)
            launch_one_lt<PREC, true, CULL, MAXD_SMALL, SS>(p, grid, st, done);
        else if (p.depth <= MAXD_MID)
            launch_one_lt<PREC, true, CULL, MAXD_MID, SS>(p, grid, st, done);
        else if (p.depth <= MAXD_REF)
            launch_one_lt<PREC, true, CULL, MAXD_REF, SS>(p, grid, st, done);
        else
            launch_one_lt<PREC, true, CULL, MAXD_LARGE, SS>(p, grid, st, done);
    }
    return hipGetLastError();
}
template <int PREC, bool SS>
static hipError_t launch_prec_lt(const KParams& p, dim3 grid, hipStream_t st, hipEvent_t done) {
    // (PATH64's fp32 colour takes the exponent through v_log / v_exp either way)
    if (PREC == PREC_PATH64 || p.int_exp)
        return p.wave_cull ? launch_depth_lt<PREC, true, true, SS>(p, grid, st, done)
                           : launch_depth_lt<PREC, true, false, SS>(p, grid, st, done);
    if constexpr (PREC == PREC_F64)
        return p.wave_cull ? launch_depth_lt<PREC, false, true, SS>(p, grid, st, done)
                           : launch_depth_lt<PREC, false, false, SS>(p, grid, st, done);
    return hipErrorInvalidValue;
}
int launch_lights_ns(const KParams& p, int prec, void* stream, void* done_event) {
    if (p.W <= 0 || p.nrows <= 0) return (int)hipSuccess;
    if (p.depth < 0 || p.depth > MAXD_LARGE || (p.flags & FLAG_SUN)) return (int)hipErrorInvalidValue;
    if (p.lights.n < 1 || p.lights.n > MAX_LIGHTS) return (int)hipErrorInvalidValue;
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
        return (int)(prec == PREC_F64 ? launch_prec_lt<PREC_F64, true>(p, grid, st, done)
                                      : launch_prec_lt<PREC_PATH64, true>(p, grid, st, done));
    }
    return (int)(prec == PREC_F64 ? launch_prec_lt<PREC_F64, false>(p, grid, st, done)
                                  : launch_prec_lt<PREC_PATH64, false>(p, grid, st, done));
}
#undef KParams

}  // namespace klt

int launch_trace_lights(const KParams& p, const LightArgs& la, int prec, void* stream, void* done_event) {
    klt::KParamsL pl;
    static_cast<KParams&>(pl) = p;
    pl.lights = la;
    return klt::launch_lights_ns(pl, prec, stream, done_event);
}

}  // namespace rt
