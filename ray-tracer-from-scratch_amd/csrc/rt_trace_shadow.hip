/* rt_trace_shadow.hip — the frame kernels of rt_trace.hip built once more (namespace
 * rt::ksh) with the light ray of RT_FLAG_SHADOWS in every segment (rt_scan_dev.h
 * light_blocked, rt_anyhit.h): the frames rendered with the flag launch these
 * (launch_trace_shadow), every other frame the plain kernels, whose code does not move. */
#define RT_SHADOW 1
#include "rt_knobs.h"

namespace rt {
namespace ksh {
#include "rt_scan_dev.h"
#include "rt_frame_dev.h"

/* The shadow unit's launchers: {F64, PATH64} x {linear, cull} x the four depth tiers, F64 with
 * the general pow() at the deepest tier only (as the ray kernels, rays_depth), each plain and
 * resolving (SS) — 36 kernels.  No sun, F32, pair, table or stamped variants. */
template <int PREC, bool INT_EXP, bool CULL, int MAXD, bool SS>
static void launch_one_sh(const KParams& p, dim3 grid, hipStream_t st, hipEvent_t done) {
    if (done)
        hipExtLaunchKernelGGL((k_trace<PREC, false, INT_EXP, CULL, MAXD, SS>), grid, dim3(BLOCK), 0, st,
                              nullptr, done, 0, p);
    else
        hipLaunchKernelGGL((k_trace<PREC, false, INT_EXP, CULL, MAXD, SS>), grid, dim3(BLOCK), 0, st, p);
}
template <int PREC, bool INT_EXP, bool CULL, bool SS>
static hipError_t launch_depth_sh(const KParams& p, dim3 grid, hipStream_t st, hipEvent_t done) {
    if constexpr (!INT_EXP) {
        launch_one_sh<PREC, false, CULL, MAXD_LARGE, SS>(p, grid, st, done);
    } else {
        if (p.depth <= MAXD_SMALL)
            launch_one_sh<PREC, true, CULL, MAXD_SMALL, SS>(p, grid, st, done);
        else if (p.depth <= MAXD_MID)
            launch_one_sh<PREC, true, CULL, MAXD_MID, SS>(p, grid, st, done);
        else if (p.depth <= MAXD_REF)
            launch_one_sh<PREC, true, CULL, MAXD_REF, SS>(p, grid, st, done);
        else
            launch_one_sh<PREC, true, CULL, MAXD_LARGE, SS>(p, grid, st, done);
    }
    return hipGetLastError();
}
template <int PREC, bool SS>
static hipError_t launch_prec_sh(const KParams& p, dim3 grid, hipStream_t st, hipEvent_t done) {
    // (PATH64's fp32 colour takes the exponent through v_log / v_exp either way)
    if (PREC == PREC_PATH64 || p.int_exp)
        return p.wave_cull ? launch_depth_sh<PREC, true, true, SS>(p, grid, st, done)
                           : launch_depth_sh<PREC, true, false, SS>(p, grid, st, done);
    if constexpr (PREC == PREC_F64)
        return p.wave_cull ? launch_depth_sh<PREC, false, true, SS>(p, grid, st, done)
                           : launch_depth_sh<PREC, false, false, SS>(p, grid, st, done);
    return hipErrorInvalidValue;
}
int launch_shadow_ns(const KParams& p, int prec, void* stream, void* done_event) {
    if (p.W <= 0 || p.nrows <= 0) return (int)hipSuccess;
    if (p.depth < 0 || p.depth > MAXD_LARGE || (p.flags & FLAG_SUN)) return (int)hipErrorInvalidValue;
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
        return (int)(prec == PREC_F64 ? launch_prec_sh<PREC_F64, true>(p, grid, st, done)
                                      : launch_prec_sh<PREC_PATH64, true>(p, grid, st, done));
    }
    return (int)(prec == PREC_F64 ? launch_prec_sh<PREC_F64, false>(p, grid, st, done)
                                  : launch_prec_sh<PREC_PATH64, false>(p, grid, st, done));
}

}  // namespace ksh

int launch_trace_shadow(const KParams& p, int prec, void* stream, void* done_event) {
    return ksh::launch_shadow_ns(p, prec, stream, done_event);
}

}  // namespace rt
