/* rt_rays_lights.hip — the radiance kernels of rt_rays.hip built once more (namespace
 * rt::krl) with the scene lights of rt_set_lights (rt_trace_lights.hip has the frame kernels
 * and the reason for KParamsL): rt_trace_rays* with an output launches these while lights are
 * set (launch_rays_lights), with or without RT_FLAG_SHADOWS; hits-only calls and the occlusion
 * query keep rt_rays.hip's kernels, whose code does not move. */
#define RT_LIGHTS 1
#include "rt_knobs.h"

namespace rt {
namespace krl {
struct KParamsL : rt::KParams {
    LightArgs lights;
};
static_assert(sizeof(KParamsL) <= 16384, "kernel arguments over 16 KB");
#define KParams KParamsL
#include "rt_scan_dev.h"
#include "rt_rays_dev.h"

/* Radiance under the lights: {F64, PATH64} x {linear, cull} x the depth tiers and F64's
 * general pow() at the deepest tier — 18 kernels, no sun. */
int launch_rays_lights_ns(const KParams& p, const RayArgs& ra, int prec, hipStream_t st, hipEvent_t done) {
    if (prec == PREC_PATH64) return (int)rays_cull<PREC_PATH64, false, true>(p, ra, st, done);
    if (prec != PREC_F64) return (int)hipErrorInvalidValue;
    return (int)(p.int_exp ? rays_cull<PREC_F64, false, true>(p, ra, st, done)
                           : rays_cull<PREC_F64, false, false>(p, ra, st, done));
}
#undef KParams
}  // namespace krl

int launch_rays_lights(const KParams& p, const RayArgs& ra, const LightArgs& la, int prec, void* stream,
                       void* done_event) {
    if (ra.n <= 0) return (int)hipSuccess;
    if (p.depth < 0 || p.depth > krl::MAXD_LARGE) return (int)hipErrorInvalidValue;
    if (!ra.shade || p.out == nullptr || (p.flags & FLAG_SUN)) return (int)hipErrorInvalidValue;
    if (la.n < 1 || la.n > MAX_LIGHTS) return (int)hipErrorInvalidValue;
    krl::KParamsL pl;
    static_cast<KParams&>(pl) = p;
    pl.lights = la;
    return krl::launch_rays_lights_ns(pl, ra, prec, static_cast<hipStream_t>(stream),
                                      static_cast<hipEvent_t>(done_event));
}

}  // namespace rt
