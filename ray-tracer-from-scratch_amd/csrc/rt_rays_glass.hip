/* rt_rays_glass.hip — the radiance kernels of rt_rays_lights.hip built once more (namespace
 * rt::krg) with the passage step of rt_set_transmission (rt_trace_glass.hip has the frame kernels
 * and the description): rt_trace_rays* with an output launches these while records are set
 * (launch_rays_glass), with or without lights and RT_FLAG_SHADOWS; hits-only calls and the
 * occlusion query keep rt_rays.hip's kernels, whose code does not move. */
#define RT_GLASS 1
#include "rt_knobs.h"

namespace rt {
namespace krg {
struct KParamsG : rt::KParams {
    LightArgs lights;
    GlassArgs glass;
};
static_assert(sizeof(KParamsG) <= 16384, "kernel arguments over 16 KB");
#define KParams KParamsG
#include "rt_scan_dev.h"
#include "rt_rays_dev.h"

/* Radiance with transmission (the lights unit's family): {F64, PATH64} x {linear, cull} x the depth tiers and F64's
 * general pow() at the deepest tier — 18 kernels, no sun. */
int launch_rays_glass_ns(const KParams& p, const RayArgs& ra, int prec, hipStream_t st, hipEvent_t done) {
    if (prec == PREC_PATH64) return (int)rays_cull<PREC_PATH64, false, true>(p, ra, st, done);
    if (prec != PREC_F64) return (int)hipErrorInvalidValue;
    return (int)(p.int_exp ? rays_cull<PREC_F64, false, true>(p, ra, st, done)
                           : rays_cull<PREC_F64, false, false>(p, ra, st, done));
}
#undef KParams
}  // namespace krg

int launch_rays_glass(const KParams& p, const RayArgs& ra, const LightArgs& la, const GlassArgs& ga, int prec,
                      void* stream, void* done_event) {
    if (ra.n <= 0) return (int)hipSuccess;
    if (p.depth < 0 || p.depth > krg::MAXD_LARGE) return (int)hipErrorInvalidValue;
    if (!ra.shade || p.out == nullptr || (p.flags & FLAG_SUN)) return (int)hipErrorInvalidValue;
    if (la.n < 1 || la.n > MAX_LIGHTS || ga.rec == nullptr) return (int)hipErrorInvalidValue;
    krg::KParamsG pg;
    static_cast<KParams&>(pg) = p;
    pg.lights = la;
    pg.glass = ga;
    return krg::launch_rays_glass_ns(pg, ra, prec, static_cast<hipStream_t>(stream),
                                      static_cast<hipEvent_t>(done_event));
}

}  // namespace rt
