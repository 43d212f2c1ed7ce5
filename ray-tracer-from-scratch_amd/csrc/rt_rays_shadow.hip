/* rt_rays_shadow.hip — the radiance kernels of rt_rays.hip built once more (namespace
 * rt::krs) with the light ray of RT_FLAG_SHADOWS in every segment: rt_trace_rays* with the
 * flag and an output launches these (launch_rays_shadow); hits-only calls, the occlusion
 * query and unflagged batches keep rt_rays.hip's kernels, whose code does not move. */
#define RT_SHADOW 1
#include "rt_knobs.h"

namespace rt {
namespace krs {
#include "rt_scan_dev.h"
#include "rt_rays_dev.h"
}  // namespace krs

/* Radiance with RT_FLAG_SHADOWS: {F64, PATH64} x {linear, cull} x the depth tiers and F64's
 * general pow() at the deepest tier — 18 kernels, no sun. */
int launch_rays_shadow(const KParams& p, const RayArgs& ra, int prec, void* stream, void* done_event) {
    using namespace krs;
    if (ra.n <= 0) return (int)hipSuccess;
    if (p.depth < 0 || p.depth > MAXD_LARGE) return (int)hipErrorInvalidValue;
    if (!ra.shade || p.out == nullptr || (p.flags & FLAG_SUN)) return (int)hipErrorInvalidValue;
    hipStream_t st = static_cast<hipStream_t>(stream);
    hipEvent_t done = static_cast<hipEvent_t>(done_event);
    if (prec == PREC_PATH64) return (int)rays_cull<PREC_PATH64, false, true>(p, ra, st, done);
    if (prec != PREC_F64) return (int)hipErrorInvalidValue;
    return (int)(p.int_exp ? rays_cull<PREC_F64, false, true>(p, ra, st, done)
                           : rays_cull<PREC_F64, false, false>(p, ra, st, done));
}

}  // namespace rt
