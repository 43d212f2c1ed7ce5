/* rt_rays_shadow.hip — the radiance kernels of rt_rays.hip built once more (namespace
 * rt::krs) with the light ray of RT_FLAG_SHADOWS in every segment: rt_trace_rays* with the
 * flag and an output launches these (launch_rays_shadow); hits-only calls, the occlusion
 * query and unflagged batches keep rt_rays.hip's kernels, whose code does not move. */
#define RT_SHADOW 1
#include "rt_rays.hip"
