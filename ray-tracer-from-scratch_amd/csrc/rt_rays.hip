/* rt_rays.hip — the kernels of rt_trace_rays* and rt_occluded* (namespace rt::kry): radiance
 * and closest hits for a batch of caller rays (rt_rays_dev.h on top of rt_scan_dev.h; no frame
 * code), the pure find_closest_hit query, and the occlusion query, which has a scan of its own:
 * any-hit against a per-ray parametric limit, with a wave-uniform exit once every ray is
 * decided (rt_anyhit.h). */
#include "rt_knobs.h"

namespace rt {
namespace kry {
#include "rt_scan_dev.h"
#include "rt_rays_dev.h"

/* The pure find_closest_hit query: one segment per ray, no shading, no bounce. */
template <bool CULL>
__global__ void __launch_bounds__(BLOCK) k_ray_hits(KParams p, RayArgs ra) {
    const size_t ray = (size_t)blockIdx.x * BLOCK + threadIdx.x;
    const bool alive = ray < (size_t)ra.n;
    d3 o, d;
    load_ray(ra, ray, alive, o, d);
    const RayD r = make_ray(o, d);
    const HitD h = scan_d<false, CULL, true>(p, r, alive, false, false, ~0ull);
    if (alive) store_hit(p, ra.hits, ray, r, h);
    count_segments(p, alive ? 1 : 0);
}

/* ---- occlusion (rt_occluded*): any-hit on the segment o .. o + d * T ---------------------
 * sphere_blocks, wall_blocks and the three scans (rt_anyhit.h; the shadow units have them
 * from rt_scan_dev.h, for the light ray). */
#include "rt_anyhit.h"

/* One lane per ray; out[ray] = 1 where the segment is blocked, *count += the wave's blocked
 * rays (ballot popcount, one atomic per wave). */
template <bool CULL>
__global__ void __launch_bounds__(BLOCK) k_ray_occluded(KParams p, OccArgs oa) {
    const size_t ray = (size_t)blockIdx.x * BLOCK + threadIdx.x;
    const bool alive = ray < (size_t)oa.n;
    RayArgs ra;
    ra.org = oa.org;
    ra.dir = oa.dir;
    ra.hits = nullptr;
    ra.n = oa.n;
    ra.shade = 0;
    d3 o, d;
    load_ray(ra, ray, alive, o, d);
    double T = __builtin_inf();
    if (alive && oa.tmax != nullptr) T = oa.tmax[ray];
    const RayD r = make_ray(o, d);
    const bool open = alive && T > 0;  // NaN and T <= 0: never occluded
    bool todo = open;
    if (CULL)
        occluded_cull(p, r, todo, T);
    else
        occluded_linear(p, r, todo, T);
    const bool blocked = open && !todo;
    if (alive && oa.out != nullptr) oa.out[ray] = blocked ? 1 : 0;
    if (oa.count != nullptr) {
        const uint64_t m = __ballot(blocked);
        if ((threadIdx.x & 63) == 0 && m != 0)
            atomicAdd(oa.count, (unsigned long long)__popcll(m));
    }
}

}  // namespace kry

int launch_rays(const KParams& p, const RayArgs& ra, int prec, void* stream, void* done_event) {
    using namespace kry;
    if (ra.n <= 0) return (int)hipSuccess;
    if (p.depth < 0 || p.depth > MAXD_LARGE) return (int)hipErrorInvalidValue;
    hipStream_t st = static_cast<hipStream_t>(stream);
    hipEvent_t done = static_cast<hipEvent_t>(done_event);
    if (!ra.shade) {
        if (ra.hits == nullptr) return (int)hipErrorInvalidValue;
        return (int)(p.wave_cull ? launch_k(k_ray_hits<true>, p, ra, st, done)
                                 : launch_k(k_ray_hits<false>, p, ra, st, done));
    }
    if (p.out == nullptr) return (int)hipErrorInvalidValue;
    const bool sun = (p.flags & FLAG_SUN) != 0;
    if (prec == PREC_PATH64)  // fp32 colour: the exponent goes through v_log / v_exp either way
        return (int)(sun ? rays_cull<PREC_PATH64, true, true>(p, ra, st, done)
                         : rays_cull<PREC_PATH64, false, true>(p, ra, st, done));
    if (prec != PREC_F64) return (int)hipErrorInvalidValue;
    if (p.int_exp)
        return (int)(sun ? rays_cull<PREC_F64, true, true>(p, ra, st, done)
                         : rays_cull<PREC_F64, false, true>(p, ra, st, done));
    return (int)(sun ? rays_cull<PREC_F64, true, false>(p, ra, st, done)
                     : rays_cull<PREC_F64, false, false>(p, ra, st, done));
}

int launch_occluded(const KParams& p, const OccArgs& oa, void* stream, void* done_event) {
    using namespace kry;
    if (oa.n <= 0) return (int)hipSuccess;
    if (oa.out == nullptr && oa.count == nullptr) return (int)hipErrorInvalidValue;
    hipStream_t st = static_cast<hipStream_t>(stream);
    hipEvent_t done = static_cast<hipEvent_t>(done_event);
    const dim3 grid((unsigned)(((size_t)oa.n + BLOCK - 1) / BLOCK));
    auto kern = p.wave_cull ? k_ray_occluded<true> : k_ray_occluded<false>;
    if (done)
        hipExtLaunchKernelGGL(kern, grid, dim3(BLOCK), 0, st, nullptr, done, 0, p, oa);
    else
        hipLaunchKernelGGL(kern, grid, dim3(BLOCK), 0, st, p, oa);
    return (int)hipGetLastError();
}

}  // namespace rt
