/* rt_knobs.h — what every kernel unit (rt_trace*.hip, rt_rays*.hip) starts with: the system
 * headers, rt_device.h, and the build knobs of the device code with their defaults.  A unit
 * defines RT_STAMP, RT_SHADOW, RT_LIGHTS or RT_GLASS before it where it wants those kernels.  Knobs that belong to
 * one function stand next to it in rt_scan_dev.h / rt_frame_dev.h. */
#include <hip/hip_ext.h>
#include <hip/hip_runtime.h>

#include <float.h>
#include <math.h>

#include <algorithm>
#include <type_traits>

#include "rt_device.h"

#ifndef RT_WALLS_FIRST
#define RT_WALLS_FIRST 1
#endif
#ifndef RT_WALL_NOSIGN     // 1: the wall test forms t = num/den for every lane and keeps t > 0 and
#define RT_WALL_NOSIGN 1   // t <= best in ONE branch, instead of a sign pre-test branch, then a
#endif                     // t > 0 branch, then the t-skip branch (fewer exec-mask instructions)
#ifndef RT_F32_WALL_FLAT   // F32 wall test without the sign pre-test branch: one branch per wall
#define RT_F32_WALL_FLAT 1
#endif
#ifndef RT_SPHERE_ONEBRANCH  // 1: Sphere::intersect's two early rejections (b > 0, det < 0)
#define RT_SPHERE_ONEBRANCH 1  // share one branch (det/4 formed for every lane: 2 VALU)
#endif
#ifndef RT_WALL_TSKIP      // 1: a wall whose t exceeds the current best skips its bounds
#define RT_WALL_TSKIP 1    // test (exact: the reference's strict < rejects it anyway);
#endif                     // fp64 paths only (the branch costs the fp32 path ~1% at c5)
#ifndef RT_TERMINAL_F32    // PATH64: the last segment of a path (sky, or the hit at max
#define RT_TERMINAL_F32 1  // depth) feeds colour only, so its normalisations run in fp32
#endif
#ifndef RT_LAZY_TERMS      // PATH64: |d|^2, 1/|d|^2, |d| only when a sphere test or a
#define RT_LAZY_TERMS 0    // reflection needs them (wave-uniform; A/B: +2% at c2, off)
#endif
#ifndef RT_PEEL           // 1: the primary segment peeled off the bounce loop (straight-line);
#define RT_PEEL 2          // 2: the first bounce too (c2 PATH64 -3%, F64 -4% over 1)
#endif
#ifndef RT_SKY_FAST        // PATH64/F32 linear scan: a tile whose keep mask is empty (no primitive's
#define RT_SKY_FAST 1      // pixel box meets it: every primary ray misses) shades its sky/ground
#endif                     // at once, without |d|^2, 1/|d|^2, |d| or the bounce loop
#ifndef RT_BOX_SCHED_BARRIER
#define RT_BOX_SCHED_BARRIER 1
#endif
#ifndef RT_CLUSTERS        // 1: cull kernels' wide-cone waves scan per-lane sphere clusters
#define RT_CLUSTERS 1
#endif
#ifndef RT_CLU_OCT         // 1: lanes walk their clusters in a per-octant near-to-far order
#define RT_CLU_OCT 1
#endif
#ifndef RT_CLUSTERS_F64    // 1: the same for the fp64-colour (F64, MIXED) cull kernels (A/B:
                           // c5 F64 -44%, MIXED -36%, c3 F64 -14.5%, MIXED -9%)
#define RT_CLUSTERS_F64 1
#endif
#ifndef RT_CLUSTERS_F32    // 1: the same for the F32 cull kernels
#define RT_CLUSTERS_F32 1
#endif
#ifndef RT_WALL_ORDER      // 1: the primary scan visits walls in the host's per-frame order
#define RT_WALL_ORDER 1    // (nearest to the camera first) when KParams::wall_order is set
#endif
#ifndef RT_UNWIND_KEND
#define RT_UNWIND_KEND 1
#endif
#ifndef RT_WAVE_TIMES      // diagnostic build: per-wave start/end stamps into KParams::stats
#define RT_WAVE_TIMES 0    // (tools/wave_times.py); never on in the product
#endif
#ifndef RT_STAGE_TIMES     // diagnostic build: shader-clock stamps at stage boundaries of every
#define RT_STAGE_TIMES 0   // wave into KParams::stats (tools/stage_times.py); never in the product
#endif
#if RT_STAGE_TIMES
#define STAGE(i) (g_stage[(i)] = __builtin_amdgcn_s_memtime())
#else
#define STAGE(i) \
    do {         \
    } while (0)
#endif
#ifndef RT_DIAG            // diagnostic build: count wave/lane entries of branch bodies
#define RT_DIAG 0          // into the unit's g_diag (rt_scan_dev.h; rt_diag_read reads the plain
#endif                     // unit's); never on in the product
#ifndef RT_STAMP
#define RT_STAMP 0  // 1 in rt_trace_stamp.hip: the same kernels, recording each wave's cost
#endif
#ifndef RT_SHADOW
#define RT_SHADOW 0 // 1 in rt_trace_shadow.hip (namespace rt::ksh) and rt_rays_shadow.hip (rt::krs):
#endif              // RT_FLAG_SHADOWS' kernels, a ray to the light at every hit (light_blocked)
#ifndef RT_GLASS
#define RT_GLASS 0  // 1 in rt_trace_glass.hip (namespace rt::kgl) and rt_rays_glass.hip (rt::krg):
#endif              // rt_set_transmission's kernels, the lights kernels with the passage step
#if RT_GLASS && !defined(RT_LIGHTS)
#define RT_LIGHTS 1
#endif
#ifndef RT_LIGHTS
#define RT_LIGHTS 0 // 1 in rt_trace_lights.hip (namespace rt::klt) and rt_rays_lights.hip (rt::krl):
#endif              // rt_set_lights' kernels, a loop over the scene lights at every hit
#if RT_DIAG
#define DIAG(i)                                                                    \
    do {                                                                            \
        const uint64_t b_ = __ballot(1);                                            \
        if ((uint64_t)__lane_id() == (uint64_t)__builtin_ctzll(b_)) {                \
            atomicAdd(&g_diag[(i)], 1ull);                                          \
            atomicAdd(&g_diag[(i) + 1], (unsigned long long)__popcll(b_));          \
        }                                                                           \
    } while (0)
#else
#define DIAG(i) \
    do {        \
    } while (0)
#endif
#ifndef RT_WPE_PATH64           // occupancy targets (rt_scan_dev.h waves_per_eu), A/B knobs
#define RT_WPE_PATH64 5
#endif
#ifndef RT_WPE_PATH64_CULL_BONUS  // PATH64 cull kernels, depth <= 8, no sun: 6 waves/SIMD (79
#define RT_WPE_PATH64_CULL_BONUS 1   // VGPRs, no scratch; A/B c5 -4.1%, c3 -6.1% vs 5, round 4)
#endif
#ifndef RT_WPE_MIXED_CULL_DROP  // MIXED cull kernels at depth > 4: one wave less
#define RT_WPE_MIXED_CULL_DROP 1
#endif
#ifndef RT_WPE_CULL64_BONUS  // F64/MIXED cull kernels: one wave/SIMD more since the recursion
#define RT_WPE_CULL64_BONUS 1    // stack moved to LDS (A/B: c5 F64 -3.5%, c3 F64 -5.6% vs 4 waves)
#endif
#ifndef RT_STACK_LDS      // 1: the cull kernels keep the recursion stack in LDS (trace_pixel_d)
#define RT_STACK_LDS 1
#endif
/* RT_AB_SLIM (A/B builds only, tools/build_variant.sh): instantiate the PATH64 no-sun
 * kernels of depth <= 8 alone (c1-c5's bench kernels), so an experiment compiles in a
 * fraction of the full family's time; any other launch fails with hipErrorInvalidValue. */
#ifndef RT_AB_SLIM
#define RT_AB_SLIM 0
#endif
