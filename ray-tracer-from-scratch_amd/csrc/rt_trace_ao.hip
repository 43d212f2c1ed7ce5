/* rt_trace_ao.hip — the kernel of rt_render_ao* (namespace rt::kao): ambient occlusion of a
 * frame's primary hits (rt_capi.h "ambient occlusion").  k_aov's geometry and primary segment —
 * one 8x8 tile per wave, tile_row / band_row, partial tiles masked, the ray generated in the
 * kernel, the primary pixel boxes, eye tables and wall order, scan_d at bounce 0 — then, at
 * every hit, ndirs any-hit probes of the hemisphere above the surface through rt_anyhit.h's
 * scans (the occlusion query's: linear, or the wave cone / cluster walk), and one byte and / or
 * one float per pixel.  No shading, no bounce, no LDS, no scratch.
 *
 * The probe directions are the same for every pixel: they travel by value behind the KParams
 * (AoArgs), are indexed by the wave-uniform loop counter and so arrive through scalar loads
 * like the scene records; |w|^2, its refined reciprocal and |w| are formed once per direction
 * from the caller's w (a sign flip changes none of their bits: x*x == (-x)*(-x)), only the flip
 * onto the pixel's hemisphere is per lane.
 *
 * A caller's direction may have components that are exactly 0 (an axis, rt_ao_directions' first
 * vector): the cluster boxes' slab planes are formed as (lo - o) * (1/d) in this unit
 * (RT_CLU_SLAB_FMA, rt_scan_dev.h), which keeps a box the ray runs through.  And a wave's
 * probes are +w_k in some lanes and -w_k in the others, so their unit directions can cancel
 * exactly: wave_cone checks its axis in this unit (RT_CONE_AXIS_CHECK) and falls back to no cone. */
#define RT_CLU_SLAB_FMA 0
#define RT_CONE_AXIS_CHECK 1
#include "rt_knobs.h"

namespace rt {
namespace kao {
#include "rt_scan_dev.h"
#include "rt_frame_dev.h"
#include "rt_anyhit.h"

/* One workgroup per dispatch unit and tile column, one 8x8 tile per wave (k_aov's coordinates). */
template <bool CULL>
__global__ void __launch_bounds__(BLOCK) k_ao(KParams p, AoArgs a) {
    const int u = tile_row(p, blockIdx.y, (int)gridDim.y);
    const int ul = p.row_units_log2;
    const int bx = ((u & ((1 << ul) - 1)) * (int)gridDim.x) + (int)blockIdx.x;
    const int trow = u >> ul;
    const int lane = threadIdx.x & 63;
    const int wave = threadIdx.x >> 6;
    const int x = bx * TILE_W + (TILE_W > 8 ? (wave & 1) * 8 : 0) + (lane & 7);
    const BandRow br = band_row(p, trow, (TILE_H > 8 ? (wave >> 1) * 8 : 0) + (lane >> 3));
    const bool valid = x < p.W && br.ok;
    // the primary ray and the tile's keep mask, as k_aov forms them
    const d3 cpos = ld3(p.pos);
    const d3 pc = (ld3(p.tl) + ld3(p.dx) * (double)x) + ld3(p.dy) * (double)br.i;  // main.cpp:132
    uint64_t braw = 0;
    if (!CULL)
        braw = box_load_primary(p);
    else if (RT_CULL_WALL_BINS && p.nwbox > 0)  // (wave-uniform: scenes with walls only)
        braw = box_load_walls(p);
    const RayD r = make_ray(cpos, cpos - pc);  // main.cpp:133-134 (direction not normalised)
    const TileO tile = tile_origin(x, br.i);
    uint64_t keep = ~0ull;
    if (!CULL) {
        if (p.nbox > 0) keep = box_keep(braw, tile);  // all lanes active
    } else if (RT_CULL_WALL_BINS && p.nwbox > 0) {
        keep = box_keep(braw, tile);  // the walls' boxes (bit w = wall w)
    }
    const HitD h = scan_d<false, CULL, true>(p, r, valid, true, keep != ~0ull, keep);
    const size_t px = (size_t)br.out * (size_t)p.W + (size_t)x;
    const bool open = valid && h.slot >= 0;
    if (!__any(open)) {  // wave-uniform: nothing to probe
        if (valid) {
            if (a.count != nullptr) a.count[px] = 0;
            if (a.ao != nullptr) a.ao[px] = 1.0f;
        }
        return;
    }
    // the probes' start point: the true surface point, lifted along the facing normal; lanes
    // without a hit carry a harmless ray and take part with todo == false
    d3 sp = D3(0.0, 0.0, 1.0);
    d3 nf = D3(0.0, 0.0, 1.0);
    if (open) {
        d3 P, N;
        if (h.slot < p.nS) {
            const double* S = p.s64[h.slot >> 2].v[h.slot & 3];
            P = r.o + r.d * h.pt;  // scene.cpp:75's intersection_point
            N = P - D3(S[0], S[1], S[2]);
        } else {
            P = r.o + r.d * h.dist;  // a wall's distance is its parameter (scene.cpp:10)
            N = ld3(p.w64[h.slot - p.nS].n);
        }
        const double f = dot(r.d, N);
        nf = f > 0 ? -N : N;
        sp = P + nf * .0001;  // main.cpp:111's offset
    }
    const double T = a.radius;
    int cnt = 0;
    for (int k = 0; k < a.ndirs; ++k) {  // converged: the cull scans' reductions need every lane
        const d3 wk = D3(a.dirs[k][0], a.dirs[k][1], a.dirs[k][2]);  // wave-uniform
        const double s = dot(wk, nf);
        RayD pr;
        pr.o = sp;
        pr.d = s < 0 ? -wk : wk;
        pr.a = lensq(wk);  // make_ray's bits for either sign
        pr.ra = rcp_refined(pr.a);
        pr.dlen = sqrt_e(pr.a);
        bool todo = open;
        if (CULL)
            occluded_cull(p, pr, todo, T);
        else
            occluded_linear(p, pr, todo, T);
        cnt += (open && !todo) ? 1 : 0;
    }
    if (valid) {
        if (a.count != nullptr) a.count[px] = (uint8_t)cnt;
        if (a.ao != nullptr) a.ao[px] = (float)((double)(a.ndirs - cnt) / (double)a.ndirs);
    }
}

int launch_ao_ns(const KParams& p, const AoArgs& a, void* stream, void* done_event) {
    if (p.W <= 0 || p.nrows <= 0) return (int)hipSuccess;
    if (!a.count && !a.ao) return (int)hipErrorInvalidValue;
    if (a.ndirs < 1 || a.ndirs > AO_MAX_DIRS || !(a.radius > 0)) return (int)hipErrorInvalidValue;
    // contiguous bands of the caller's own frame, one pixel per lane, in row order or centre-out
    if (p.tstride > 1 || p.ss_log2 || p.row_units_log2 || p.row_perm_n) return (int)hipErrorInvalidValue;
    const dim3 grid((p.W + TILE_W - 1) / TILE_W, (p.nrows + TILE_H - 1) / TILE_H, 1);
    hipStream_t st = static_cast<hipStream_t>(stream);
    hipEvent_t done = static_cast<hipEvent_t>(done_event);
    auto kern = p.wave_cull ? k_ao<true> : k_ao<false>;
    if (done)
        hipExtLaunchKernelGGL(kern, grid, dim3(BLOCK), 0, st, nullptr, done, 0, p, a);
    else
        hipLaunchKernelGGL(kern, grid, dim3(BLOCK), 0, st, p, a);
    return (int)hipGetLastError();
}

}  // namespace kao

int launch_ao(const KParams& p, const AoArgs& a, void* stream, void* done_event) {
    return kao::launch_ao_ns(p, a, stream, done_event);
}

}  // namespace rt
