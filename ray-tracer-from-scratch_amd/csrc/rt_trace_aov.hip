/* rt_trace_aov.hip — the kernel of rt_render_aov* (namespace rt::kav): the PRIMARY segment of a
 * frame, its closest hit written as per-pixel layers (rt_device.h AovArgs) instead of a colour.
 * The frame family's geometry — one 8x8 tile per wave, tile_row for the dispatch unit, band_row
 * for the band, partial tiles masked — and its primary segment: the ray generated in the kernel
 * (main.cpp:132-134), the primary pixel boxes, eye tables and wall order of the frame's
 * arguments, scan_d as trace_pixel_d calls it at bounce 0 (the linear scan, or the wave cull /
 * cluster walk of the scenes with RT_OPT_WAVE_CULL_MIN_SPHERES spheres or more).  No shading, no
 * bounce, no recursion stack, no LDS.  The record is written by rt_rays_dev.h's store_hit, so
 * its bytes are k_ray_hits' by construction; the derived layers are formed from the same
 * fields with the exact helpers (sqrt_e, rcp_refined / div_r: IEEE's bits, rt_selftest). */
#include "rt_knobs.h"

namespace rt {
namespace kav {
#include "rt_scan_dev.h"
#include "rt_frame_dev.h"
#include "rt_rays_dev.h"

/* The layers of one pixel (all but the record): pixel `px` of the band, hit h of ray r.  Which
 * layers exist is wave-uniform (kernel arguments).  A lane writes 4 bytes per scalar layer and
 * three 4-byte words per vector layer; a wave, 8 runs of 8 consecutive pixels per layer. */
__device__ __forceinline__ void store_layers(const KParams& p, const AovArgs& a, size_t px,
                                             const RayD& r, const HitD& h) {
    const bool hit = h.slot >= 0;
    if (a.index != nullptr) a.index[px] = hit ? scene_index(p, h.slot) : -1;
    if (a.depth != nullptr) {
        // world distance: a sphere's compared value is projection * |d| already (scene.cpp:77), a
        // wall's is the parameter t (scene.cpp:10)
        double z = __builtin_inf();
        if (hit) z = h.slot < p.nS ? h.dist : h.dist * r.dlen;
        a.depth[px] = (float)z;
    }
    if (a.normal != nullptr) {
        d3 nn = D3(0.0, 0.0, 0.0);
        if (hit) {
            d3 N;  // the record's normal (store_hit)
            if (h.slot < p.nS) {
                const double* S = p.s64[h.slot >> 2].v[h.slot & 3];
                N = (r.o + r.d * h.pt) - D3(S[0], S[1], S[2]);
            } else {
                N = ld3(p.w64[h.slot - p.nS].n);
            }
            nn = normalize_e(N);  // vec.cpp:21-24
        }
        float* o = a.normal + px * 3;
        o[0] = (float)nn.x;
        o[1] = (float)nn.y;
        o[2] = (float)nn.z;
    }
    if (a.albedo != nullptr) {
        d3 c = D3(0.0, 0.0, 0.0);
        if (hit) c = ld3(p.mat[h.slot].color);
        float* o = a.albedo + px * 3;
        o[0] = (float)c.x;
        o[1] = (float)c.y;
        o[2] = (float)c.z;
    }
}

/* One workgroup per dispatch unit and tile column, one 8x8 tile per wave (trace_grid's and
 * trace_tile's coordinates). */
template <bool CULL>
__global__ void __launch_bounds__(BLOCK) k_aov(KParams p, AovArgs a) {
    const int u = tile_row(p, blockIdx.y, (int)gridDim.y);
    const int ul = p.row_units_log2;
    const int bx = ((u & ((1 << ul) - 1)) * (int)gridDim.x) + (int)blockIdx.x;
    const int trow = u >> ul;
    const int lane = threadIdx.x & 63;
    const int wave = threadIdx.x >> 6;
    const int x = bx * TILE_W + (TILE_W > 8 ? (wave & 1) * 8 : 0) + (lane & 7);
    const BandRow br = band_row(p, trow, (TILE_H > 8 ? (wave >> 1) * 8 : 0) + (lane >> 3));
    const bool valid = x < p.W && br.ok;
    // the primary ray and the tile's keep mask, as trace_pixel_d forms them
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
    // every lane runs the (converged) scan; only valid lanes test and store
    const HitD h = scan_d<false, CULL, true>(p, r, valid, true, keep != ~0ull, keep);
    if (valid) {
        const size_t px = (size_t)br.out * (size_t)p.W + (size_t)x;
        if (a.hit != nullptr) store_hit(p, a.hit, px, r, h);
        store_layers(p, a, px, r, h);
    }
}

int launch_aov_ns(const KParams& p, const AovArgs& a, void* stream, void* done_event) {
    if (p.W <= 0 || p.nrows <= 0) return (int)hipSuccess;
    if (!a.hit && !a.index && !a.depth && !a.normal && !a.albedo) return (int)hipErrorInvalidValue;
    // contiguous bands of the caller's own frame, one pixel per lane, in row order or centre-out
    if (p.tstride > 1 || p.ss_log2 || p.row_units_log2 || p.row_perm_n) return (int)hipErrorInvalidValue;
    const dim3 grid((p.W + TILE_W - 1) / TILE_W, (p.nrows + TILE_H - 1) / TILE_H, 1);
    hipStream_t st = static_cast<hipStream_t>(stream);
    hipEvent_t done = static_cast<hipEvent_t>(done_event);
    auto kern = p.wave_cull ? k_aov<true> : k_aov<false>;
    if (done)
        hipExtLaunchKernelGGL(kern, grid, dim3(BLOCK), 0, st, nullptr, done, 0, p, a);
    else
        hipLaunchKernelGGL(kern, grid, dim3(BLOCK), 0, st, p, a);
    return (int)hipGetLastError();
}

}  // namespace kav

int launch_aov(const KParams& p, const AovArgs& a, void* stream, void* done_event) {
    return kav::launch_aov_ns(p, a, stream, done_event);
}

}  // namespace rt
