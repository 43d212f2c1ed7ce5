/* rt_frame_dev.h — what a frame adds to rt_scan_dev.h's device code: the dispatch order of
 * tile rows, the tile and mirror bins, one pixel's path in fp64 (trace_pixel_d), two pixels per
 * lane (trace_pair_p64) and in fp32 (trace_pixel_f), band rows, the supersample resolve, a
 * wave's tile, a workgroup of the grid and the frame kernel k_trace.  Not a header of its own:
 * included inside the namespace of a frame unit (rt_trace.hip, rt_trace_stamp.hip,
 * rt_trace_shadow.hip, rt_trace_lights.hip, rt_trace_glass.hip) behind rt_scan_dev.h; the ray
 * units do not include it. */

/* Dispatch order of tile rows (workgroup row blockIdx.y -> tile row).  Per-tile cost is
 * very uneven (sky/ground tiles end after one segment, tiles over reflective walls bounce
 * to full depth), and a heavy wave dispatched late ends the kernel long after the last
 * light one: the dispatcher goes row by row, so rows are visited centre-out from the
 * host's estimate of the heaviest row (KParams::row_center, rt_capi.cpp) — heavy work
 * first, the cheap rows fill in around it.  Identity when row_center < 0. */
// Wave-start loads.  1: no early return before the trace (a workgroup past the end of a
// row part runs with every lane invalid) and the primary box load is unconditional, so it
// no longer waits on nbox (A/B: c2 PATH64 -0.1..1.3%, F32 -1.3..2.6%, c1 -1..4.5%, c3
// +-0.6%).  2: also every wave-start kernel-argument value in ONE batch with one wait,
// pinned by an empty asm (A/B: c2 PATH64 +15%, F64 +7% — slower, off).
#ifndef RT_EARLY_LOADS
#define RT_EARLY_LOADS 1
#endif
__device__ __forceinline__ uint32_t row_perm_word(const KParams& p, int j) {
    return reinterpret_cast<const uint32_t*>(p.row_perm)[min(j >> 1, ROW_PERM_MAX / 2 - 1)];
}
/* c = row_center, rpn = row_perm_n, w = row_perm_word(j): the loaded values */
__device__ __forceinline__ int tile_row_of(int c, int rpn, uint32_t w, int j, int n) {
    const int L = min(c, n - 1 - c);  // rows c-L .. c+L alternate
    const int d = (j + 1) >> 1;
    const int alt = (j & 1) ? c + d : c - d;
    const int e = j - 2 * L;  // one side is exhausted: continue on the other
    const int rest = (c - L == 0) ? c + L + e : c - L - e;
    int t = j <= 2 * L ? alt : rest;
    t = (c < 0 || c >= n) ? j : t;
    const int pj = (int16_t)((j & 1) ? (w >> 16) : (w & 0xffff));
    return rpn == n ? pj : t;
}
__device__ __forceinline__ int tile_row(const KParams& p, int j, int n) {
    // branch-free (scalar selects), so that its kernel-argument loads — including the dword
    // holding entry j of an explicit order (a 16-bit load would be a vector load) — issue in
    // the wave's first batch instead of one dependent round trip after another
    return tile_row_of(p.row_center, p.row_perm_n, row_perm_word(p, j), j, n);
}

__device__ __forceinline__ uint64_t uniform64(uint64_t v) {
    const unsigned lo = __builtin_amdgcn_readfirstlane((unsigned)v);
    const unsigned hi = __builtin_amdgcn_readfirstlane((unsigned)(v >> 32));
    return ((uint64_t)hi << 32) | lo;
}
/* The primitives whose pixel box meets this wave's 8x8 tile (rt_device.h PrimBox): lane l
 * tests box l, one ballot.  box_load issues the load (early, so its latency hides behind
 * ray generation), box_keep does the branch-free compare and the ballot.  All lanes
 * active. */
__device__ __forceinline__ uint64_t box_load(const KParams& p, const PrimBox* boxes) {
    const int l = threadIdx.x & 63;
    const uint64_t v = *reinterpret_cast<const uint64_t*>(boxes + (l < p.nbox ? l : 0));
    return l < p.nbox ? v : 0x80007fff80007fffull;  // x0 = i0 = 32767 > x1 = i1: never meets
}
/* Pixel origin of the wave's 8x8 tile from a lane's own pixel (every wave covers an 8x8
 * square, lane = 8 * row + column): wave-uniform, independent of how tiles map to
 * workgroups. */
struct TileO {
    int x0, y0;
};
__device__ __forceinline__ TileO tile_origin(int x, int i) {
    const int lane = threadIdx.x & 63;
    return {__builtin_amdgcn_readfirstlane(x - (lane & 7)),
            __builtin_amdgcn_readfirstlane(i - (lane >> 3))};
}
/* The primary boxes: p.box always holds BIN_MAX_PRIMS (= 64) entries, so lane l's load is
 * in bounds whatever nbox is; the select after it needs nbox, the load does not. */
__device__ __forceinline__ uint64_t box_load_primary(const KParams& p) {
    static_assert(BIN_MAX_PRIMS == 64, "one box per lane");
    const int l = threadIdx.x & 63;
    const uint64_t v = *reinterpret_cast<const uint64_t*>(p.box + l);
    return l < p.nbox ? v : 0x80007fff80007fffull;
}
/* The cull kernels' wall boxes (RT_CULL_WALL_BINS): p.box[0 .. nwbox-1] = walls 0.. */
__device__ __forceinline__ uint64_t box_load_walls(const KParams& p) {
    const int l = threadIdx.x & 63;
    const uint64_t v = *reinterpret_cast<const uint64_t*>(p.box + l);
    return l < p.nwbox ? v : 0x80007fff80007fffull;
}
__device__ __forceinline__ uint64_t box_keep(uint64_t raw, TileO t) {
    const int x0 = (int16_t)(raw & 0xffff), x1 = (int16_t)((raw >> 16) & 0xffff);
    const int i0 = (int16_t)((raw >> 32) & 0xffff), i1 = (int16_t)(raw >> 48);
    const bool hit = (x0 <= t.x0 + 7) & (x1 >= t.x0) & (i0 <= t.y0 + 7) & (i1 >= t.y0);
    return uniform64(__ballot(hit));
}
__device__ __forceinline__ uint64_t tile_keep(const KParams& p, const PrimBox* boxes, TileO t) {
    return box_keep(box_load(p, boxes), t);
}

/* Bounce k <= mir_depth after chains of wall hits (rt_device.h "mirror bins"): a lane whose
 * previous k segments hit walls w1..wk has a ray of the camera mirrored along that chain,
 * so it can only hit primitives whose box for that chain meets the tile.  The wave's keep
 * mask is the union over the distinct chains its live lanes followed (at most
 * RT_MIR_CHAINS of them; more, or a sphere anywhere in a chain, returns ~0 = scan all).
 * st_m: the lane's material-slot stack (valid where alive).  All lanes active; k
 * wave-uniform. */
#ifndef RT_MIR_CHAINS
#define RT_MIR_CHAINS 1  // A/B: 4 chains = the same speed at c2, more SALU
#endif
template <int MAXD>
__device__ __forceinline__ uint64_t mirror_keep(const KParams& p, bool alive, const int* st_m,
                                                int k, TileO t) {
    uint64_t todo = uniform64(__ballot(alive));
    if (todo == 0 || k > p.mir_depth) return ~0ull;
    uint64_t keep = 0;
    for (int c = 0; c < RT_MIR_CHAINS; ++c) {
        const int l0 = __builtin_ctzll(todo);
        bool same = alive;
        int q = 0, off = 0, lvl = 1;
#pragma unroll
        for (int j = 0; j < MIR_MAX_DEPTH && j < MAXD; ++j) {
            if (j < k) {
                const int sj = __builtin_amdgcn_readlane(st_m[j], l0);
                if (sj < p.nS) return ~0ull;  // a sphere bounce: no linear mirror
                same = same && st_m[j] == sj;
                q = q * p.nW + (sj - p.nS);
                if (j > 0) off += lvl;
                lvl *= p.nW;
            }
        }
        keep |= tile_keep(p, p.mbox + (off + q) * p.nbox, t);
        todo &= ~uniform64(__ballot(same));
        if (todo == 0) return keep;
    }
    return ~0ull;
}

/* One pixel on the exact fp64 ray path.  COLOR64: colour arithmetic in fp64 too (F64 /
 * MIXED, the parity modes); otherwise in fp32 (PATH64). */
template <bool MIXED, bool COLOR64, bool SUN, bool INT_EXP, bool CULL, int MAXD>
__device__ __forceinline__ d3 trace_pixel_d(const KParams& p, int x, int i, bool alive,
                                            int& segs, uint64_t& t_start, uint64_t braw_in,
                                            uint64_t* g_stage = nullptr) {
    using CT = typename std::conditional<COLOR64, double, float>::type;
    const d3 cpos = ld3(p.pos);
    const d3 pc = (ld3(p.tl) + ld3(p.dx) * (double)x) + ld3(p.dy) * (double)i;  // main.cpp:132
    uint64_t braw = 0;
    if (!CULL)
        braw = RT_EARLY_LOADS >= 2 ? braw_in : RT_EARLY_LOADS ? box_load_primary(p) : box_load(p, p.box);
    else if (RT_CULL_WALL_BINS && p.nwbox > 0)  // (wave-uniform: scenes with walls only)
        braw = box_load_walls(p);
    // main.cpp:133-134 (direction not normalised); the sphere terms only where needed
    // (PATH64: the fp32 terminal segment needs none of them)
    constexpr bool LAZY = RT_LAZY_TERMS && !COLOR64 && !CULL && RT_TERMINAL_F32;
    constexpr bool SKYF = RT_SKY_FAST && !COLOR64 && !CULL && RT_TERMINAL_F32;
    RayD r = (LAZY || SKYF) ? make_ray_lazy(cpos, cpos - pc) : make_ray(cpos, cpos - pc);
    bool terms = !LAZY;
    STAGE(1);
    constexpr bool sun = SUN;
    // the wave's start stamp for the dispatch-order feedback (stamped build only): here,
    // between ray generation and the box compare's wait on its load
    t_start = RT_STAMP ? __builtin_amdgcn_s_memtime() : 0;
    if (RT_BOX_SCHED_BARRIER) __builtin_amdgcn_sched_barrier(0);  // compare after ray gen
    const TileO tile = tile_origin(x, i);
    uint64_t keep = ~0ull;
    if (!CULL) {
        keep = box_keep(braw, tile);  // all lanes active
        if (p.nbox == 0) keep = ~0ull;
    } else if (RT_CULL_WALL_BINS && p.nwbox > 0) {  // (wave-uniform)
        keep = box_keep(braw, tile);  // the walls' boxes (bit w = wall w)
    }
    STAGE(6);
    if (SKYF) {
        if (keep == 0) {  // wave-uniform: every primary ray of the tile misses (tile bins)
            f3 c = F3(0.f, 0.f, 0.f);
            if (alive) {
                ++segs;
                c = sky32(r.d);
            }
            STAGE(2);
            STAGE(3);
            STAGE(4);
            return D3(c.x, c.y, c.z);
        }
        if (!LAZY) ray_terms(r);
    }
    const uint64_t smask = p.nS >= 64 ? ~0ull : (1ull << p.nS) - 1;

    // The register stack of the recursion (per level: shading scalar, sun scalar, material
    // slot).  In the cull kernels (deep configs) it lives in LDS instead (RT_STACK_LDS): a
    // VGPR array indexed by the runtime bounce counter costs a select per element on every
    // push and holds 2-3 VGPRs per level for the whole bounce loop, which is what the deep
    // fp64 kernels spilled to scratch.  LDS: one ds_write per value per bounce, one read
    // per level in the unwind, [level][lane] so a wave's accesses are conflict-free.
    constexpr bool LSTK = RT_STACK_LDS >= 2 || (RT_STACK_LDS && CULL);  // 2: every kernel
    __shared__ CT lds_s[LSTK ? MAXD * BLOCK : 1];
    __shared__ CT lds_k[(LSTK && SUN) ? MAXD * BLOCK : 1];
    __shared__ int lds_m[LSTK ? MAXD * BLOCK : 1];
    CT st_s[LSTK ? 1 : MAXD];
    CT st_k[LSTK ? 1 : MAXD];
    int st_m[LSTK ? 1 : MAXD];
    const int tid = (int)threadIdx.x;
    auto push = [&](int k, CT sv, CT kv, int mv) __attribute__((always_inline)) {
        if constexpr (LSTK) {
            lds_s[k * BLOCK + tid] = sv;
            if (SUN) lds_k[k * BLOCK + tid] = kv;
            lds_m[k * BLOCK + tid] = mv;
        } else {
            st_s[k] = sv;
            st_k[k] = kv;
            st_m[k] = mv;
        }
    };
    auto ld_s = [&](int q) __attribute__((always_inline)) -> CT {
        if constexpr (LSTK) return lds_s[q * BLOCK + tid]; else return st_s[q];
    };
    auto ld_k = [&](int q) __attribute__((always_inline)) -> CT {
        if constexpr (LSTK) return SUN ? lds_k[q * BLOCK + tid] : (CT)0; else return st_k[q];
    };
    auto ld_m = [&](int q) __attribute__((always_inline)) -> int {
        if constexpr (LSTK) return lds_m[q * BLOCK + tid]; else return st_m[q];
    };
#if RT_LIGHTS
    // Coloured lights: a level keeps acc[c] + ka per channel (shade_lights_*) instead of the
    // scalar s.  Three values per level are 6 VGPRs in fp64, so this part of the stack lives
    // in LDS in every lights kernel ([channel][level][lane], conflict-free as lds_s); the
    // material slots keep their place (registers where mirror_keep reads them).
    __shared__ CT lds_l[3 * MAXD * BLOCK];
    auto push_l = [&](int k, CT vx, CT vy, CT vz, int mv) __attribute__((always_inline)) {
        lds_l[(0 * MAXD + k) * BLOCK + tid] = vx;
        lds_l[(1 * MAXD + k) * BLOCK + tid] = vy;
        lds_l[(2 * MAXD + k) * BLOCK + tid] = vz;
        if constexpr (LSTK) lds_m[k * BLOCK + tid] = mv; else st_m[k] = mv;
    };
    auto ld_l = [&](int c, int q) __attribute__((always_inline)) -> CT {
        return lds_l[(c * MAXD + q) * BLOCK + tid];
    };
#endif
    int n = 0;
    d3 c64 = D3(0, 0, 0);
    f3 c32 = F3(0.f, 0.f, 0.f);
    // One segment (one closest-hit query per live lane) at bounce k.  Converged: lanes
    // whose path ended stay (alive == false) so the wave can reduce over its live rays; k
    // is wave-uniform.
    auto segment = [&](const int k) __attribute__((always_inline)) {
        // tile bins: the primary segment, and the first bounce when the whole wave
        // reflected off one wall (both wave-uniform)
        uint64_t km = ~0ull;
        if (!CULL && k == 0 && p.nbox > 0) km = keep;
#if !RT_GLASS  // (a ray that passed through a pane did not reflect off it: no mirrored camera)
        if (!CULL && k >= 1 && k <= p.mir_depth) km = mirror_keep<MAXD>(p, alive, st_m, k, tile);
#endif
        if (CULL && RT_CULL_WALL_BINS && k == 0) km = keep;  // ~0 when the walls have no boxes
        if (LAZY && !terms && (km & smask) != 0) {  // a sphere may be tested
            ray_terms(r);
            terms = true;
        }
#if RT_DIAG
        if (k >= 1 && __any(alive)) {
            if (km != ~0ull) DIAG(12);
            else DIAG(14);
        }
#endif
        const HitD h = scan_d<MIXED, CULL, !COLOR64 || RT_CLUSTERS_F64>(p, r, alive, k == 0, km != ~0ull, km);
        if (k == 0) STAGE(2);
        const bool last = k >= p.depth || k >= MAXD;  // remaining_iterations <= 0 (main.cpp:105)
        if (LAZY && !terms && __any(alive && !last && h.slot >= 0)) {  // a reflection follows
            ray_terms(r);
            terms = true;
        }
#if RT_SHADOW
        // the light ray of every lane that hit, while the wave is still converged; not a
        // counted segment.  A shadowed hit has diffuse = specular = 0: s = 0*kd + 0*ks + ka
        const bool dark = light_blocked<CULL>(p, r, h, alive);
#endif
#if RT_LIGHTS
        // the light rays of every lane that hit (RT_FLAG_SHADOWS: a runtime branch), one
        // any-hit scan per light while the wave is still converged; bit l = light l is hidden
        const unsigned dark = lights_blocked<CULL>(p, r, h, alive);
#endif
        if (!alive) return;
        ++segs;
        if (!COLOR64 && RT_TERMINAL_F32 && (last || h.slot < 0)) {
            // PATH64, last segment of the path: nothing here feeds another ray
            DIAG(10);
            if (h.slot < 0) {
                c32 = sky32(r.d);
            } else {
                const f3 nv32 = fnormalize(tof(r.d));
                const d3 pos = r.o + r.d * h.dist;
                f3 N32;
                if (h.slot < p.nS) {
                    const double* S = p.s64[h.slot >> 2].v[h.slot & 3];
                    N32 = tof((r.o + r.d * h.pt) - D3(S[0], S[1], S[2]));
                } else {
                    N32 = tof(ld3(p.w64[h.slot - p.nS].n));
                }
                const DevMat32& m32 = p.mat32[h.slot];
#if RT_LIGHTS
                c32 = mul3(m32.color, shade_lights_f(p, m32, pos, fnormalize(N32), nv32, dark));
#else
                const float2 sh = shade_f(m32, tof(pos), fnormalize(N32), nv32, sun);
#if RT_SHADOW
                c32 = local_color_f(m32, dark ? m32.ka : sh.x, sh.y, sun);
#else
                c32 = local_color_f(m32, sh.x, sh.y, sun);
#endif
#endif
            }
            alive = false;
            return;
        }
        DIAG(8);
        const double rdl = rcp_refined(r.dlen);
        const d3 nv = div3(r.d, r.dlen, rdl);  // normalize(d); normalize(-d) == -nv
        if (h.slot < 0) {
            if (COLOR64) {
                c64 = sky_d(r, nv.z);
            } else if (r.d.z < 0.0) {
                c32 = F3(0.025f, 0.05f, 0.075f);
            } else {
                const float tz = fsqrt(fsqrt((float)nv.z));
                c32 = F3(fmaf(tz, 0.14f - 0.36f, 0.36f), fmaf(tz, 0.21f - 0.45f, 0.45f),
                         fmaf(tz, 0.49f - 0.57f, 0.57f));
            }
            alive = false;
            return;
        }
        const d3 pos = r.o + r.d * h.dist;  // main.cpp:99 (sphere world distance used as t)
        d3 N;
        if (h.slot < p.nS) {
            const double* S = p.s64[h.slot >> 2].v[h.slot & 3];
            N = (r.o + r.d * h.pt) - D3(S[0], S[1], S[2]);  // un-normalised, length r
        } else {
            N = ld3(p.w64[h.slot - p.nS].n);
        }
        const DevMat& m = p.mat[h.slot];
        // normalize(N): a wall's is a scene constant (host, same IEEE operations); the MIXED
        // cull kernels keep recomputing it (the select costs them 4 VGPRs and a wave/SIMD)
        const d3 nn = (h.slot < p.nS || (MIXED && CULL)) ? normalize_e(N)
                                                           : ld3(p.wnn[h.slot - p.nS]);
#if RT_LIGHTS
        // acc[c] + ka per channel; local = color * that, at push and at unwind alike
        CT vx, vy, vz;
        if constexpr (COLOR64) {
            const d3 v = shade_lights_d<INT_EXP>(p, m, pos, nn, -nv, dark);
            vx = v.x, vy = v.y, vz = v.z;
        } else {
            const f3 v = shade_lights_f(p, p.mat32[h.slot], pos, tof(nn), tof(nv), dark);
            vx = v.x, vy = v.y, vz = v.z;
        }
        if (last) {
            if constexpr (COLOR64)
                c64 = mul3(m.color, D3(vx, vy, vz));
            else
                c32 = mul3(p.mat32[h.slot].color, F3(vx, vy, vz));
            alive = false;
            return;
        }
        push_l(k, vx, vy, vz, h.slot);
#else
        CT s, ks;
        if (COLOR64) {
            const ShadeD sh = shade_d<INT_EXP>(m, pos, nn, -nv, sun);
            s = sh.s;
            ks = sh.ksun;
        } else {
            const float2 sh = shade_f(p.mat32[h.slot], tof(pos), tof(nn), tof(nv), sun);
            s = sh.x;
            ks = sh.y;
        }
#if RT_SHADOW
        if (dark) s = COLOR64 ? (CT)m.ka : (CT)p.mat32[h.slot].ka;
#endif
        if (last) {
            if (COLOR64)
                c64 = local_color_d(m, s, ks, sun);
            else
                c32 = local_color_f(p.mat32[h.slot], s, ks, sun);
            alive = false;
            return;
        }
        push(k, s, ks, h.slot);
#endif
        n = k + 1;
#if RT_GLASS
        // rt_set_transmission: a transmissive hit goes on with the ray that passes through
        const DevGlass& gl = p.glass.rec[h.slot];
        if (gl.tau > 0) {
            const NextRay nr = glass_next(p, gl, r, h, pos, N, nv, nn);
            if (LAZY) {
                r = make_ray_lazy(nr.o, nr.d);
                terms = false;
            } else {
                r = make_ray(nr.o, nr.d);
            }
            return;
        }
#endif
        // start + reflect(d, N) (main.cpp:111-113, vec.cpp:51-57)
        const double cc = 2 * dot(nv, nn);
        if (LAZY) {
            r = make_ray_lazy(pos + N * .0001, nv - nn * cc);
            terms = false;
        } else {
            r = make_ray(pos + N * .0001, nv - nn * cc);
        }
        };
    // The primary segment is peeled off the bounce loop (RT_PEEL): it runs as straight-line
    // code with k == 0 folded, so the loop's phi copies and control are only paid by waves
    // that bounce.
    int kend = 0;  // wave-uniform: bounce iterations run (every lane's n <= kend)
    if (RT_PEEL >= 2) {
        if (__any(alive)) {
            segment(0);
            if (!__any(alive)) {
                kend = 1;
            } else {
                segment(1);
                for (int k = 2;; ++k) {
                    if (!__any(alive)) {
                        kend = k;
                        break;
                    }
                    segment(k);
                }
            }
        }
    } else if (RT_PEEL) {
        if (__any(alive)) {
            segment(0);
            for (int k = 1;; ++k) {
                if (!__any(alive)) {
                    kend = k;
                    break;
                }
                segment(k);
            }
        }
    } else {
        for (int k = 0;; ++k) {
            if (!__any(alive)) {
                kend = k;
                break;
            }
            segment(k);
        }
    }
    STAGE(3);
    for (int q = MAXD - 1; q >= 0; --q) {
        if ((!RT_UNWIND_KEND || q < kend) && q < n) {  // uniform test: levels no lane reached
            const int mq = ld_m(q);
            const DevMat& m = p.mat[mq];
#if RT_LIGHTS
            if constexpr (COLOR64) {
                const d3 L = mul3(m.color, D3(ld_l(0, q), ld_l(1, q), ld_l(2, q)));
#if RT_GLASS
                c64 = lerp(L, c64, p.glass.rec[mq].w);  // tau in metallic's place where tau > 0
#else
                c64 = lerp(L, c64, m.km);  // vec.cpp:45-49 via main.cpp:117
#endif
            } else {
                const DevMat32& m32 = p.mat32[mq];
                const f3 L = mul3(m32.color, F3(ld_l(0, q), ld_l(1, q), ld_l(2, q)));
#if RT_GLASS
                const float km = p.glass.rec[mq].wf;
#else
                const float km = m32.km;
#endif
                c32 = F3(fmaf(km, c32.x - L.x, L.x), fmaf(km, c32.y - L.y, L.y),
                         fmaf(km, c32.z - L.z, L.z));
            }
#else
            if (COLOR64) {
                const d3 L = local_color_d(m, ld_s(q), ld_k(q), sun);
                c64 = lerp(L, c64, m.km);  // vec.cpp:45-49 via main.cpp:117
            } else {
                const DevMat32& m32 = p.mat32[mq];
                const f3 L = local_color_f(m32, ld_s(q), ld_k(q), sun);
                const float km = m32.km;
                c32 = F3(fmaf(km, c32.x - L.x, L.x), fmaf(km, c32.y - L.y, L.y),
                         fmaf(km, c32.z - L.z, L.z));
            }
#endif
        }
    }
    STAGE(4);
    if (COLOR64) return c64;
    return D3(c32.x, c32.y, c32.z);
}

/* ------------------------------------------------------------------------ */
/* PATH64, two pixels per lane (RT_OPT_PIXEL_PAIRS)                          */
/* ------------------------------------------------------------------------ */
/* A wave traces a 16x8 tile: lane l holds pixel (x0 + l%8, i0 + l/8) and the pixel 8
 * columns to its right.  At c2 the primary pass issues about as many SALU, branch and
 * scalar-load instructions as VALU and a SIMD issues ~one instruction per
 * quad-cycle there; those are per-wave costs (the primitive's record, the loop, the
 * exec-mask bookkeeping of each test's branch), so two pixels per lane pay them once for
 * 128 pixels, and each test's two independent dependency chains share one branch.
 * Every test is trace_pixel_d's (PATH64: exact fp64 paths, fp32 colour) evaluated for
 * both pixels of the lane under ONE branch taken when either pixel needs its body; the
 * results are kept by predicated selects, so each pixel's hit, path and colour are
 * bitwise those of the one-pixel kernel (tested: test_pixel_pairs_bitwise). */
template <int MAXD>
struct PxS {  // one pixel's path state (its register stack lives in separate arrays: the
    RayD r;   // promotion of a dynamically indexed array to registers needs an array alloca)
    int n;
    f3 c;
    bool alive;
};


/* sphere_exact_oc's accept path for one pixel, branch-free given g (the early rejections
 * passed).  The x == 0 case of scene.cpp:64-66 folds in: sqrt(0) = 0 gives num == -dt
 * exactly, so q = div_r(num, a) is its pt and its proj is 2q (the reference's /a); for
 * x > 0 num <= 0 gives q <= 0, rejected by dist > 0 as sphere_exact_oc's num test does. */
__device__ __forceinline__ void sphere_accept(double dt, double x, bool g, int s, const RayD& r,
                                              HitD& h) {
    const bool x0 = x == 0;
    const double sq = sqrt_e(g && !x0 ? x : 1.0);
    const double num = -dt - (x0 ? 0.0 : sq);
    const double q = div_r(num, r.a, r.ra);
    const double dist = (x0 ? 2.0 * q : q) * r.dlen;  // world distance, scene.cpp:77
    const bool take = g && num > 0 && dist > 0 && dist < h.dist;
    h.dist = take ? dist : h.dist;
    h.pt = take ? q : h.pt;
    h.slot = take ? s : h.slot;
}
/* Sphere s for both pixels (spheres in index order: strict < keeps the earlier). */
template <int MAXD>
__device__ __forceinline__ void sphere_pair(const d3 oc0, double c0, const d3 oc1, double c1,
                                            int s, const PxS<MAXD>& a, const PxS<MAXD>& b,
                                            HitD& ha, HitD& hb) {
    const double dta = dot(a.r.d, oc0), dtb = dot(b.r.d, oc1);
    const double xa = dta * dta - a.r.a * c0, xb = dtb * dtb - b.r.a * c1;
    const bool ga = a.alive && !(dta > 0 || !(xa >= 0));
    const bool gb = b.alive && !(dtb > 0 || !(xb >= 0));
    if (ga || gb) {
        DIAG(2);
        sphere_accept(dta, xa, ga, s, a.r, ha);
        sphere_accept(dtb, xb, gb, s, b.r, hb);
    }
}
/* wall_exact's bounds test and take for one pixel, branch-free given g (t > 0, t <= best). */
__device__ __forceinline__ void wall_accept(const Wall64& Wl, int w, const KParams& p, double t,
                                            bool g, const RayD& r, const d3 P, HitD& h) {
    const d3 q = (r.o + r.d * t) - P;  // ray::at (scene.h:16) minus the corner
    const double px = dot(q, ld3(Wl.X));
    const double py = dot(q, ld3(Wl.Y));
    const bool inb = g && px >= 0 && px <= Wl.len && py >= 0 && py <= Wl.wid;
    bool take = inb && t < h.dist;
    if (inb && !take && t == h.dist && h.slot >= 0)  // tie: the lower scene index wins (rare)
        take = p.wall_j[w] < scene_index(p, h.slot);
    h.dist = take ? t : h.dist;
    h.slot = take ? p.nS + w : h.slot;
}
template <bool EYE, int MAXD>
__device__ __forceinline__ void wall_pair_px(const Wall64& Wl, int w, const KParams& p,
                                             const PxS<MAXD>& a, const PxS<MAXD>& b, HitD& ha,
                                             HitD& hb) {
    const d3 n = ld3(Wl.n);
    const d3 P = ld3(Wl.P);
    const double dena = dot(n, a.r.d), denb = dot(n, b.r.d);
    const double numa = EYE ? p.eye_w[w] : dot(P - a.r.o, n);
    const double numb = EYE ? p.eye_w[w] : dot(P - b.r.o, n);
    // as wall_exact (RT_WALL_NOSIGN, RT_WALL_TSKIP): t <= 0, NaN, +-inf and t > best fail
    const double ta = div_r_nz(numa, dena, rcp_refined(dena));
    const double tb = div_r_nz(numb, denb, rcp_refined(denb));
    const bool ga = a.alive && ta > 0 && !(ta > ha.dist);
    const bool gb = b.alive && tb > 0 && !(tb > hb.dist);
    if (ga || gb) {
        DIAG(6);
        wall_accept(Wl, w, p, ta, ga, a.r, P, ha);
        wall_accept(Wl, w, p, tb, gb, b.r, P, hb);
    }
}
template <bool EYE, int MAXD>
__device__ __forceinline__ void sphere_pair_idx(const KParams& p, int s, const PxS<MAXD>& a,
                                                const PxS<MAXD>& b, HitD& ha, HitD& hb) {
    if (EYE) {
        const double* E = p.eye_s[s];
        const d3 oc = D3(E[0], E[1], E[2]);
        sphere_pair(oc, E[3], oc, E[3], s, a, b, ha, hb);
    } else {
        const double* S = p.s64[s >> 2].v[s & 3];
        const d3 C = D3(S[0], S[1], S[2]);
        const d3 oca = a.r.o - C, ocb = b.r.o - C;
        sphere_pair(oca, lensq(oca) - S[3], ocb, lensq(ocb) - S[3], s, a, b, ha, hb);
    }
}
/* closest_hit_bin / closest_hit_d for both pixels of every lane (keep wave-uniform). */
template <bool EYE, int MAXD>
__device__ __forceinline__ void scan_pair_bin(const KParams& p, const PxS<MAXD>& a,
                                              const PxS<MAXD>& b, uint64_t keep, HitD& ha,
                                              HitD& hb) {
    uint64_t sm = p.nS >= 64 ? keep : keep & ((1ull << p.nS) - 1);
    while (sm) {
        const int s = __builtin_ctzll(sm);
        sm &= sm - 1;
        sphere_pair_idx<EYE>(p, s, a, b, ha, hb);
    }
    uint64_t wm = p.nS >= 64 ? 0 : keep >> p.nS;
    while (wm) {
        const int w = __builtin_ctzll(wm);
        wm &= wm - 1;
        wall_pair_px<EYE>(p.w64[w], w, p, a, b, ha, hb);
    }
}
template <bool EYE, int MAXD>
__device__ __forceinline__ void scan_pair_all(const KParams& p, const PxS<MAXD>& a,
                                              const PxS<MAXD>& b, HitD& ha, HitD& hb) {
    for (int s = 0; s < p.nS; ++s) sphere_pair_idx<EYE>(p, s, a, b, ha, hb);
    for (int w = 0; w < p.nW; ++w) wall_pair_px<EYE>(p.w64[w], w, p, a, b, ha, hb);
}

/* Tile bins for a 16-pixel-wide tile (box_keep's compare, one ballot). */
__device__ __forceinline__ uint64_t box_keep16(uint64_t raw, TileO t) {
    const int x0 = (int16_t)(raw & 0xffff), x1 = (int16_t)((raw >> 16) & 0xffff);
    const int i0 = (int16_t)((raw >> 32) & 0xffff), i1 = (int16_t)(raw >> 48);
    const bool hit = (x0 <= t.x0 + 15) & (x1 >= t.x0) & (i0 <= t.y0 + 7) & (i1 >= t.y0);
    return uniform64(__ballot(hit));
}
/* mirror_keep (RT_MIR_CHAINS = 1) over both pixels of every lane: the keep mask of the wall
 * chain that every live pixel of the wave followed, or ~0. */
template <int MAXD>
__device__ __forceinline__ uint64_t mirror_keep_pair(const KParams& p, const PxS<MAXD>& a,
                                                     const PxS<MAXD>& b, const int* ma,
                                                     const int* mb, int k, TileO t) {
    const uint64_t todo = uniform64(__ballot(a.alive || b.alive));
    if (todo == 0 || k > p.mir_depth) return ~0ull;
    const int l0 = __builtin_ctzll(todo);
    const bool lead_a = __builtin_amdgcn_readlane((int)a.alive, l0) != 0;
    bool same_a = true, same_b = true;
    int q = 0, off = 0, lvl = 1;
#pragma unroll
    for (int j = 0; j < MIR_MAX_DEPTH && j < MAXD; ++j) {
        if (j < k) {
            const int sj = __builtin_amdgcn_readlane(lead_a ? ma[j] : mb[j], l0);
            if (sj < p.nS) return ~0ull;  // a sphere bounce: no linear mirror
            same_a = same_a && ma[j] == sj;
            same_b = same_b && mb[j] == sj;
            q = q * p.nW + (sj - p.nS);
            if (j > 0) off += lvl;
            lvl *= p.nW;
        }
    }
    if (uniform64(__ballot((a.alive && !same_a) || (b.alive && !same_b))) != 0) return ~0ull;
    const int l = threadIdx.x & 63;
    const PrimBox* boxes = p.mbox + (off + q) * p.nbox;
    const uint64_t raw = *reinterpret_cast<const uint64_t*>(boxes + (l < p.nbox ? l : 0));
    return box_keep16(l < p.nbox ? raw : 0x80007fff80007fffull, t);
}

/* trace_pixel_d<PATH64>'s per-pixel work after the scan of segment k (the lambda's body). */
template <bool SUN, int MAXD>
__device__ __forceinline__ void pair_after_scan(const KParams& p, PxS<MAXD>& s, float* st_s,
                                                float* st_k, int* st_m, const HitD& h, int k,
                                                int& segs) {
    if (!s.alive) return;
    ++segs;
    const bool last = k >= p.depth || k >= MAXD;  // remaining_iterations <= 0 (main.cpp:105)
    if (last || h.slot < 0) {  // the path's last segment: colour only, in fp32
        if (h.slot < 0) {
            s.c = sky32(s.r.d);
        } else {
            const f3 nv32 = fnormalize(tof(s.r.d));
            const d3 pos = s.r.o + s.r.d * h.dist;
            f3 N32;
            if (h.slot < p.nS) {
                const double* S = p.s64[h.slot >> 2].v[h.slot & 3];
                N32 = tof((s.r.o + s.r.d * h.pt) - D3(S[0], S[1], S[2]));
            } else {
                N32 = tof(ld3(p.w64[h.slot - p.nS].n));
            }
            const DevMat32& m32 = p.mat32[h.slot];
            const float2 sh = shade_f(m32, tof(pos), fnormalize(N32), nv32, SUN);
            s.c = local_color_f(m32, sh.x, sh.y, SUN);
        }
        s.alive = false;
        return;
    }
    const double rdl = rcp_refined(s.r.dlen);
    const d3 nv = div3(s.r.d, s.r.dlen, rdl);  // normalize(d)
    const d3 pos = s.r.o + s.r.d * h.dist;     // main.cpp:99
    d3 N;
    if (h.slot < p.nS) {
        const double* S = p.s64[h.slot >> 2].v[h.slot & 3];
        N = (s.r.o + s.r.d * h.pt) - D3(S[0], S[1], S[2]);  // un-normalised, length r
    } else {
        N = ld3(p.w64[h.slot - p.nS].n);
    }
    const d3 nn = h.slot < p.nS ? normalize_e(N) : ld3(p.wnn[h.slot - p.nS]);
    const float2 sh = shade_f(p.mat32[h.slot], tof(pos), tof(nn), tof(nv), SUN);
    st_s[k] = sh.x;
    st_k[k] = sh.y;
    st_m[k] = h.slot;
    s.n = k + 1;
    const double cc = 2 * dot(nv, nn);
    s.r = make_ray(pos + N * .0001, nv - nn * cc);  // main.cpp:111-113
}

template <bool SUN, int MAXD>
__device__ __forceinline__ void trace_pair_p64(const KParams& p, int x, int i, bool va, bool vb,
                                               int& segs, uint64_t& t_start, f3& ca, f3& cb) {
    const d3 cpos = ld3(p.pos);
    const d3 pca = (ld3(p.tl) + ld3(p.dx) * (double)x) + ld3(p.dy) * (double)i;  // main.cpp:132
    const d3 pcb = (ld3(p.tl) + ld3(p.dx) * (double)(x + 8)) + ld3(p.dy) * (double)i;
    const uint64_t braw = box_load_primary(p);
    PxS<MAXD> a, b;
    float as_[MAXD], ak_[MAXD], bs_[MAXD], bk_[MAXD];
    int am_[MAXD], bm_[MAXD];
    a.r = make_ray_lazy(cpos, cpos - pca);  // main.cpp:133-134
    b.r = make_ray_lazy(cpos, cpos - pcb);
    a.alive = va;
    b.alive = vb;
    a.n = b.n = 0;
    a.c = b.c = F3(0.f, 0.f, 0.f);
    t_start = RT_STAMP ? __builtin_amdgcn_s_memtime() : 0;
    if (RT_BOX_SCHED_BARRIER) __builtin_amdgcn_sched_barrier(0);
    const TileO tile = tile_origin(x, i);
    uint64_t keep = box_keep16(braw, tile);
    if (p.nbox == 0) keep = ~0ull;
    if (keep == 0) {  // every primary ray of the 16x8 tile misses (sky fast path)
        if (va) {
            ++segs;
            a.c = sky32(a.r.d);
        }
        if (vb) {
            ++segs;
            b.c = sky32(b.r.d);
        }
        ca = a.c;
        cb = b.c;
        return;
    }
    ray_terms(a.r);
    ray_terms(b.r);
    auto segment = [&](const int k) __attribute__((always_inline)) {
        uint64_t km = ~0ull;
        if (k == 0 && p.nbox > 0) km = keep;
        if (k >= 1 && k <= p.mir_depth) km = mirror_keep_pair<MAXD>(p, a, b, am_, bm_, k, tile);
        HitD ha = no_hit(), hb = no_hit();
        const bool eye = k == 0 && p.eye;
        if (km != ~0ull) {
            if (eye)
                scan_pair_bin<true>(p, a, b, km, ha, hb);
            else
                scan_pair_bin<false>(p, a, b, km, ha, hb);
        } else {
            if (eye)
                scan_pair_all<true>(p, a, b, ha, hb);
            else
                scan_pair_all<false>(p, a, b, ha, hb);
        }
        pair_after_scan<SUN, MAXD>(p, a, as_, ak_, am_, ha, k, segs);
        pair_after_scan<SUN, MAXD>(p, b, bs_, bk_, bm_, hb, k, segs);
    };
    int kend = 0;  // wave-uniform: bounce iterations run
    if (__any(a.alive || b.alive)) {
        segment(0);
        if (!__any(a.alive || b.alive)) {
            kend = 1;
        } else {
            segment(1);
            for (int k = 2;; ++k) {
                if (!__any(a.alive || b.alive)) {
                    kend = k;
                    break;
                }
                segment(k);
            }
        }
    }
    // unwind (main.cpp:117 via vec.cpp:45-49), innermost bounce first
    for (int q = MAXD - 1; q >= 0; --q) {
        if (q < kend) {
            if (q < a.n) {
                const DevMat32& m = p.mat32[am_[q]];
                const f3 L = local_color_f(m, as_[q], ak_[q], SUN);
                a.c = F3(fmaf(m.km, a.c.x - L.x, L.x), fmaf(m.km, a.c.y - L.y, L.y),
                         fmaf(m.km, a.c.z - L.z, L.z));
            }
            if (q < b.n) {
                const DevMat32& m = p.mat32[bm_[q]];
                const f3 L = local_color_f(m, bs_[q], bk_[q], SUN);
                b.c = F3(fmaf(m.km, b.c.x - L.x, L.x), fmaf(m.km, b.c.y - L.y, L.y),
                         fmaf(m.km, b.c.z - L.z, L.z));
            }
        }
    }
    ca = a.c;
    cb = b.c;
}

/* ------------------------------------------------------------------------ */
/* fp32 throughput path                                                      */
/* ------------------------------------------------------------------------ */
/* fp32 sphere test (scaled form; det == 0 keeps scene.cpp:65's 2x distance).
 * IN_ORDER as for sphere_exact. */
template <bool IN_ORDER = true>
__device__ __forceinline__ void sphere_f(const float* S, int s, f3 o, f3 d, float a, float ra,
                                         float rl, float& best, float& bpt, int& slot,
                                         const KParams* p = nullptr) {
    const f3 oc = o - F3(S[0], S[1], S[2]);
    const float bh = fdot(d, oc);
    const float cq = fmaf(-S[3], S[3], fdot(oc, oc));
    const float det = fmaf(bh, bh, -a * cq);
    if (bh <= 0.0f && det >= 0.0f) {
        const float num = -bh - fsqrt(det);
        const float proj = (det == 0.0f) ? -2.0f * bh * ra : num * ra;
        const float dist = proj * a * rl;  // proj * |d|
        const bool ok = (det == 0.0f || num > 0.0f) && dist > 0.0f;
        bool take = ok && dist < best;
        if (!IN_ORDER && ok && !take && dist == best && slot >= 0)
            take = scene_index(*p, s) < scene_index(*p, slot);
        if (take) {
            best = dist;
            bpt = (det == 0.0f) ? -bh * ra : proj;
            slot = s;
        }
    }
}

/* clusters_scan for the F32 kernels: the same walk over the lane's own clusters with the
 * fp32 sphere test (sphere_f, scene-index tie rule); a pruned cluster's spheres lie at a
 * distance >= t_entry |d| > best (box margin 1e-3 x the scene extent). */
__device__ __forceinline__ void clusters_scan_f(const KParams& p, f3 o, f3 d, float a, float ra,
                                                float rl, bool alive, float& best, float& bpt,
                                                int& slot) {
    const SlabRay sr = slab_ray(o, d);
    const bool near = fmax3abs(o.x, o.y, o.z) <= p.clu_oinf;
    const int oct = clu_octant(d);
    uint64_t cm = 0;
    if (RT_CLU_FAST) {
        cm = p.nclu <= 32 ? clusters_mask<false, false>(p, sr, alive, near, oct)
                          : clusters_mask<false, true>(p, sr, alive, near, oct);
    } else {
        for (int c = 0; c < p.nclu; ++c) {
            const bool in = !near || slab_t(p.clu[c], sr) < __builtin_inff();
            cm |= (uint64_t)(alive && in) << c;
        }
    }
    const float dax = p.clu_axis == 0 ? d.x : (p.clu_axis == 1 ? d.y : d.z);
    const bool rev = dax < 0.0f;
    const float dl = a * rl;  // |d|
    while (__any(cm != 0)) {
        if (cm != 0) {
            const int c = rev ? 63 - __builtin_clzll(cm) : __builtin_ctzll(cm);
            cm &= ~(1ull << c);
            const float t = near ? slab_t(p.clu[c], sr) : 0.0f;
            if (t * dl * (1.0f - 1e-3f) <= best) {
                const CluSph* cs = p.csph + c * CLU_SIZE;
#pragma unroll
                for (int k = 0; k < CLU_SIZE; ++k) {
                    const int s = cs[k].slot;
                    if (s >= 0) sphere_f<false>(cs[k].f, s, o, d, a, ra, rl, best, bpt, slot, &p);
                }
            }
        }
    }
}

/* Two spheres (k0, k0+1 of group G) per packed fp32 instruction: the cheap prefix
 * (oc, b/2, c, det) runs as v_pk_* on {sphere k0, sphere k0+1}; the rare hit path
 * (sqrt, divide, compare) per sphere.  Same arithmetic as sphere_f, lane for lane. */
__device__ __forceinline__ void sphere_pair_f(const SphG32& G, int k0, int s0, int nS, f3 o,
                                              f3 d, float a, float ra, float rl, float& best,
                                              float& bpt, int& slot) {
    const f2 cx = {G.c[0][k0], G.c[0][k0 + 1]}, cy = {G.c[1][k0], G.c[1][k0 + 1]};
    const f2 cz = {G.c[2][k0], G.c[2][k0 + 1]}, rr = {G.c[3][k0], G.c[3][k0 + 1]};
    const f2 ocx = f2(o.x) - cx, ocy = f2(o.y) - cy, ocz = f2(o.z) - cz;
    const f2 bh = __builtin_elementwise_fma(
        f2(d.x), ocx, __builtin_elementwise_fma(f2(d.y), ocy, f2(d.z) * ocz));
    const f2 cq = __builtin_elementwise_fma(
        -rr, rr, __builtin_elementwise_fma(ocx, ocx, __builtin_elementwise_fma(ocy, ocy, ocz * ocz)));
    const f2 det = __builtin_elementwise_fma(bh, bh, -f2(a) * cq);
#pragma unroll
    for (int k = 0; k < 2; ++k) {
        if (s0 + k >= nS) break;
        const float b1 = bh[k], d1 = det[k];
        if (b1 <= 0.0f && d1 >= 0.0f) {
            const float num = -b1 - fsqrt(d1);
            const float proj = (d1 == 0.0f) ? -2.0f * b1 * ra : num * ra;
            const float dist = proj * a * rl;
            if ((d1 == 0.0f || num > 0.0f) && dist > 0.0f && dist < best) {
                best = dist;
                bpt = (d1 == 0.0f) ? -b1 * ra : proj;
                slot = s0 + k;
            }
        }
    }
}

/* A 64-byte record (Wall32, SphG32) as one s_load_dwordx16: the F32 cull kernels' walls and
 * cone survivors (see clusters_mask's box loads). */
template <class T>
__device__ __forceinline__ T rec64_sload(const T* q) {
    static_assert(sizeof(T) == 64, "one s_load_dwordx16");
    typedef int v16i __attribute__((ext_vector_type(16)));
    v16i a;
    asm volatile("s_load_dwordx16 %0, %1, 0x0\n\ts_waitcnt lgkmcnt(0)"
                 : "=s"(a)
                 : "s"(q)
                 : "memory");
    return __builtin_bit_cast(T, a);
}
template <bool SL = false>
__device__ __forceinline__ void walls_f(const KParams& p, f3 o, f3 d, float& best, int& slot,
                                        uint64_t wmask = ~0ull) {
    for (int w = 0; w < p.nW; ++w) {
        if (w < 64 && !((wmask >> w) & 1)) continue;  // wave-uniform (tile bins)
        const Wall32 Wl = SL ? rec64_sload(p.w32 + w) : p.w32[w];
        const f3 nw = F3(Wl.n[0], Wl.n[1], Wl.n[2]), P = F3(Wl.P[0], Wl.P[1], Wl.P[2]);
        const float den = fdot(nw, d);
        const float num = fdot(P - o, nw);
        // RT_F32_WALL_FLAT: no sign pre-test branch; t <= 0, NaN and inf fail below
        if (!RT_F32_WALL_FLAT && !((num > 0 && den > 0) || (num < 0 && den < 0))) continue;
        const float t = num * frcp(den);
        const f3 q = fmad3(d, t, o) - P;
        const float px = fdot(q, F3(Wl.X[0], Wl.X[1], Wl.X[2]));
        const float py = fdot(q, F3(Wl.Y[0], Wl.Y[1], Wl.Y[2]));
        const bool sgn = RT_F32_WALL_FLAT || ((num > 0 && den > 0) || (num < 0 && den < 0));
        if (sgn && t > 0 && px >= 0 && px <= Wl.len && py >= 0 && py <= Wl.wid) {
            bool take = t < best;
            if (!take && t == best && slot >= 0) take = p.wall_j[w] < scene_index(p, slot);
            if (take) {
                best = t;
                slot = p.nS + w;
            }
        }
    }
}

template <bool SUN, bool CULL, int MAXD>
__device__ __forceinline__ f3 trace_pixel_f(const KParams& p, int x, int i, bool alive,
                                            int& segs, uint64_t& t_start, uint64_t braw_in) {
    const d3 pcd = (ld3(p.tl) + ld3(p.dx) * (double)x) + ld3(p.dy) * (double)i;
    const d3 dd = ld3(p.pos) - pcd;
    f3 o = F3((float)p.pos[0], (float)p.pos[1], (float)p.pos[2]);
    f3 d = F3((float)dd.x, (float)dd.y, (float)dd.z);
    constexpr bool sun = SUN;

    float st_s[MAXD];
    float st_k[MAXD];
    int st_m[MAXD];
    int n = 0;
    f3 c = F3(0.f, 0.f, 0.f);
    t_start = RT_STAMP ? __builtin_amdgcn_s_memtime() : 0;  // see trace_pixel_d
    const TileO tile = tile_origin(x, i);
#if RT_EARLY_LOADS >= 2
    // unconditional compare (all lanes active), so the wave-start box load is not sunk
    uint64_t keep = CULL ? ~0ull : box_keep(braw_in, tile);
    if (p.nbox <= 0) keep = ~0ull;
#else
    const uint64_t keep = (!CULL && p.nbox > 0) ? tile_keep(p, p.box, tile) : ~0ull;
#endif
    // the cull kernels' primary walls behind their pixel boxes (RT_CULL_WALL_BINS)
    uint64_t wkeep = ~0ull;
    if (CULL && RT_CULL_WALL_BINS && p.nwbox > 0) wkeep = box_keep(box_load_walls(p), tile);
    if (!CULL && RT_SKY_FAST && keep == 0) {
        // wave-uniform: every primary ray misses (tile bins): the loop's miss shading below,
        // operation for operation, without the loop
        if (alive) {
            ++segs;
            const f3 nv = d * frsq(fdot(d, d));
            if (d.z < 0.0f) {
                c = F3(0.025f, 0.05f, 0.075f);
            } else {
                const float tz = fsqrt(fsqrt(nv.z));
                c = F3(fmaf(tz, 0.14f - 0.36f, 0.36f), fmaf(tz, 0.21f - 0.45f, 0.45f),
                       fmaf(tz, 0.49f - 0.57f, 0.57f));
            }
        }
        return c;
    }
    auto segment = [&](const int k) __attribute__((always_inline)) {
        const float a = fdot(d, d);
        const float ra = frcp(a);
        const float rl = frsq(a);
        float best = FLT_MAX, bpt = 0.0f;
        int slot = -1;
        // tile bins: the primary segment, and the first bounce when the whole wave
        // reflected off one wall (both wave-uniform)
        uint64_t km = ~0ull;
        if (!CULL && k == 0 && p.nbox > 0) km = keep;
        if (!CULL && k >= 1 && k <= p.mir_depth) km = mirror_keep<MAXD>(p, alive, st_m, k, tile);
        const bool binned = km != ~0ull;
        if (!CULL && binned) {
            // kept spheres in index order, kept walls
            if (alive) {
                uint64_t sm = p.nS >= 64 ? km : km & ((1ull << p.nS) - 1);
                while (sm) {
                    const int s = __builtin_ctzll(sm);
                    sm &= sm - 1;
                    const SphG32& G = p.s32[s >> 2];
                    const float Sf[4] = {G.c[0][s & 3], G.c[1][s & 3], G.c[2][s & 3], G.c[3][s & 3]};
                    sphere_f(Sf, s, o, d, a, ra, rl, best, bpt, slot);
                }
                walls_f(p, o, d, best, slot, p.nS >= 64 ? 0 : km >> p.nS);
            }
        } else if (CULL) {
            const Cone cn = (RT_EYE_CONE && k == 0) ? wave_cone_eye(o, d, alive)
                                                    : wave_cone(o, d, alive);
            if (RT_WALLS_FIRST) {
                uint64_t wm = k == 0 ? wkeep : ~0ull;
                if (RT_CULL_WALL_CONE && k > 0 && cn.on && p.nW > 0 && p.nW <= 64)
                    wm = wall_cone_mask(p, cn);
                if (alive) walls_f<RT_WALL_SLOAD>(p, o, d, best, slot, wm);
            }
            // wide cone: each lane its own sphere clusters (clusters_scan)
            const bool clusters = RT_CLUSTERS_F32 && p.nclu > 0 && cn.cos_t < p.clu_cos;
            if (clusters) clusters_scan_f(p, o, d, a, ra, rl, alive, best, bpt, slot);
            for (int c0 = 0; !clusters && c0 < p.nS; c0 += 64) {
                float lb;
                SphRec rec;
                uint64_t m = cull_chunk<false>(p, cn, c0, &lb, rec);
                // (a distance skip costs more than it saves at fp32 test prices: A/B)
                if (alive) {
                    while (m) {
                        const int l = __builtin_ctzll(m);
                        m &= m - 1;
                        const int sidx = c0 + l;
                        // the survivor's record by index, not out of the testing lane's
                        // registers (nor through rec64_sload: a wait per survivor, c5 +31%)
                        const SphG32& G = p.s32[sidx >> 2];
                        const float Sf[4] = {G.c[0][sidx & 3], G.c[1][sidx & 3], G.c[2][sidx & 3],
                                             G.c[3][sidx & 3]};
                        sphere_f<false>(Sf, sidx, o, d, a, ra, rl, best, bpt, slot, &p);
                    }
                }
            }
            if (!RT_WALLS_FIRST && alive) walls_f(p, o, d, best, slot);
        } else if (alive) {
            const int ng = (p.nS + 3) >> 2;
            for (int g = 0; g < ng; ++g) {
                const SphG32 G = p.s32[g];  // one s_load_dwordx16
#pragma unroll
                for (int h2 = 0; h2 < 2; ++h2) {
                    const int s0 = 4 * g + 2 * h2;
                    if (s0 >= p.nS) break;
                    sphere_pair_f(G, 2 * h2, s0, p.nS, o, d, a, ra, rl, best, bpt, slot);
                }
            }
        }
        if (!alive) return;
        ++segs;
        if (!CULL && !binned) walls_f(p, o, d, best, slot);
        const f3 nv = d * rl;
        if (slot < 0) {
            if (d.z < 0.0f) {
                c = F3(0.025f, 0.05f, 0.075f);
            } else {
                const float tz = fsqrt(fsqrt(nv.z));
                c = F3(fmaf(tz, 0.14f - 0.36f, 0.36f), fmaf(tz, 0.21f - 0.45f, 0.45f),
                       fmaf(tz, 0.49f - 0.57f, 0.57f));
            }
            alive = false;
            return;
        }
        const f3 pos = fmad3(d, best, o);
        f3 N;
        if (slot < p.nS) {
            const SphG32& G = p.s32[slot >> 2];
            N = fmad3(d, bpt, o) - F3(G.c[0][slot & 3], G.c[1][slot & 3], G.c[2][slot & 3]);
        } else {
            const Wall32& Wl = p.w32[slot - p.nS];
            N = F3(Wl.n[0], Wl.n[1], Wl.n[2]);
        }
        const DevMat32& m = p.mat32[slot];
        const f3 nn = fnormalize(N);
        const float2 sh = shade_f(m, pos, nn, nv, sun);
        if (k >= p.depth || k >= MAXD) {
            c = local_color_f(m, sh.x, sh.y, sun);
            alive = false;
            return;
        }
        st_s[k] = sh.x;
        st_k[k] = sh.y;
        st_m[k] = slot;
        n = k + 1;
        const float cc = 2.0f * fdot(nv, nn);
        o = fmad3(N, 1e-4f, pos);
        d = fmad3(nn, -cc, nv);
        };
    int kend = 0;  // wave-uniform: bounce iterations run (every lane's n <= kend)
    // the primary segment and the first bounce peeled (see trace_pixel_d); the F32 cull
    // kernels peel the primary only (the second copy: c3 +6%, c5 +9%)
    if (RT_PEEL >= 2 && !CULL) {
        if (__any(alive)) {
            segment(0);
            if (!__any(alive)) {
                kend = 1;
            } else {
                segment(1);
                for (int k = 2;; ++k) {
                    if (!__any(alive)) {
                        kend = k;
                        break;
                    }
                    segment(k);
                }
            }
        }
    } else if (RT_PEEL) {
        if (__any(alive)) {
            segment(0);
            for (int k = 1;; ++k) {
                if (!__any(alive)) {
                    kend = k;
                    break;
                }
                segment(k);
            }
        }
    } else {
        for (int k = 0;; ++k) {
            if (!__any(alive)) {
                kend = k;
                break;
            }
            segment(k);
        }
    }
    for (int q = MAXD - 1; q >= 0; --q) {
        if ((!RT_UNWIND_KEND || q < kend) && q < n) {  // uniform test: levels no lane reached
            const DevMat32& m = p.mat32[st_m[q]];
            const f3 L = local_color_f(m, st_s[q], st_k[q], sun);
            const float km = m.km;
            c = F3(fmaf(km, c.x - L.x, L.x), fmaf(km, c.y - L.y, L.y), fmaf(km, c.z - L.z, L.z));
        }
    }
    return c;
}

/* The store's pixel coordinates are formed again after the trace from the wave-uniform
 * tile (SGPRs) and the lane id read with v_mbcnt (not threadIdx.x, so the compiler cannot
 * merge it with the first computation): otherwise x, r and the valid flag stay live across
 * the whole bounce loop, and in the deep cull kernels (c5) they were what the register
 * allocator spilled to scratch — one store and one reload per lane, 12 B each. */
#ifndef RT_STORE_RECOMPUTE
#define RT_STORE_RECOMPUTE 1
#endif
__device__ __forceinline__ int lane_mbcnt() {
    return (int)__builtin_amdgcn_mbcnt_hi(~0u, __builtin_amdgcn_mbcnt_lo(~0u, 0u));
}

/* Rows of a band's tile row trow, sub-row sr (0..TILE_H-1): the frame row i it traces and
 * whether it exists, and the output row it is stored at.  A contiguous band (tstride <= 1)
 * is rows [row0, row0 + nrows), stored band-relative.  An interleaved part (KParams::tstride
 * = nparts > 1, rt_render_device_interleaved) owns the frame's tile rows tphase, tphase +
 * tstride, ...; it stores them back to back (band-relative) or, with out_frame, at their
 * frame rows. */
struct BandRow {
    int i, out;
    bool ok;
};
__device__ __forceinline__ BandRow band_row(const KParams& p, int trow, int sr) {
    const int rloc = trow * TILE_H + sr;
    BandRow b;
    if (p.tstride > 1) {
        b.i = (p.tphase + trow * p.tstride) * TILE_H + sr;
        b.ok = b.i < p.frame_h;
        b.out = p.out_frame ? b.i : rloc;
    } else {
        b.i = p.row0 + rloc;
        b.ok = rloc < p.nrows;
        b.out = rloc;
    }
    return b;
}

/* RT_OPT_SUPERSAMPLE's resolve (KParams::ss_log2 = k, S = 2^k): the wave's 8x8 square holds
 * the S x S samples of (8/S)^2 output pixels, sample (a, b) of a pixel at lane bits 0..k-1 (a)
 * and 3..3+k-1 (b).  An xor-butterfly over the column bits, then the row bits, is the
 * balanced pairwise tree of rt_capi.h (v[:, 0::2] + v[:, 1::2] repeated, then rows): fp64
 * addition is commutative, so every lane of a square ends with the same bits whichever half
 * of a pair it was, and a band that cuts a tile elsewhere than the full frame does stores the
 * same bytes.  Runs with all 64 lanes active (cross-lane reads of inactive lanes are
 * undefined): callers keep it outside any `if (valid)`.  1 / S^2 is a power of two, so the
 * final product is exact.
 * Lane xor 1, 2 and 8 are DPP moves (quad_perm, row_ror:8: no LDS round trip).  Xor 4 only
 * occurs at k = 3, after xor 1 and 2 made each quad uniform, where the half-row mirror
 * (lane i <-> 7 - i) reads the same value as lane i ^ 4 would.  Xor 16 and 32 go through
 * ds_bpermute.  The three channels take each step together, so a step costs one wait. */
template <int CTRL>
__device__ __forceinline__ double dpp_d(double v) {
    const unsigned long long b = (unsigned long long)__double_as_longlong(v);
    const unsigned lo = (unsigned)__builtin_amdgcn_update_dpp(0, (int)(unsigned)b, CTRL, 0xF, 0xF, false);
    const unsigned hi = (unsigned)__builtin_amdgcn_update_dpp(0, (int)(unsigned)(b >> 32), CTRL, 0xF, 0xF, false);
    return __longlong_as_double((long long)(((unsigned long long)hi << 32) | lo));
}
__device__ __forceinline__ void ss_resolve(int k, double& cr, double& cg, double& cb) {
    if (k >= 1) {  // columns: lane ^ 1
        cr += dpp_d<0xB1>(cr);
        cg += dpp_d<0xB1>(cg);
        cb += dpp_d<0xB1>(cb);
    }
    if (k >= 2) {  // lane ^ 2
        cr += dpp_d<0x4E>(cr);
        cg += dpp_d<0x4E>(cg);
        cb += dpp_d<0x4E>(cb);
    }
    if (k >= 3) {  // lane ^ 4 (quads uniform: the half-row mirror)
        cr += dpp_d<0x141>(cr);
        cg += dpp_d<0x141>(cg);
        cb += dpp_d<0x141>(cb);
    }
    if (k >= 1) {  // rows: lane ^ 8
        cr += dpp_d<0x128>(cr);
        cg += dpp_d<0x128>(cg);
        cb += dpp_d<0x128>(cb);
    }
    if (k >= 2) {  // lane ^ 16
        const double a = __shfl_xor(cr, 16, 64), b = __shfl_xor(cg, 16, 64), c = __shfl_xor(cb, 16, 64);
        cr += a;
        cg += b;
        cb += c;
    }
    if (k >= 3) {  // lane ^ 32
        const double a = __shfl_xor(cr, 32, 64), b = __shfl_xor(cg, 32, 64), c = __shfl_xor(cb, 32, 64);
        cr += a;
        cg += b;
        cb += c;
    }
    const double inv = __longlong_as_double((long long)(1023 - 2 * k) << 52);  // 1 / S^2
    cr *= inv;
    cg *= inv;
    cb *= inv;
}

/* One tile per wave: tile column bx, tile row trow (after the row order), gx tile columns.
 * SS: the tile is 8x8 samples of a supersampled frame, resolved before the store. */
template <int PREC, bool SUN, bool INT_EXP, bool CULL, int MAXD, bool SS = false>
__device__ __forceinline__ void trace_tile(const KParams& p, int bx, int trow, int gx,
                                           uint64_t braw) {
#if RT_WAVE_TIMES
    const uint64_t t_start = __builtin_amdgcn_s_memrealtime();
#endif
    const int lane = threadIdx.x & 63;
    const int wave = threadIdx.x >> 6;
    const int x = bx * TILE_W + (TILE_W > 8 ? (wave & 1) * 8 : 0) + (lane & 7);
    const BandRow br = band_row(p, trow, (TILE_H > 8 ? (wave >> 1) * 8 : 0) + (lane >> 3));
    const bool valid = x < p.W && br.ok;
    uint64_t t_tile = 0;  // the wave's start stamp (taken inside trace_pixel_*)
    const int i = br.i;
    int segs = 0;
    // every lane runs the (converged) bounce loop; only valid lanes trace and store
    // the store's coordinates (see RT_STORE_RECOMPUTE)
    auto store = [&](double cr, double cg, double cb) __attribute__((always_inline)) {
        if constexpr (SS) {
            // Invariant: the frame's width and the band's row count are multiples of S and a
            // wave's square starts at multiples of 8, so the S x S samples of an output pixel
            // are all valid or all invalid.  Invalid lanes hold garbage, which therefore only
            // ever mixes into squares that are not stored.
            const int k = p.ss_log2, sm = (1 << k) - 1;
            ss_resolve(k, cr, cg, cb);  // every lane, before any divergence
            // coordinates formed again from the tile, as the cull kernels' store below: here
            // in the linear kernels too, where it keeps them out of scratch (`make asm`)
            const bool recompute = RT_STORE_RECOMPUTE && BLOCK == 64;
            const int ls = recompute ? lane_mbcnt() : lane;
            const int xs = recompute ? bx * TILE_W + (ls & 7) : x;
            const BandRow bs = recompute ? band_row(p, trow, ls >> 3) : br;
            if (xs < p.W && bs.ok && (ls & sm) == 0 && ((ls >> 3) & sm) == 0)
                store_px(p, (size_t)(bs.out >> k) * (size_t)(p.W >> k) + (size_t)(xs >> k), cr, cg, cb);
        } else if (RT_STORE_RECOMPUTE && CULL && BLOCK == 64) {  // (linear kernels: no spill, A/B +1..12%)
            const int l2 = lane_mbcnt();
            const int xs = bx * TILE_W + (l2 & 7);
            const BandRow bs = band_row(p, trow, l2 >> 3);
            if (xs < p.W && bs.ok) store_pixel(p, bs.out, xs, cr, cg, cb);
        } else if (valid) {
            store_pixel(p, br.out, x, cr, cg, cb);
        }
    };
    if (PREC == PREC_F32) {
        const f3 c = trace_pixel_f<SUN, CULL, MAXD>(p, x, i, valid, segs, t_tile, braw);
        store(c.x, c.y, c.z);
    } else {
#if RT_STAGE_TIMES
        uint64_t g_stage[8];
        STAGE(0);
        const d3 c =
            trace_pixel_d<PREC == PREC_MIXED, PREC != PREC_PATH64, SUN, INT_EXP, CULL, MAXD>(
                p, x, i, valid, segs, t_tile, braw, g_stage);
#else
        const d3 c =
            trace_pixel_d<PREC == PREC_MIXED, PREC != PREC_PATH64, SUN, INT_EXP, CULL, MAXD>(
                p, x, i, valid, segs, t_tile, braw);
#endif
        store(c.x, c.y, c.z);
#if RT_STAGE_TIMES
        STAGE(5);
        {
            int sg = segs;
            for (int off = 32; off > 0; off >>= 1) sg += __shfl_xor(sg, off, 64);
            if (p.stats != nullptr && lane == 0 && bx < gx) {
                const size_t wid = ((size_t)trow * gx + bx) * (BLOCK / 64) + wave;
                for (int q = 0; q < 6; ++q) p.stats[8 * wid + q] = g_stage[q];
                p.stats[8 * wid + 6] = (unsigned long long)sg;
                p.stats[8 * wid + 7] = g_stage[6];
            }
        }
#endif
    }
    count_segments(p, segs);
    if (RT_STAMP && lane == 0 && bx < gx) {
        // this tile's cost for the host's next tile-row order (rt_capi.cpp row feedback)
        const uint64_t c = (__builtin_amdgcn_s_memtime() - t_tile) >> 5;
        p.tile_cost[((size_t)trow * gx + bx) * (BLOCK / 64) + wave] = (uint16_t)(c < 65535 ? c : 65535);
    }
#if RT_WAVE_TIMES
    // diagnostic build: per wave {start, end, segments << 32 | CU id} (100 MHz clock)
    for (int off = 32; off > 0; off >>= 1) segs += __shfl_xor(segs, off, 64);
    if (p.stats != nullptr && lane == 0 && bx < gx) {
        const size_t wid = ((size_t)trow * gx + bx) * (BLOCK / 64) + wave;
        p.stats[3 * wid] = t_start;
        p.stats[3 * wid + 1] = __builtin_amdgcn_s_memrealtime();
        p.stats[3 * wid + 2] = ((unsigned long long)segs << 32) | (unsigned)__smid();
    }
#endif
}


/* One workgroup of a frame's grid (x: tile column or part of one, y: dispatch unit). */
template <int PREC, bool SUN, bool INT_EXP, bool CULL, int MAXD, bool SS = false>
__device__ __forceinline__ void trace_grid(const KParams& p) {
    // workgroup row -> dispatch unit (a tile row, or a part of one: KParams::row_units_log2)
    // the primary pixel boxes (one per lane; wave-start load, used after ray generation)
    const uint64_t braw = (RT_EARLY_LOADS >= 2 && !CULL) ? box_load_primary(p) : 0;
    // dispatch units of the row order (tile rows or parts of them)
    const int n_units = (int)gridDim.y;
#if RT_EARLY_LOADS >= 2
    // every kernel-argument value the wave start needs — the dispatch order's entry and ray
    // generation's scalars (main.cpp:132) — loaded in one batch with one wait
    const int j = blockIdx.y;
    const uint32_t pw = row_perm_word(p, j);
    const int rc = p.row_center, rpn = p.row_perm_n;
    {
        const double a0 = p.pos[0], a1 = p.pos[1], a2 = p.pos[2], b0 = p.tl[0], b1 = p.tl[1],
                     b2 = p.tl[2], c0 = p.dx[0], c1 = p.dx[1], c2 = p.dx[2], e0 = p.dy[0],
                     e1 = p.dy[1], e2 = p.dy[2];
        asm volatile("" ::"s"(a0), "s"(a1), "s"(a2), "s"(b0), "s"(b1), "s"(b2), "s"(c0),
                     "s"(c1), "s"(c2), "s"(e0), "s"(e1), "s"(e2), "s"(p.W), "s"(p.row0),
                     "s"(p.nbox), "s"(pw), "s"(rc), "s"(rpn), "s"(p.row_units_log2),
                     "s"(gridDim.x), "s"(gridDim.y));
    }
    const int u = tile_row_of(rc, rpn, pw, j, n_units);
#else
    const int u = tile_row(p, blockIdx.y, n_units);
#endif
    const int ul = p.row_units_log2;
    const int gx = (p.W + TILE_W - 1) / TILE_W;
    const int bx = ((u & ((1 << ul) - 1)) * (int)gridDim.x) + (int)blockIdx.x;
    // the last part of a row may be short (wave-uniform): such a wave's lanes are all
    // invalid (x >= W), so it can also run through with nothing to trace or store
    if (!RT_EARLY_LOADS && bx >= gx) return;
    trace_tile<PREC, SUN, INT_EXP, CULL, MAXD, SS>(p, bx, u >> ul, gx, braw);
}

/* The frame kernel: one workgroup of BLOCK threads per dispatch unit and tile column. */
template <int PREC, bool SUN, bool INT_EXP, bool CULL, int MAXD, bool SS = false>
__global__ void __launch_bounds__(BLOCK)
__attribute__((amdgpu_waves_per_eu(
    shadow_waves<PREC, CULL, MAXD>(waves_per_eu<PREC, SUN, INT_EXP, CULL, MAXD>()), 8)))
k_trace(KParams p) {
    trace_grid<PREC, SUN, INT_EXP, CULL, MAXD, SS>(p);
}
