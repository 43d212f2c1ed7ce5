/* rt_rays_dev.h — closest hits and radiance for a batch of caller rays (rt_trace_rays*):
 * find_closest_hit (main.cpp:67-84) and recursive_ray_tracing (main.cpp:89-119) for any
 * ray, not only pixel (x, i) of a camera.  One lane per ray, one wave per 64 consecutive
 * rays; lanes past the end of the batch stay in the wave with alive == false (the ballots
 * and wave reductions of the scans need every lane present) and never load or store.
 *
 * The path is built from rt_scan_dev.h's device functions — make_ray, scan_d (linear scan,
 * or the wave cone / per-lane cluster walk of the cull kernels), shade_d / shade_f,
 * local_color_*, sky_d, the reflection step — and the recursion stack of trace_pixel_d with its
 * reverse lerp unwind.  What a frame adds on top of that (rt_frame_dev.h: eye tables, tile
 * bins, mirror bins, the row order) has no meaning for caller rays and is not included: every
 * segment, the first included, is scanned like a frame's unbinned bounce segment.
 *
 * Not a header of its own: included inside the namespace of a ray unit (rt_rays.hip, rt::kry;
 * rt_rays_shadow.hip, rt::krs, with the light ray of RT_FLAG_SHADOWS; rt_rays_lights.hip,
 * rt::krl, with the scene lights of rt_set_lights; rt_rays_glass.hip, rt::krg, with the
 * passage step of rt_set_transmission) behind rt_scan_dev.h. */
#ifndef RT_RAY_STACK_LDS
#define RT_RAY_STACK_LDS 1
#endif

/* The hit record as find_closest_hit returns it (Collision, scene.h): the compared distance,
 * the un-normalised normal — intersection_point - center for a sphere (scene.cpp:75-77), the
 * stored normal for a wall (scene.cpp:30) — and the scene index; a miss is main.cpp:70's
 * placeholder {DBL_MAX, (0,0,0), -1}.  Five 8-byte vector stores per lane. */
__device__ __forceinline__ void store_hit(const KParams& p, DevHit* hits, size_t ray,
                                          const RayD& r, const HitD& h) {
    double dist = DBL_MAX;
    d3 N = D3(0.0, 0.0, 0.0);
    int idx = -1;
    if (h.slot >= 0) {
        dist = h.dist;
        idx = scene_index(p, h.slot);
        if (h.slot < p.nS) {
            const double* S = p.s64[h.slot >> 2].v[h.slot & 3];
            N = (r.o + r.d * h.pt) - D3(S[0], S[1], S[2]);
        } else {
            N = ld3(p.w64[h.slot - p.nS].n);
        }
    }
    DevHit* o = hits + ray;
    o->distance = dist;
    o->normal[0] = N.x;
    o->normal[1] = N.y;
    o->normal[2] = N.z;
    *reinterpret_cast<unsigned long long*>(&o->index) = (unsigned long long)(unsigned)idx;
}

/* Lane's ray out of the batch.  Dead lanes get a harmless ray (they take part in the wave's
 * reductions only through their alive flag). */
__device__ __forceinline__ void load_ray(const RayArgs& ra, size_t ray, bool alive, d3& o, d3& d) {
    o = D3(0.0, 0.0, 0.0);
    d = D3(0.0, 0.0, 1.0);
    if (alive) {
        o = ld3(ra.org + ray * 3);
        d = ld3(ra.dir + ray * 3);
    }
}

/* One caller ray on the exact fp64 path: trace_pixel_d's bounce loop without the frame-only
 * shortcuts.  COLOR64: colour arithmetic in fp64 (F64); otherwise in fp32 (PATH64), the last
 * segment of a path included (RT_TERMINAL_F32), as in the frame kernels. */
template <bool COLOR64, bool SUN, bool INT_EXP, bool CULL, int MAXD>
__device__ __forceinline__ d3 trace_ray_d(const KParams& p, const RayArgs& ra, size_t ray, d3 o,
                                          d3 d, bool alive, int& segs) {
    using CT = typename std::conditional<COLOR64, double, float>::type;
    constexpr bool sun = SUN;
    RayD r = make_ray(o, d);
    // the recursion stack (trace_pixel_d's) in LDS, in the linear-scan kernels too
    // (RT_RAY_STACK_LDS): as registers they spilled where their frame counterparts do not
    constexpr bool LSTK = RT_RAY_STACK_LDS || RT_STACK_LDS >= 2 || (RT_STACK_LDS && CULL);
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
    // coloured lights: acc[c] + ka per channel and level, in LDS (trace_pixel_d's lds_l)
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
    // One segment at bounce k (wave-uniform); converged, as in trace_pixel_d.
    auto segment = [&](const int k) __attribute__((always_inline)) {
        const HitD h = scan_d<false, CULL, true>(p, r, alive, false, false, ~0ull);
        const bool last = k >= p.depth || k >= MAXD;  // remaining_iterations <= 0 (main.cpp:105)
#if RT_SHADOW
        // the light ray of every lane that hit (trace_pixel_d's step): converged, not counted
        const bool dark = light_blocked<CULL>(p, r, h, alive);
#endif
#if RT_LIGHTS
        // one light ray per light with RT_FLAG_SHADOWS (trace_pixel_d's step): bit l = hidden
        const unsigned dark = lights_blocked<CULL>(p, r, h, alive);
#endif
        if (!alive) return;
        ++segs;
        if (k == 0 && ra.hits != nullptr) store_hit(p, ra.hits, ray, r, h);
        if (!COLOR64 && RT_TERMINAL_F32 && (last || h.slot < 0)) {
            // PATH64, last segment of the path: nothing here feeds another ray
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
        // normalize(N): a wall's is a scene constant (host, same IEEE operations)
        const d3 nn = h.slot < p.nS ? normalize_e(N) : ld3(p.wnn[h.slot - p.nS]);
#if RT_LIGHTS
        CT vx, vy, vz;  // acc[c] + ka per channel (trace_pixel_d)
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
        if (dark) s = COLOR64 ? (CT)m.ka : (CT)p.mat32[h.slot].ka;  // diffuse = specular = 0
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
            r = make_ray(nr.o, nr.d);
            return;
        }
#endif
        // start + reflect(d, N) (main.cpp:111-113, vec.cpp:51-57)
        const double cc = 2 * dot(nv, nn);
        r = make_ray(pos + N * .0001, nv - nn * cc);
    };
    int kend = 0;  // wave-uniform: segments run (every lane's n <= kend)
    if (__any(alive)) {
        segment(0);  // peeled: k == 0 folded (the hit record's store)
        for (int k = 1;; ++k) {
            if (!__any(alive)) {
                kend = k;
                break;
            }
            segment(k);
        }
    }
    for (int q = MAXD - 1; q >= 0; --q) {
        if (q < kend && q < n) {  // kend: uniform test for the levels no lane reached
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
    if (COLOR64) return c64;
    return D3(c32.x, c32.y, c32.z);
}

/* Occupancy targets: the frame kernels' (waves_per_eu), which the ray kernels meet with the
 * same registers — except the PATH64 no-sun linear-scan kernels, RT_RAY_WPE_P64_LIN (A/B). */
#ifndef RT_RAY_WPE_P64_LIN
#define RT_RAY_WPE_P64_LIN 4
#endif
template <int PREC, bool SUN, bool INT_EXP, bool CULL, int MAXD>
constexpr int ray_waves_per_eu() {
    if (PREC == PREC_PATH64 && !SUN && !CULL && MAXD < 16) return RT_RAY_WPE_P64_LIN;
    return waves_per_eu<PREC, SUN, INT_EXP, CULL, MAXD>();
}

/* Radiance (and, with RayArgs::hits, the first segment's hit record) of ray blockIdx.x *
 * BLOCK + threadIdx.x; the colour goes to pixel `ray` of KParams::out in KParams::outf. */
template <int PREC, bool SUN, bool INT_EXP, bool CULL, int MAXD>
__global__ void __launch_bounds__(BLOCK)
__attribute__((amdgpu_waves_per_eu(
    shadow_waves<PREC, CULL, MAXD>(ray_waves_per_eu<PREC, SUN, INT_EXP, CULL, MAXD>()), 8)))
k_rays(KParams p, RayArgs ra) {
    const size_t ray = (size_t)blockIdx.x * BLOCK + threadIdx.x;
    const bool alive = ray < (size_t)ra.n;
    d3 o, d;
    load_ray(ra, ray, alive, o, d);
    int segs = 0;
    const d3 c = trace_ray_d<PREC != PREC_PATH64, SUN, INT_EXP, CULL, MAXD>(p, ra, ray, o, d,
                                                                             alive, segs);
    if (alive) store_px(p, ray, c.x, c.y, c.z);
    count_segments(p, segs);
}

template <class K>
static hipError_t launch_k(K kern, const KParams& p, const RayArgs& ra, hipStream_t st,
                           hipEvent_t done) {
    const dim3 grid((unsigned)(((size_t)ra.n + BLOCK - 1) / BLOCK));
    if (done)
        hipExtLaunchKernelGGL(kern, grid, dim3(BLOCK), 0, st, nullptr, done, 0, p, ra);
    else
        hipLaunchKernelGGL(kern, grid, dim3(BLOCK), 0, st, p, ra);
    return hipGetLastError();
}
/* The depth buckets of the frame kernels (launch_depth). */
template <int PREC, bool SUN, bool INT_EXP, bool CULL>
static hipError_t rays_depth(const KParams& p, const RayArgs& ra, hipStream_t st, hipEvent_t done) {
    if constexpr (!INT_EXP) {
        // a scene with a non-integer specular exponent (general pow()): one instantiation
        return launch_k(k_rays<PREC, SUN, false, CULL, MAXD_LARGE>, p, ra, st, done);
    } else {
        if (p.depth <= MAXD_SMALL) return launch_k(k_rays<PREC, SUN, true, CULL, MAXD_SMALL>, p, ra, st, done);
        if (p.depth <= MAXD_MID) return launch_k(k_rays<PREC, SUN, true, CULL, MAXD_MID>, p, ra, st, done);
        if (p.depth <= MAXD_REF) return launch_k(k_rays<PREC, SUN, true, CULL, MAXD_REF>, p, ra, st, done);
        return launch_k(k_rays<PREC, SUN, true, CULL, MAXD_LARGE>, p, ra, st, done);
    }
}
template <int PREC, bool SUN, bool INT_EXP>
static hipError_t rays_cull(const KParams& p, const RayArgs& ra, hipStream_t st, hipEvent_t done) {
    return p.wave_cull ? rays_depth<PREC, SUN, INT_EXP, true>(p, ra, st, done)
                       : rays_depth<PREC, SUN, INT_EXP, false>(p, ra, st, done);
}
