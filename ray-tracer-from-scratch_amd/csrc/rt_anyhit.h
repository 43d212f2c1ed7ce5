/* rt_anyhit.h — any-hit scans on the segment o .. o + d * T, for the occlusion query
 * (rt_rays.hip k_ray_occluded) and the light ray of RT_FLAG_SHADOWS (rt_scan_dev.h
 * light_blocked).  Not a header of its own: it is included inside the namespace of a unit
 * that has rt_scan_dev.h's device functions in front of it (RayD, div_r, wave_cone,
 * cull_chunk, clusters_mask, ...), once per unit.
 *
 * A lane is blocked as soon as one primitive j has a Collision c = scene[j]->intersect(ray)
 * with c.distance > 0 (find_closest_hit's acceptance, main.cpp:77) whose PARAMETER along the
 * ray is <= T: a wall's c.distance is that parameter (scene.cpp:10), a sphere's is
 * `projection`, the value scene.cpp:77 multiplies by |d|.  Both are the exact fp64 values of
 * the closest-hit path and the decision is the fp64 <= on them; no best hit is kept, so there
 * is no HitD, no visiting order and no tie rule.  `todo` = the lane is live, its T admits a
 * blocker (T > 0: a NaN or non-positive limit is free at once) and nothing has blocked it yet;
 * the scans stop as soon as no lane of the wave has anything left to decide. */

/* Sphere::intersect up to `projection`: sphere_exact_oc's arithmetic and exact rejections. */
__device__ __forceinline__ bool sphere_blocks(const double* S, const RayD& r, double T) {
    const d3 oc = r.o - D3(S[0], S[1], S[2]);
    const double c = lensq(oc) - S[3];
    const double dt = dot(r.d, oc);      // b / 2
    const double x = dt * dt - r.a * c;  // det / 4
    if (dt > 0 || !(x >= 0)) return false;
    double proj;
    if (x == 0) {
        proj = 2.0 * div_r(-dt, r.a, r.ra);  // scene.cpp:65's /a kept
    } else {
        const double num = -dt - sqrt_e(x);
        if (!(num > 0)) return false;
        proj = div_r(num, r.a, r.ra);
    }
    return proj * r.dlen > 0 && proj <= T;  // c.distance > 0, then the parameter against T
}

/* Wall::intersect: wall_exact's t and bounds. */
__device__ __forceinline__ bool wall_blocks(const Wall64& Wl, const RayD& r, double T) {
    const d3 n = ld3(Wl.n);
    const d3 P = ld3(Wl.P);
    const double den = dot(n, r.d);
    const double num = dot(P - r.o, n);
    double t;
    if (RT_WALL_NOSIGN) {
        t = div_r_nz(num, den, rcp_refined(den));  // see wall_exact: 0, NaN, inf fail t > 0
    } else {
        if (!((num > 0 && den > 0) || (num < 0 && den < 0))) return false;
        t = div_r(num, den, rcp_refined(den));
    }
    if (!(t > 0) || !(t <= T)) return false;
    const d3 q = (r.o + r.d * t) - P;
    const double px = dot(q, ld3(Wl.X));
    const double py = dot(q, ld3(Wl.Y));
    return px >= 0 && px <= Wl.len && py >= 0 && py <= Wl.wid;
}

/* Linear scenes: walls, then groups of 4 spheres per scalar load behind closest_hit_d's
 * conservative fp32 cull (sphere_cull: it drops a sphere only where the exact test rejects). */
__device__ __forceinline__ void occluded_linear(const KParams& p, const RayD& r, bool& todo,
                                                double T) {
    for (int w = 0; w < p.nW; ++w) {
        if (!__any(todo)) return;
        if (todo) todo = !wall_blocks(p.w64[w], r, T);
    }
    const bool PRE = RT_SPH_PRECULL && p.nS >= 4;  // wave-uniform, as closest_hit_d
    RayF rf;
    if (PRE) rf = make_rayf(r);
    const int ng = (p.nS + 3) >> 2;
    for (int g = 0; g < ng; ++g) {
        if (!__any(todo)) return;
        if (!todo) continue;
        if (PRE) {
            const SphG32 G = p.s32[g];
            bool cu[4];
            sphere_cull_pair(G, 0, rf, cu[0], cu[1]);
            sphere_cull_pair(G, 2, rf, cu[2], cu[3]);
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                const int s = 4 * g + k;
                if (s < p.nS && !cu[k] && todo) todo = !sphere_blocks(p.s64[g].v[k], r, T);
            }
        } else {
            const SphG64 G = p.s64[g];
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                const int s = 4 * g + k;
                if (s < p.nS && todo) todo = !sphere_blocks(G.v[k], r, T);
            }
        }
    }
}

/* Margin of the limit tests against the fp32 lower bounds (a cone survivor's distance bound,
 * a cluster box's entry parameter): a sphere is skipped only where the bound, shrunk by 1e-3,
 * still exceeds the lane's limit — far above the bounds' own fp32 error. */
constexpr double OCC_LB_MARGIN = 1.0 - 1e-3;

/* clusters_scan's walk for the undecided lanes: a cluster whose box entry lies beyond the
 * lane's limit holds no blocker (its spheres' parameters are >= the entry). */
__device__ __forceinline__ void occluded_clusters(const KParams& p, const RayD& r, bool& todo,
                                                  double T) {
    const f3 o = F3((float)r.o.x, (float)r.o.y, (float)r.o.z);
    const f3 d = F3((float)r.d.x, (float)r.d.y, (float)r.d.z);
    const SlabRay sr = slab_ray(o, d);
    const bool near = fmax3abs(o.x, o.y, o.z) <= p.clu_oinf;
    const int oct = clu_octant(d);
    uint64_t cm = 0;
    if (RT_CLU_FAST) {
        cm = p.nclu <= 32 ? clusters_mask<RT_CLU_OCT, false>(p, sr, todo, near, oct)
                          : clusters_mask<RT_CLU_OCT, true>(p, sr, todo, near, oct);
    } else {
        for (int c = 0; c < p.nclu; ++c) {
            const bool in = !near || slab_t(p.clu[c], sr) < __builtin_inff();
            cm |= (uint64_t)(todo && in) << clu_bit<RT_CLU_OCT>(p.clu[c], oct, c);
        }
    }
    while (__any(todo && cm != 0)) {
        if (todo && cm != 0) {
            const int k = __builtin_ctzll(cm);
            cm &= cm - 1;
            const int c = RT_CLU_OCT ? (int)p.cord[oct * CLU_MAX + k] : k;
            const float t = near ? slab_t(p.clu[c], sr) : 0.0f;
            if ((double)t * OCC_LB_MARGIN <= T) {
                const CluSph* cs = p.csph + c * p.clu_ls;
#pragma unroll
                for (int q = 0; q < CLU_SIZE; ++q) {
                    if (q == CLU_SIZE_D && p.clu_ls == CLU_SIZE_D) break;
                    if (cs[q].slot >= 0 && todo) todo = !sphere_blocks(cs[q].c, r, T);
                }
            }
        }
    }
}

/* Wave-cull scenes: scan_d's choice — the undecided rays' cone over 64 spheres at a time, or
 * each lane's own cluster walk when the cone is wide — with the limit as a further cull. */
__device__ __forceinline__ void occluded_cull(const KParams& p, const RayD& r, bool& todo,
                                              double T) {
    if (!__any(todo)) return;  // (the cone's reductions need a live ray)
    const f3 co = F3((float)r.o.x, (float)r.o.y, (float)r.o.z);
    const f3 cd = F3((float)r.d.x, (float)r.d.y, (float)r.d.z);
    const Cone cn = wave_cone(co, cd, todo);
    uint64_t wm = ~0ull;  // walls to test (bit w = wall w; walls past 63: all)
    if (RT_CULL_WALL_CONE && cn.on && p.nW > 0 && p.nW <= 64) wm = wall_cone_mask(p, cn);
    for (int w = 0; w < p.nW; ++w) {
        if (wm != ~0ull && !((wm >> w) & 1)) continue;
        if (!__any(todo)) return;
        // (the record through scalar loads, as the cull kernels' walls_d_kept: the compiler's
        // own loads take the vector memory path here)
        const Wall64 Wl = RT_WALL_SLOAD ? wall64_sload(p.w64 + w) : p.w64[w];
        if (todo) todo = !wall_blocks(Wl, r, T);
    }
    if (RT_CLUSTERS && p.nclu > 0 && cn.cos_t < p.clu_cos) {
        occluded_clusters(p, r, todo, T);
        return;
    }
    const double Tw = T * r.dlen;  // the limit as a world distance, for cull_chunk's bound
    for (int c0 = 0; c0 < p.nS; c0 += 64) {
        if (!__any(todo)) return;
        float lb;
        SphRec rec;
        uint64_t m = cull_chunk<true>(p, cn, c0, &lb, rec);
        while (m) {
            const int l = __builtin_ctzll(m);
            m &= m - 1;
            const double bound = (double)lane_f(lb, l);
            if (!__any(todo)) return;
            if (todo && bound * OCC_LB_MARGIN <= Tw) {
                const int sidx = c0 + l;
                todo = !sphere_blocks(p.s64[sidx >> 2].v[sidx & 3], r, T);
            }
        }
    }
}
