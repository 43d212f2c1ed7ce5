/*
 * rt_scan_dev.h — the device code every kernel unit shares, for gfx950 (CDNA4): vec3
 * (vec.cpp:3-57), Sphere::intersect (scene.cpp:40-78), Wall::intersect (scene.cpp:4-35),
 * find_closest_hit (main.cpp:67-84) as a linear, wave-culled or clustered scan (scan_d), the
 * light ray of RT_FLAG_SHADOWS, the shading helpers out_color / diffuse_shading / specular
 * (main.cpp:28-62), the pixel store and the occupancy targets.  With rt_frame_dev.h on top
 * (primary ray generation, main.cpp:132-134; recursive_ray_tracing, main.cpp:89-119, one
 * thread per pixel) it replaces the reference's rt_scene loop (main.cpp:124-139) and
 * everything under it; rt_rays_dev.h builds the same path for caller rays.
 * Not a header of its own: included inside `namespace rt { namespace <unit> {`, which the
 * including unit opens behind rt_knobs.h.  It depends on RT_STAMP, RT_SHADOW and RT_LIGHTS only.
 *
 * Precisions (template PREC):
 *   PREC_F64   the reference's fp64 arithmetic.  The units are built with
 *              -ffp-contract=off, so nothing is fused that the reference (x86-64, no
 *              FMA) does not fuse; where operations are restructured for speed the
 *              result is provably bit-identical (see "exact rewrites" below).  The only
 *              non-bit-exact operations are pow (x^e by squaring for integer e, sky
 *              z^0.25 as sqrt(sqrt(z))): <= a few ulp, vs glibc's correctly rounded pow.
 *   PREC_F32   fp32 with fused multiply-adds and hardware rcp/rsq/sqrt/exp/log: the
 *              throughput path; flips at geometric discontinuities.
 *   PREC_MIXED fp32 conservative cull in the primitive scan, PREC_F64's exact test on
 *              every primitive the cull cannot reject, fp64 shading: output == F64.
 *   PREC_PATH64 PREC_F64's exact ray path (hits, positions, normals, reflections) with
 *              the colour arithmetic (shading, sky, lerp) in fp32: every pixel follows the
 *              reference's path, colours within ~1e-6 (no discontinuity flips).
 *
 * Exact rewrites (each identity holds in IEEE binary64 barring overflow/underflow):
 *   - b = 2*dot(d,oc) is exact, so b*b - (4a)*c == 4*(dot*dot - a*c) and
 *     (-b - sqrt(det)) / (2a) == (-dot - sqrt(det/4)) / a (power-of-two scalings
 *     commute with rounding; sqrt(4x) == 2*sqrt(x)).
 *   - x / y for several x and one y: LLVM's fp64 division is rcp + two Newton steps +
 *     one fma correction wrapped in div_scale/div_fixup, which are identities for
 *     normal-range operands; sharing the refined reciprocal across numerators gives
 *     the same bits (checked on device by rt_selftest, tests/test_gpu_parity.py).
 *   - normalize(-d) == -normalize(d) (negation commutes with rounding).
 *
 * Recursion -> iteration with identical rounding: the reference returns
 * lerp(local, traced, metallic) from the innermost bounce outward (vec.cpp:45-49).
 * Each bounce pushes (shading scalar s, sun scalar, material slot) onto a per-thread
 * register stack indexed by the wave-uniform bounce counter; the stack is unwound in
 * reverse with the same operations, so local = color*s is recomputed bit-identically.
 */
#if RT_DIAG
__device__ unsigned long long g_diag[16];  // DIAG's counters, one set per unit
#endif

/* ------------------------------------------------------------------------ */
/* fp64 vector math, vec.cpp:3-57 (this TU: -ffp-contract=off)               */
/* ------------------------------------------------------------------------ */
struct d3 {
    double x, y, z;
};
__device__ __forceinline__ d3 D3(double x, double y, double z) { return d3{x, y, z}; }
__device__ __forceinline__ d3 operator+(d3 a, d3 b) { return D3(a.x + b.x, a.y + b.y, a.z + b.z); }
__device__ __forceinline__ d3 operator-(d3 a, d3 b) { return D3(a.x - b.x, a.y - b.y, a.z - b.z); }
__device__ __forceinline__ d3 operator-(d3 a) { return D3(-a.x, -a.y, -a.z); }
__device__ __forceinline__ d3 operator*(d3 a, d3 b) { return D3(a.x * b.x, a.y * b.y, a.z * b.z); }
__device__ __forceinline__ d3 operator*(d3 a, double s) { return D3(a.x * s, a.y * s, a.z * s); }
__device__ __forceinline__ double dot(d3 a, d3 b) { return a.x * b.x + a.y * b.y + a.z * b.z; }
__device__ __forceinline__ double lensq(d3 a) { return a.x * a.x + a.y * a.y + a.z * a.z; }
__device__ __forceinline__ d3 lerp(d3 a, d3 b, double t) {
    return D3(a.x + t * (b.x - a.x), a.y + t * (b.y - a.y), a.z + t * (b.z - a.z));
}
__device__ __forceinline__ d3 ld3(const double* p) { return D3(p[0], p[1], p[2]); }

/* Reciprocal refined exactly as LLVM's fp64 division refines it (rcp + 2 Newton). */
__device__ __forceinline__ double rcp_refined(double b) {
    double r = __builtin_amdgcn_rcp(b);
    double e = __builtin_fma(-b, r, 1.0);
    r = __builtin_fma(r, e, r);
    e = __builtin_fma(-b, r, 1.0);
    return __builtin_fma(r, e, r);
}
/* a / b correctly rounded, given r = rcp_refined(b) (a == 0 keeps IEEE's signed zero). */
__device__ __forceinline__ double div_r(double a, double b, double r) {
    const double q = a * r;
    const double e = __builtin_fma(-b, q, a);
    const double q1 = __builtin_fma(e, r, q);
    return a == 0.0 ? q : q1;
}
/* a / b for a != 0 (or where the sign of a zero quotient cannot matter): div_r without
 * its a == 0 select. */
__device__ __forceinline__ double div_r_nz(double a, double b, double r) {
    const double q = a * r;
    const double e = __builtin_fma(-b, q, a);
    return __builtin_fma(e, r, q);
}
/* sqrt(x) correctly rounded: LLVM's fp64 sqrt sequence (rsq + Goldschmidt/Newton
 * refinement) without its range scaling, which is the identity for x >= 2^-767; smaller
 * (and zero/negative) arguments take the library path. */
__device__ __forceinline__ double sqrt_e(double x) {
    // tiny, zero, negative, NaN and +inf take the library path (+inf: rsq(inf) = 0 would
    // give inf * 0 = NaN below; the library passes inf through)
    if (!(x >= 0x1p-767 && x <= DBL_MAX)) return sqrt(x);
    const double y = __builtin_amdgcn_rsq(x);
    double g = x * y;
    double h = y * 0.5;
    const double r = __builtin_fma(-h, g, 0.5);
    g = __builtin_fma(g, r, g);
    double d = __builtin_fma(-g, g, x);
    h = __builtin_fma(h, r, h);
    g = __builtin_fma(d, h, g);
    d = __builtin_fma(-g, g, x);
    return __builtin_fma(d, h, g);
}
/* v / len(v) component-wise (vec.cpp:21), one shared reciprocal. */
__device__ __forceinline__ d3 normalize_e(d3 v) {
    const double l = sqrt_e(lensq(v));
    const double r = rcp_refined(l);
    return D3(div_r(v.x, l, r), div_r(v.y, l, r), div_r(v.z, l, r));
}
__device__ __forceinline__ d3 div3(d3 v, double l, double r) {
    return D3(div_r(v.x, l, r), div_r(v.y, l, r), div_r(v.z, l, r));
}
/* x^n for x >= 0 and integer n >= 0 by binary powering. */
__device__ __forceinline__ double pow_int(double x, int n) {
    double acc = 1.0, b = x;
    while (n) {
        if (n & 1) acc *= b;
        n >>= 1;
        if (n) b *= b;
    }
    return acc;
}
/* x^e for x >= 0.  INT_EXP (host-checked at rt_set_scene: every specular exponent is an
 * integer in [0, 1024], as in the reference scene and all configs: 30, 50) compiles only
 * the binary powering; otherwise the general pow() is kept — it is large, and its
 * register footprint counts for the whole kernel even where it never runs. */
template <bool INT_EXP>
__device__ __forceinline__ double pow_e(double x, double e) {
    if (INT_EXP) return pow_int(x, (int)e);
    if (e >= 0.0 && e <= 1024.0 && e == __builtin_rint(e)) return pow_int(x, (int)e);
    return pow(x, e);
}

typedef float f2 __attribute__((ext_vector_type(2)));

/* fp32 vector math (throughput path; FMAs explicit) */
struct f3 {
    float x, y, z;
};
__device__ __forceinline__ f3 F3(float x, float y, float z) { return f3{x, y, z}; }
__device__ __forceinline__ f3 operator+(f3 a, f3 b) { return F3(a.x + b.x, a.y + b.y, a.z + b.z); }
__device__ __forceinline__ f3 operator-(f3 a, f3 b) { return F3(a.x - b.x, a.y - b.y, a.z - b.z); }
__device__ __forceinline__ f3 operator-(f3 a) { return F3(-a.x, -a.y, -a.z); }
__device__ __forceinline__ f3 operator*(f3 a, float s) { return F3(a.x * s, a.y * s, a.z * s); }
__device__ __forceinline__ float fdot(f3 a, f3 b) { return fmaf(a.x, b.x, fmaf(a.y, b.y, a.z * b.z)); }
__device__ __forceinline__ float frsq(float x) { return __builtin_amdgcn_rsqf(x); }
__device__ __forceinline__ float frcp(float x) { return __builtin_amdgcn_rcpf(x); }
__device__ __forceinline__ float fsqrt(float x) { return __builtin_amdgcn_sqrtf(x); }
__device__ __forceinline__ f3 fnormalize(f3 a) { return a * frsq(fdot(a, a)); }
__device__ __forceinline__ f3 fmad3(f3 a, float s, f3 b) {  // a*s + b
    return F3(fmaf(a.x, s, b.x), fmaf(a.y, s, b.y), fmaf(a.z, s, b.z));
}
__device__ __forceinline__ float fmax3abs(float a, float b, float c) {
    return fmaxf(fmaxf(fabsf(a), fabsf(b)), fabsf(c));
}
/* x^e for x >= 0 via v_log_f32 / v_exp_f32 (pow(0,e>0) = 0, pow(x,0) = 1). */
__device__ __forceinline__ float fpow(float x, float e) {
    if (e == 0.0f) return 1.0f;
    return __builtin_amdgcn_exp2f(e * __builtin_amdgcn_logf(x));
}

/* main.cpp:14-19 */
__device__ __forceinline__ d3 ground_color() { return D3(0.025, 0.05, 0.075); }
__device__ __forceinline__ d3 sky_low() { return D3(0.36, 0.45, 0.57); }
__device__ __forceinline__ d3 sky_high() { return D3(0.14, 0.21, 0.49); }
__device__ __forceinline__ d3 sun_color() { return D3(1.64, 1.27, 0.99); }
__device__ __forceinline__ d3 sun_direction() { return D3(.7, .4, .7); }

/* Largest bounce count compiled: the register stack is sized per instantiation. */
constexpr int MAXD_SMALL = 4;
constexpr int MAXD_MID = 8;
constexpr int MAXD_REF = 10;  // rt_scene's default recursion depth (main.cpp:89)
constexpr int MAXD_LARGE = 16;

/* ------------------------------------------------------------------------ */
/* closest hit (find_closest_hit, main.cpp:67-84)                            */
/* ------------------------------------------------------------------------ */
/* Winner of the scan.  The reference's strict `0 < d < best` scan in scene order returns
 * the lowest scene index among the minimum distance; spheres are visited in scene order
 * (ties among them keep the earlier one) and a wall that ties the best compares scene
 * indices, so the winner is the same. */
struct HitD {
    double dist;  // the value find_closest_hit compares (sphere: world, wall: parametric)
    double pt;    // sphere: parameter of the intersection point used for the normal
    int slot;     // material slot: sphere s -> s, wall w -> nS + w; -1 = miss
};

struct RayD {
    d3 o, d;
    double a;     // |d|^2
    double ra;    // rcp_refined(a)
    double dlen;  // sqrt(a) == d.length()
};

/* Sphere::intersect (scene.cpp:40-78), exact, in the scaled form (file header).  Only
 * branches that can produce an accepted distance are evaluated; every skip is exact:
 *   dot > 0 (b > 0)    -> proj = (-b - sqrt(det)) / 2a < 0, rejected by d > 0
 *   x < 0 (det < 0)    -> miss (scene.cpp:57)
 *   -dot - sqrt(x) <= 0 -> proj <= 0, rejected
 * and p1 is never the minimum: (-b+sq)/2a >= (-b-sq)/2a by monotonic rounding. */
__device__ __forceinline__ int scene_index(const KParams& p, int slot) {
    return slot < p.nS ? p.sph_j[slot] : p.wall_j[slot - p.nS];
}

/* IN_ORDER: spheres visited in increasing index before any wall, so a tie keeps the
 * earlier hit (strict <, main.cpp:77); otherwise a tie compares scene indices. */
/* oc = origin - center and c = |oc|^2 - r^2 given (eye tables) or computed here. */
template <bool IN_ORDER = true>
__device__ __forceinline__ void sphere_exact_oc(const d3 oc, const double c, int s,
                                                const RayD& r, HitD& h,
                                                const KParams* p = nullptr) {
    const double dt = dot(r.d, oc);  // b / 2
    const double x = dt * dt - r.a * c;  // det / 4
    if (RT_SPHERE_ONEBRANCH) {
        if (dt > 0 || !(x >= 0)) return;  // one branch for both rejections
    } else {
        if (dt > 0) return;
        if (!(x >= 0)) return;
    }
    DIAG(2);
    double proj, pt;
    if (x == 0) {
        pt = div_r(-dt, r.a, r.ra);  // -b / (2a)
        proj = 2.0 * pt;             // (-b - sqrt(0)) / a: scene.cpp:65's /a kept
    } else {
        const double num = -dt - sqrt_e(x);
        if (!(num > 0)) return;
        proj = div_r(num, r.a, r.ra);
        pt = proj;
    }
    const double dist = proj * r.dlen;  // world distance, scene.cpp:77
    bool take = dist > 0 && dist < h.dist;
    if (!IN_ORDER && !take && dist > 0 && dist == h.dist && h.slot >= 0)
        take = scene_index(*p, s) < scene_index(*p, h.slot);
    if (take) {
        h.dist = dist;
        h.pt = pt;
        h.slot = s;
    }
}
template <bool IN_ORDER = true>
__device__ __forceinline__ void sphere_exact(const double* S, int s, const RayD& r, HitD& h,
                                             const KParams* p = nullptr) {
    const d3 oc = r.o - D3(S[0], S[1], S[2]);
    sphere_exact_oc<IN_ORDER>(oc, lensq(oc) - S[3], s, r, h, p);
}

/* Wall::intersect (scene.cpp:4-35), exact.  t = num/denom is formed only when the signs
 * make t > 0 possible (denom == 0 or NaN can never pass the bounds check). */
template <bool EYE = false>
__device__ __forceinline__ void wall_exact(const Wall64& Wl, int w, const KParams& p,
                                           const RayD& r, HitD& h) {
    const d3 n = ld3(Wl.n);
    const d3 P = ld3(Wl.P);
    const double den = dot(n, r.d);
    const double num = EYE ? p.eye_w[w] : dot(P - r.o, n);
    double t;
    if (RT_WALL_NOSIGN) {
        // t <= 0 (opposite signs or num == 0), NaN (0/0) and +-inf (den == 0: rcp_refined
        // gives NaN) all fail t > 0, as in the reference (scene.cpp:12); the zero-quotient
        // sign does not matter since 0 fails t > 0 either way
        t = div_r_nz(num, den, rcp_refined(den));
        if (!(t > 0) || (RT_WALL_TSKIP && t > h.dist)) return;  // t > best loses anyway
    } else {
        if (!((num > 0 && den > 0) || (num < 0 && den < 0))) return;
        DIAG(4);
        t = div_r(num, den, rcp_refined(den));
        if (!(t > 0)) return;
        if (RT_WALL_TSKIP && t > h.dist) return;  // loses to the current best either way
    }
    DIAG(6);
    const d3 q = (r.o + r.d * t) - P;  // ray::at (scene.h:16) minus the corner
    const double px = dot(q, ld3(Wl.X));
    const double py = dot(q, ld3(Wl.Y));
    if (px >= 0 && px <= Wl.len && py >= 0 && py <= Wl.wid) {
        bool take = t < h.dist;
        if (!take && t == h.dist && h.slot >= 0)  // tie: the lower scene index wins (rare)
            take = p.wall_j[w] < scene_index(p, h.slot);
        if (take) {
            h.dist = t;
            h.slot = p.nS + w;
        }
    }
}

/* MIXED: fp32 conservative cull in front of the exact sphere test.  A sphere is skipped
 * only when the fp32 evaluation proves, with a margin covering its rounding error, that
 * the exact test rejects it (det < 0, or b > 0).  Margins:
 *   |b/2 error| <= 18u*dinf*B,  |det/4 error| <= 133u*a*B^2 + ...,  B = |o|inf+|C|inf+r,
 * bounded here by K*dinf*B and 8K*a*B^2 with K = 512u. */
struct RayF {
    f3 o, d;
    float a;
    float kb;     // K * dinf
    float kdet;   // 8K * a
    float oinf;
};
constexpr float CULL_U = 1.0f / 16777216.0f;  // 2^-24
constexpr float CULL_K = 512.0f * CULL_U;

__device__ __forceinline__ bool sphere_cull(const float* S, const RayF& r) {
    const f3 oc = r.o - F3(S[0], S[1], S[2]);
    const float bh = fdot(r.d, oc);
    const float c = fmaf(-S[3], S[3], fdot(oc, oc));
    const float det = fmaf(bh, bh, -r.a * c);
    const float B = r.oinf + fmax3abs(S[0], S[1], S[2]) + S[3];
    return (bh > r.kb * B) || (det < -r.kdet * (B * B));
}

__device__ __forceinline__ bool wall_cull(const Wall32& Wl, const RayF& r) {
    const f3 n = F3(Wl.n[0], Wl.n[1], Wl.n[2]), P = F3(Wl.P[0], Wl.P[1], Wl.P[2]);
    const float den = fdot(n, r.d);
    const float num = fdot(P - r.o, n);
    const float B = r.oinf + fmax3abs(P.x, P.y, P.z);
    const float mnum = CULL_K * B;
    const float mden = r.kb;
    if ((num < -mnum && den > mden) || (num > mnum && den < -mden)) return true;  // t < 0
    if (fabsf(num) <= 64.0f * mnum || fabsf(den) <= 64.0f * mden) return false;   // ill-conditioned
    // t's relative error <= mnum/|num| + mden/|den| (<= 1/32 here); bound the point error.
    const float t = num * frcp(den);
    const float rel = mnum / fabsf(num) + mden / fabsf(den) + 4.0f * CULL_U;
    const f3 q = fmad3(r.d, t, r.o) - P;
    const float len_dt = fsqrt(r.a) * fabsf(t);
    const float err = 2.0f * len_dt * rel + CULL_K * (B + len_dt + Wl.len + Wl.wid);
    const float px = fdot(q, F3(Wl.X[0], Wl.X[1], Wl.X[2]));
    const float py = fdot(q, F3(Wl.Y[0], Wl.Y[1], Wl.Y[2]));
    return px < -err || px > Wl.len + err || py < -err || py > Wl.wid + err;
}

/* ------------------------------------------------------------------------ */
/* wave-cooperative sphere cull                                              */
/* ------------------------------------------------------------------------ */
/* Every lane of a wave scans the same primitive list, so the wave can cull the list
 * once for all its live rays: bound them by a cone (apex = centre of the origins' box,
 * widened by its half-diagonal rho; axis = mean direction; half-angle = the widest
 * direction), test 64 spheres at a time against it — lane l tests sphere c0 + l — and
 * ballot the survivors.  A ray o_i + t d_i (t >= 0) that meets ball(C, r) puts
 * o_c + t d_i inside ball(C, r + rho), so a sphere whose inflated ball misses the cone
 * is missed by every live ray: the exact per-lane test would reject it (det < 0 or no
 * positive root).  Margins (1e-4 relative + absolute) dwarf the fp32 error of the bound.
 * Cost per bounce: ten wave reductions + ceil(nS/64) cull passes; enabled by the host
 * when the scene is large enough to pay for it (KParams::wave_cull). */
/* Wave64 reductions returning a wave-uniform (scalar) value: a butterfly inside each
 * 16-lane row with DPP (xor 1, xor 2, half-mirror, mirror — each step leaves groups
 * uniform, so a mirror acts as the next xor), then the four row results read out with
 * v_readlane.  Every lane must be active (the bounce loops are converged). */
template <int CTRL>
__device__ __forceinline__ float dpp(float v) {
    return __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(v), CTRL, 0xF, 0xF, false));
}
__device__ __forceinline__ float lane_f(float v, int l) {
    return __int_as_float(__builtin_amdgcn_readlane(__float_as_int(v), l));
}
__device__ __forceinline__ float wsum(float v) {
    v += dpp<0xB1>(v);
    v += dpp<0x4E>(v);
    v += dpp<0x141>(v);
    v += dpp<0x140>(v);
    return (lane_f(v, 0) + lane_f(v, 16)) + (lane_f(v, 32) + lane_f(v, 48));
}
#ifndef RT_DPP_ASM
#define RT_DPP_ASM 1
#endif
#if RT_DPP_ASM
/* In IEEE mode fminf/fmaxf of a value the compiler cannot prove canonical (a DPP move,
 * a readlane) gets a v_max x,x,x canonicalise first, which also blocks folding the DPP
 * move into the min: five VALU per step.  The operands here are never NaN (origins,
 * cosines), so the steps are written as fused v_min/v_max_f32_dpp, one VALU each; the
 * four row results meet through row_bcast:15 / row_bcast:31 in lane 63.  s_nop 1 before
 * each DPP read covers the VALU-write -> DPP-read hazard the compiler cannot see. */
#define RT_WRED(OP)                                                                        \
    "s_nop 1\n\t" OP " %0, %0, %0 quad_perm:[1,0,3,2] row_mask:0xf bank_mask:0xf\n\t"      \
    "s_nop 1\n\t" OP " %0, %0, %0 quad_perm:[2,3,0,1] row_mask:0xf bank_mask:0xf\n\t"      \
    "s_nop 1\n\t" OP " %0, %0, %0 row_half_mirror row_mask:0xf bank_mask:0xf\n\t"          \
    "s_nop 1\n\t" OP " %0, %0, %0 row_mirror row_mask:0xf bank_mask:0xf\n\t"               \
    "s_nop 1\n\t" OP " %0, %0, %0 row_bcast:15 row_mask:0xa bank_mask:0xf\n\t"             \
    "s_nop 1\n\t" OP " %0, %0, %0 row_bcast:31 row_mask:0xc bank_mask:0xf\n\t"             \
    "s_nop 1"
__device__ __forceinline__ float wmin(float v) {
    asm volatile(RT_WRED("v_min_f32_dpp") : "+v"(v));
    return lane_f(v, 63);
}
__device__ __forceinline__ float wmax(float v) {
    asm volatile(RT_WRED("v_max_f32_dpp") : "+v"(v));
    return lane_f(v, 63);
}
#undef RT_WRED
#else
__device__ __forceinline__ float wmin(float v) {
    v = fminf(v, dpp<0xB1>(v));
    v = fminf(v, dpp<0x4E>(v));
    v = fminf(v, dpp<0x141>(v));
    v = fminf(v, dpp<0x140>(v));
    return fminf(fminf(lane_f(v, 0), lane_f(v, 16)), fminf(lane_f(v, 32), lane_f(v, 48)));
}
__device__ __forceinline__ float wmax(float v) {
    v = fmaxf(v, dpp<0xB1>(v));
    v = fmaxf(v, dpp<0x4E>(v));
    v = fmaxf(v, dpp<0x141>(v));
    v = fmaxf(v, dpp<0x140>(v));
    return fmaxf(fmaxf(lane_f(v, 0), lane_f(v, 16)), fmaxf(lane_f(v, 32), lane_f(v, 48)));
}
#endif
__device__ __forceinline__ float uni(float v) { return v; }  // reductions are already scalar
__device__ __forceinline__ double lane_d(double v, int l) {
    const long long b = __double_as_longlong(v);
    const int lo = __builtin_amdgcn_readlane((int)(b & 0xffffffff), l);
    const int hi = __builtin_amdgcn_readlane((int)(b >> 32), l);
    return __longlong_as_double(((long long)hi << 32) | (unsigned)lo);
}

struct Cone {
    f3 apex;
    f3 u;
    float rho, cos_t, sin_t, scale;
    bool on;
};

/* RT_CONE_AXIS_CHECK (default 0; 1 in rt_trace_ao.hip only): wave_cone rejects a non-finite
 * axis.  The sum of the live lanes' unit directions is exactly 0 when they cancel in pairs —
 * impossible to arrange with pixel rays, the rule with rt_render_ao's probes, which are +w_k in
 * some lanes and -w_k in the others. */
#ifndef RT_CONE_AXIS_CHECK
#define RT_CONE_AXIS_CHECK 0
#endif
__device__ __forceinline__ Cone wave_cone(f3 o, f3 d, bool alive) {
    Cone c;
    const float inf = __builtin_inff();
    const f3 lo = F3(uni(wmin(alive ? o.x : inf)), uni(wmin(alive ? o.y : inf)),
                     uni(wmin(alive ? o.z : inf)));
    const f3 hi = F3(uni(wmax(alive ? o.x : -inf)), uni(wmax(alive ? o.y : -inf)),
                     uni(wmax(alive ? o.z : -inf)));
    c.apex = (lo + hi) * 0.5f;
    const f3 ext = (hi - lo) * 0.5f;
    c.rho = fsqrt(fdot(ext, ext)) * 1.0001f;
    c.scale = fmax3abs(c.apex.x, c.apex.y, c.apex.z) + c.rho;
    const f3 dn = alive ? fnormalize(d) : F3(0.f, 0.f, 0.f);
    const f3 su = F3(uni(wsum(dn.x)), uni(wsum(dn.y)), uni(wsum(dn.z)));
    c.u = fnormalize(su);
    c.cos_t = uni(wmin(alive ? fdot(c.u, dn) : 1.0f)) - 1e-4f;
#if RT_CONE_AXIS_CHECK
    // live directions that cancel exactly (w and -w) leave su == 0 and a NaN axis; the dead
    // lanes' 1.0 then survives the minimum (fminf drops a NaN) and the cone would claim to be
    // narrow around a NaN axis, culling every sphere and wall: no cone instead
    if (!(fmax3abs(c.u.x, c.u.y, c.u.z) <= 2.0f)) c.cos_t = -1.0f;
#endif
    c.sin_t = fsqrt(fmaxf(0.0f, 1.0f - c.cos_t * c.cos_t));
    c.on = c.cos_t > 0.05f;  // a near-hemispherical fan culls nothing: skip the pass
    return c;
}

/* The primary segment's cone (RT_EYE_CONE): every primary ray starts at the camera, so the
 * apex is that shared origin (rho 0 — what wave_cone's box reductions return for equal
 * origins, without them), the axis the sum of the first and last live lanes' directions
 * (any axis is valid: the half-angle is measured against it), and one reduction remains:
 * the widest live direction. */
#ifndef RT_EYE_CONE
#define RT_EYE_CONE 1
#endif
__device__ __forceinline__ Cone wave_cone_eye(f3 o, f3 d, bool alive) {
    Cone c;
    const uint64_t am = __ballot(alive);
    const int l0 = am ? __builtin_ctzll(am) : 0;
    const int l1 = am ? 63 - __builtin_clzll(am) : 0;
    c.apex = F3(lane_f(o.x, l0), lane_f(o.y, l0), lane_f(o.z, l0));
    c.rho = 0.0f;
    c.scale = fmax3abs(c.apex.x, c.apex.y, c.apex.z);
    const f3 dn = alive ? fnormalize(d) : F3(0.f, 0.f, 0.f);
    c.u = fnormalize(F3(lane_f(dn.x, l0) + lane_f(dn.x, l1), lane_f(dn.y, l0) + lane_f(dn.y, l1),
                        lane_f(dn.z, l0) + lane_f(dn.z, l1)));
    c.cos_t = uni(wmin(alive ? fdot(c.u, dn) : 1.0f)) - 1e-4f;
    c.sin_t = fsqrt(fmaxf(0.0f, 1.0f - c.cos_t * c.cos_t));
    c.on = c.cos_t > 0.05f;
    return c;
}

/* Cull pass over spheres [c0, c0+64): lane l tests sphere c0 + l.  Returns the ballot of
 * survivors; *lb receives (in lane l) a lower bound on sphere c0+l's hit distance for any
 * live ray of the wave: |hit - o_i| >= |C - o_i| - r >= |C - apex| - rho - r. */
struct SphRec {
    float f[4];   // fp32 {cx, cy, cz, r} of sphere c0 + lane
    double d[4];  // fp64 {cx, cy, cz, r^2} (WANT64 && !RT_CULL_REC64_SCALAR only)
};
/* RT_CULL_REC64_SCALAR: the cull pass loads only the fp32 records (16 B per lane instead of
 * 48: ~1.5% of the spheres survive the cone), and each survivor's fp64 record comes in
 * afterwards by one wave-uniform scalar load (the index is a ballot bit) instead of eight
 * v_readlane from the testing lane's registers. */
#ifndef RT_CULL_REC64_SCALAR
#define RT_CULL_REC64_SCALAR 1
#endif
template <bool WANT64>
__device__ __forceinline__ uint64_t cull_chunk(const KParams& p, const Cone& cn, int c0,
                                               float* lb, SphRec& rec) {
    const int s = c0 + (int)(threadIdx.x & 63);
    bool keep = false;
    float bound = 0.0f;
    if (s < p.nS) {
        keep = true;
#pragma unroll
        for (int k = 0; k < 4; ++k) rec.f[k] = p.s32[s >> 2].c[k][s & 3];
        const float* S = rec.f;
        if (WANT64 && !RT_CULL_REC64_SCALAR) {
#pragma unroll
            for (int k = 0; k < 4; ++k) rec.d[k] = p.s64[s >> 2].v[s & 3][k];
        }
        const f3 v = F3(S[0], S[1], S[2]) - cn.apex;
        const float L2 = fdot(v, v);
        const float R = S[3] + cn.rho +
                        1e-4f * (1.0f + cn.scale + fmax3abs(S[0], S[1], S[2]) + S[3]);
        if (L2 > R * R) {  // apex outside the inflated ball
            const float il = frsq(L2);
            bound = fmaxf(0.0f, (L2 * il - R) * 0.9999f);
            if (cn.on) {
                const float sa = fminf(R * il, 1.0f);
                const float ca = fsqrt(fmaxf(0.0f, 1.0f - sa * sa));
                const float cphi = fdot(cn.u, v) * il;
                keep = cphi >= cn.cos_t * ca - cn.sin_t * sa - 1e-4f;
            }
        }
    }
    *lb = bound;
    const uint64_t m = __ballot(keep);
    // diagnostics (KParams::stats: [0] cull passes, [1] spheres kept, [2] spheres considered)
    if (p.stats != nullptr && (threadIdx.x & 63) == 0) {
        const int nin = p.nS - c0 < 64 ? p.nS - c0 : 64;
        atomicAdd(p.stats + 0, 1ull);
        atomicAdd(p.stats + 1, (unsigned long long)__popcll(m));
        atomicAdd(p.stats + 2, (unsigned long long)nin);
    }
    return m;
}

__device__ __forceinline__ RayF make_rayf(const RayD& r) {
    RayF rf;
    rf.o = F3((float)r.o.x, (float)r.o.y, (float)r.o.z);
    rf.d = F3((float)r.d.x, (float)r.d.y, (float)r.d.z);
    rf.a = fdot(rf.d, rf.d);
    rf.kb = CULL_K * fmax3abs(rf.d.x, rf.d.y, rf.d.z);
    rf.kdet = 8.0f * CULL_K * rf.a;
    rf.oinf = fmax3abs(rf.o.x, rf.o.y, rf.o.z);
    return rf;
}
/* DBL_MAX as an opaque scalar (SGPR pair): as a literal the register allocator of the deep
 * cull kernels kept it in a VGPR pair and spilled that to scratch, reloading it inside the
 * sphere loop; from SGPRs each use is a plain copy.  (The linear-scan kernels, which did not
 * spill, keep the literal: A/B c1 +2..12% otherwise.) */
#ifndef RT_DMAX_SGPR
#define RT_DMAX_SGPR 1
#endif
__device__ __forceinline__ double dbl_max_s() {
    if (!RT_DMAX_SGPR) return DBL_MAX;
    uint32_t lo, hi;
    asm("s_mov_b32 %0, -1" : "=s"(lo));
    asm("s_mov_b32 %0, 0x7fefffff" : "=s"(hi));
    return __longlong_as_double((long long)(((uint64_t)hi << 32) | lo));
}
__device__ __forceinline__ HitD no_hit() {
    HitD h;
    h.dist = DBL_MAX;
    h.pt = 0;
    h.slot = -1;
    return h;
}
/* sphere s (wave-uniform index), exact, behind the MIXED per-lane fp32 cull */
template <bool MIXED>
__device__ __forceinline__ void sphere_by_index(const KParams& p, int s, const RayD& r,
                                                const RayF& rf, HitD& h) {
    const float Sf[4] = {p.s32[s >> 2].c[0][s & 3], p.s32[s >> 2].c[1][s & 3],
                         p.s32[s >> 2].c[2][s & 3], p.s32[s >> 2].c[3][s & 3]};
    if (MIXED && sphere_cull(Sf, rf)) return;
    sphere_exact(p.s64[s >> 2].v[s & 3], s, r, h);
}
#ifndef RT_WALL_SLOAD  // 1: the cull kernels' wall records through scalar loads (asm)
#define RT_WALL_SLOAD 1
#endif
/* Wall w's fp64 record as two s_load_dwordx16 (the cull kernels: see clusters_mask's box
 * loads for why the compiler's own loads there go through the vector memory path). */
__device__ __forceinline__ Wall64 wall64_sload(const Wall64* q) {
    typedef int v16i __attribute__((ext_vector_type(16)));
    struct Two {
        v16i a, b;
    } t;
    asm volatile("s_load_dwordx16 %0, %2, 0x0\n\ts_load_dwordx16 %1, %2, 0x40\n\t"
                 "s_waitcnt lgkmcnt(0)"
                 : "=s"(t.a), "=s"(t.b)
                 : "s"(q)
                 : "memory");
    return __builtin_bit_cast(Wall64, t);
}
template <bool MIXED, bool EYE = false, bool SL = false>
__device__ __forceinline__ void walls_d(const KParams& p, const RayD& r, const RayF& rf, HitD& h) {
    for (int w = 0; w < p.nW; ++w) {
        if (MIXED && wall_cull(p.w32[w], rf)) continue;
        if (SL)
            wall_exact<EYE>(wall64_sload(p.w64 + w), w, p, r, h);
        else
            wall_exact<EYE>(p.w64[w], w, p, r, h);
    }
}

/* Walls against the wave's cone (RT_CULL_WALL_CONE): lane w tests wall w's circumscribed
 * ball (centre P + X len/2 + Y wid/2, radius half the diagonal: every point the exact test
 * can accept — the rectangle, its bounds checked in fp64 to ~1e-15 — lies in it) exactly as
 * cull_chunk tests a sphere, with the same margins; a wall whose inflated ball misses the
 * cone is missed by every live ray.  nW <= 64, all lanes active. */
/* May a ray of the cone meet ball(C, rad)?  cull_chunk's test and margins. */
__device__ __forceinline__ bool cone_ball(const Cone& cn, const f3 C, float rad) {
    const f3 v = C - cn.apex;
    const float L2 = fdot(v, v);
    const float R = rad + cn.rho + 1e-4f * (1.0f + cn.scale + fmax3abs(C.x, C.y, C.z) + rad);
    if (!(L2 > R * R)) return true;  // apex inside the inflated ball (or NaN): keep
    const float il = frsq(L2);
    const float sa = fminf(R * il, 1.0f);
    const float ca = fsqrt(fmaxf(0.0f, 1.0f - sa * sa));
    const float cphi = fdot(cn.u, v) * il;
    return cphi >= cn.cos_t * ca - cn.sin_t * sa - 1e-4f;
}
/* Wall w's circumscribed ball (fp32): the rectangle's centre and half its diagonal. */
__device__ __forceinline__ bool cone_wall(const Cone& cn, const Wall32& Wl) {
    const float hl = 0.5f * Wl.len, hw = 0.5f * Wl.wid;
    const f3 C = F3(fmaf(Wl.Y[0], hw, fmaf(Wl.X[0], hl, Wl.P[0])),
                    fmaf(Wl.Y[1], hw, fmaf(Wl.X[1], hl, Wl.P[1])),
                    fmaf(Wl.Y[2], hw, fmaf(Wl.X[2], hl, Wl.P[2])));
    return cone_ball(cn, C, fsqrt(fmaf(hl, hl, hw * hw)) * 1.0001f);
}
__device__ __forceinline__ uint64_t ballot_u(bool b) {
    const uint64_t m = __ballot(b);
    return ((uint64_t)__builtin_amdgcn_readfirstlane((unsigned)(m >> 32)) << 32) |
           __builtin_amdgcn_readfirstlane((unsigned)m);
}
__device__ __forceinline__ uint64_t wall_cone_mask(const KParams& p, const Cone& cn) {
    const int w = (int)(threadIdx.x & 63);
    return ballot_u(w < p.nW && cone_wall(cn, p.w32[w]));
}

/* The cull kernels' primary walls behind the wall pixel boxes (RT_CULL_WALL_BINS): only
 * the walls whose box meets the wave's tile (wave-uniform mask, bit w = wall w), in index
 * order as walls_d. */
template <bool MIXED>
__device__ __forceinline__ void walls_d_kept(const KParams& p, const RayD& r, const RayF& rf,
                                             HitD& h, uint64_t wm) {
    while (wm) {
        const int w = __builtin_ctzll(wm);
        wm &= wm - 1;
        if (MIXED && wall_cull(p.w32[w], rf)) continue;
        if (RT_WALL_SLOAD)
            wall_exact<false>(wall64_sload(p.w64 + w), w, p, r, h);
        else
            wall_exact<false>(p.w64[w], w, p, r, h);
    }
}

/* RT_SPH_PRECULL: the linear scans' unbinned segments (a bounce whose lanes follow no
 * common wall chain: every sphere is tested) run MIXED's conservative fp32 cull
 * (sphere_cull, the same predicate bit for bit) two spheres per packed instruction first,
 * and the exact test only where a lane's cull cannot prove the miss — at c2 ~9 of 10
 * exact sphere tests of such a scan reject every lane. */
#ifndef RT_SPH_PRECULL
#define RT_SPH_PRECULL 1
#endif
/* sphere_cull for spheres k0, k0 + 1 of group G in packed fp32 (v_pk_fma / v_pk_mul: each
 * element rounds as the scalar fmaf / * does, so the predicate is sphere_cull's). */
__device__ __forceinline__ void sphere_cull_pair(const SphG32& G, int k0, const RayF& r, bool& cull0,
                                                 bool& cull1) {
    const f2 cx = {G.c[0][k0], G.c[0][k0 + 1]}, cy = {G.c[1][k0], G.c[1][k0 + 1]};
    const f2 cz = {G.c[2][k0], G.c[2][k0 + 1]}, rr = {G.c[3][k0], G.c[3][k0 + 1]};
    const f2 ocx = f2(r.o.x) - cx, ocy = f2(r.o.y) - cy, ocz = f2(r.o.z) - cz;
    const f2 bh = __builtin_elementwise_fma(
        f2(r.d.x), ocx, __builtin_elementwise_fma(f2(r.d.y), ocy, f2(r.d.z) * ocz));
    const f2 cq = __builtin_elementwise_fma(
        -rr, rr, __builtin_elementwise_fma(ocx, ocx, __builtin_elementwise_fma(ocy, ocy, ocz * ocz)));
    const f2 det = __builtin_elementwise_fma(bh, bh, -f2(r.a) * cq);
    const float B0 = r.oinf + fmax3abs(cx.x, cy.x, cz.x) + rr.x;
    const float B1 = r.oinf + fmax3abs(cx.y, cy.y, cz.y) + rr.y;
    cull0 = (bh.x > r.kb * B0) || (det.x < -r.kdet * (B0 * B0));
    cull1 = (bh.y > r.kb * B1) || (det.y < -r.kdet * (B1 * B1));
}

/* Linear scan (no wave cull): groups of 4 spheres per scalar load.  EYE: the primary
 * segment, origin terms from the eye tables (rt_device.h). */
template <bool MIXED, bool EYE>
__device__ __forceinline__ HitD closest_hit_d(const KParams& p, const RayD& r) {
    DIAG(0);
    HitD h = no_hit();
    RayF rf;
    constexpr bool PRE_K = RT_SPH_PRECULL && !MIXED && !EYE;
    // (wave-uniform: scenes of a few spheres — c1's one — do not pay for the ray's fp32 copy,
    // A/B c1 +7%)
    const bool PRE = PRE_K && p.nS >= 4;
    if (MIXED || PRE) rf = make_rayf(r);
    const int ng = (p.nS + 3) >> 2;
    for (int g = 0; g < ng; ++g) {
        if (PRE) {
            const SphG32 G = p.s32[g];  // one s_load_dwordx16
            bool cu[4];
            sphere_cull_pair(G, 0, rf, cu[0], cu[1]);
            sphere_cull_pair(G, 2, rf, cu[2], cu[3]);
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                const int s = 4 * g + k;
                if (s < p.nS && !cu[k]) sphere_exact(p.s64[g].v[k], s, r, h);
            }
        } else if (MIXED) {
            const SphG32 G = p.s32[g];  // one s_load_dwordx16
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                const int s = 4 * g + k;
                const float Sf[4] = {G.c[0][k], G.c[1][k], G.c[2][k], G.c[3][k]};
                if (s < p.nS && !sphere_cull(Sf, rf)) {
                    if (EYE) {
                        const double* E = p.eye_s[s];
                        sphere_exact_oc(D3(E[0], E[1], E[2]), E[3], s, r, h);
                    } else {
                        sphere_exact(p.s64[g].v[k], s, r, h);
                    }
                }
            }
        } else if (EYE) {
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                const int s = 4 * g + k;
                const double* E = p.eye_s[s];
                if (s < p.nS) sphere_exact_oc(D3(E[0], E[1], E[2]), E[3], s, r, h);
            }
        } else {
            const SphG64 G = p.s64[g];  // two s_load_dwordx16
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                const int s = 4 * g + k;
                if (s < p.nS) sphere_exact(G.v[k], s, r, h);
            }
        }
    }
    walls_d<MIXED, EYE>(p, r, rf, h);
    return h;
}

/* Primary segment behind the tile bins (rt_device.h PrimBox): only the primitives whose
 * pixel box meets the wave's tile are tested, spheres in increasing index (the strict-<
 * tie rule holds: a skipped sphere cannot hit), then walls.  keep is wave-uniform. */
template <bool MIXED, bool EYE>
__device__ __forceinline__ HitD closest_hit_bin(const KParams& p, const RayD& r, uint64_t keep) {
    DIAG(0);
    HitD h = no_hit();
    RayF rf;
    if (MIXED) rf = make_rayf(r);
    uint64_t sm = p.nS >= 64 ? keep : keep & ((1ull << p.nS) - 1);
    while (sm) {
        const int s = __builtin_ctzll(sm);
        sm &= sm - 1;
        if (EYE) {
            const double* E = p.eye_s[s];
            sphere_exact_oc(D3(E[0], E[1], E[2]), E[3], s, r, h);
        } else {
            sphere_by_index<MIXED>(p, s, r, rf, h);
        }
    }
    uint64_t wm = p.nS >= 64 ? 0 : keep >> p.nS;
    if (EYE && RT_WALL_ORDER && p.wall_order_n == p.nW) {
        // primary rays: the walls nearest to the camera first (host order, KParams::
        // wall_order), so a wall behind the best hit skips its bounds test (t-skip); any
        // order finds the reference's winner (wall ties compare scene indices)
        uint64_t ord = p.wall_order;
        for (int k = 0; k < p.nW && wm; ++k, ord >>= 4) {
            const int w = (int)(ord & 15);
            if (!((wm >> w) & 1)) continue;
            wm &= ~(1ull << w);
            wall_exact<EYE>(p.w64[w], w, p, r, h);
        }
        return h;
    }
    while (wm) {
        const int w = __builtin_ctzll(wm);
        wm &= wm - 1;
        if (MIXED && wall_cull(p.w32[w], rf)) continue;
        wall_exact<EYE>(p.w64[w], w, p, r, h);
    }
    return h;
}

/* out_color, main.cpp:28-37: only normalize(v).z is used; z^0.25 as sqrt(sqrt(z)). */
__device__ __forceinline__ d3 sky_d(const RayD& r, double nvz) {
    if (r.d.z < 0.0) return ground_color();
    return lerp(sky_low(), sky_high(), sqrt_e(sqrt_e(nvz)));
}

/* Shading of one hit (main.cpp:99-104 + diffuse_shading + specular), returning
 * s = diffuse*kd + spec*ks + ka (local = color * s) and the (optional) sun scalar.
 * Shared normalisations are computed once: the same operations on the same operands
 * as the reference's repeated calls. */
struct ShadeD {
    double s;
    double ksun;
};
template <bool INT_EXP>
__device__ __forceinline__ ShadeD shade_d(const DevMat& m, const d3 pos, const d3 nn,
                                          const d3 view, bool sun) {
    const d3 ldir = normalize_e(D3(0.0 - pos.x, 0.0 - pos.y, 0.0 - pos.z));  // LIGHT_POS - pos
    const double lamb = dot(ldir, nn);
    const double diffuse = lamb > 0 ? lamb : 0;
    double res = dot(normalize_e(view + ldir), nn);
    res = res > 0 ? res : 0;
    const double spec = pow_e<INT_EXP>(res, m.ex);
    ShadeD sh;
    sh.s = diffuse * m.kd + spec * m.ks + m.ka;
    sh.ksun = 0;
    if (sun) {  // build-defined (rt_oracle.c sun_term)
        const d3 sd = normalize_e(sun_direction());
        double a = dot(sd, nn);
        a = a > 0 ? a : 0;
        double hs = dot(normalize_e(view + sd), nn);
        hs = hs > 0 ? hs : 0;
        sh.ksun = a * m.kd + pow_e<INT_EXP>(hs, m.ex) * m.ks;
    }
    return sh;
}

/* local = color * s (+ (SUN_COLOR * color) * ksun): identical operations at push and at
 * unwind. */
__device__ __forceinline__ d3 local_color_d(const DevMat& m, double s, double ksun, bool sun) {
    const d3 col = ld3(m.color);
    d3 L = col * s;
    if (sun) L = L + (sun_color() * col) * ksun;
    return L;
}

__device__ __forceinline__ RayD make_ray(d3 o, d3 d) {
    RayD r;
    r.o = o;
    r.d = d;
    r.a = lensq(d);
    r.ra = rcp_refined(r.a);
    r.dlen = sqrt_e(r.a);
    return r;
}
/* Origin and direction only: |d|^2, its reciprocal and |d| are formed by ray_terms when a
 * sphere test or a reflection needs them (wave-uniform decisions; walls and fp32 terminal
 * shading use none of them). */
__device__ __forceinline__ RayD make_ray_lazy(d3 o, d3 d) {
    RayD r;
    r.o = o;
    r.d = d;
    r.a = r.ra = r.dlen = 0.0;
    return r;
}
__device__ __forceinline__ void ray_terms(RayD& r) {
    r.a = lensq(r.d);
    r.ra = rcp_refined(r.a);
    r.dlen = sqrt_e(r.a);
}

/* fp32 shading of one hit for PATH64: the same formulas as shade_d on the exact fp64
 * geometry rounded to fp32 (colour only — nothing here feeds the next ray). */
__device__ __forceinline__ float2 shade_f(const DevMat32& m, const f3 pos, const f3 nn,
                                          const f3 nv, bool sun) {
    const float kd = m.kd, ks = m.ks, ka = m.ka, ex = m.ex;
    const f3 ldir = fnormalize(-pos);
    const float lamb = fmaxf(fdot(ldir, nn), 0.0f);
    const float res = fmaxf(fdot(fnormalize(ldir - nv), nn), 0.0f);
    float2 r;
    r.x = fmaf(lamb, kd, fmaf(fpow(res, ex), ks, ka));
    r.y = 0.0f;
    if (sun) {
        const f3 sd = fnormalize(F3(.7f, .4f, .7f));
        const float sa = fmaxf(fdot(sd, nn), 0.0f);
        const float hs = fmaxf(fdot(fnormalize(sd - nv), nn), 0.0f);
        r.y = fmaf(sa, kd, fpow(hs, ex) * ks);
    }
    return r;
}
__device__ __forceinline__ f3 local_color_f(const DevMat32& m, float s, float ksun, bool sun) {
    const f3 col = F3(m.color[0], m.color[1], m.color[2]);
    f3 L = col * s;
    if (sun) L = fmad3(F3(1.64f * col.x, 1.27f * col.y, 0.99f * col.z), ksun, L);
    return L;
}
__device__ __forceinline__ f3 tof(d3 v) { return F3((float)v.x, (float)v.y, (float)v.z); }

/* PATH64's terminal miss (out_color, main.cpp:28-37) in fp32: ground below the horizon by
 * the exact direction's sign, else the sky lerp at normalize(d).z^0.25. */
__device__ __forceinline__ f3 sky32(const d3& d) {
    const f3 nv32 = fnormalize(tof(d));
    if (d.z < 0.0) return F3(0.025f, 0.05f, 0.075f);
    const float tz = fsqrt(fsqrt(nv32.z));
    return F3(fmaf(tz, 0.14f - 0.36f, 0.36f), fmaf(tz, 0.21f - 0.45f, 0.45f),
              fmaf(tz, 0.49f - 0.57f, 0.57f));
}

/* find_closest_hit for one segment of every live lane: the wave-culled scan (CULL) or the
 * linear scan.  Converged: every lane of the wave calls it (alive masks the tests). */
/* Sphere clusters (rt_device.h Clu32/CluSph): a wide-cone wave's lanes each test their own
 * ray against the cluster boxes, then walk their own clusters — against the first split's
 * axis along the ray, so roughly near to far — skipping a cluster whose box entry already
 * lies beyond the lane's best hit, and run the exact test (order-independent tie rule) on
 * its spheres.  Conservative: the boxes are the balls' bounds widened by 1e-3 x the scene
 * extent, against fp32 slab errors ~1e-5 x extent for origins within 100 x the extent
 * (others test every cluster, unpruned); a skipped cluster's spheres lie at a world
 * distance >= t_entry |d| > best, so they lose even a tie.  slab_t: entry parameter of the
 * ray into the box (0 inside), +inf on a miss; NaN slab terms (origin on a box plane with
 * d = 0 there: the ray misses the ball by the margin) reject. */
/* RT_CLU_OCT: the lane walks its clusters near to far in the host's order for its
 * direction octant (Clu32::rank, KParams::cord); otherwise in index order, reversed when
 * the ray runs against the first split's axis. */
__device__ __forceinline__ int clu_octant(const f3 d) {
    return (d.x < 0.0f ? 1 : 0) | (d.y < 0.0f ? 2 : 0) | (d.z < 0.0f ? 4 : 0);
}
template <bool OCT>
__device__ __forceinline__ int clu_bit(const Clu32& B, int oct, int c) {
    if (!OCT) return c;
    const uint32_t lo = *reinterpret_cast<const uint32_t*>(B.rank);
    const uint32_t hi = *reinterpret_cast<const uint32_t*>(B.rank + 4);
    return (int)(((oct < 4 ? lo : hi) >> (8 * (oct & 3))) & 0xff);
}
#ifndef RT_CLU_FAST  // 1: the cluster box pass RT_CLU_UNROLL boxes per iteration (scalar loads in one
#define RT_CLU_FAST 1  // batch), slab planes as one fma each, the octant rank by one v_perm_b32,
#endif                 // a 32-bit candidate mask while nclu <= 32
#ifndef RT_CLU_UNROLL
#define RT_CLU_UNROLL 2
#endif
#ifndef RT_CLU_SCHED
#define RT_CLU_SCHED 1
#endif
#ifndef RT_CLU_SLOAD  // 1: the box pass's boxes through scalar loads (asm), see clusters_mask
#define RT_CLU_SLOAD 1
#endif
#ifndef RT_CULL_WALL_CONE  // 1: the cull kernels' bounce segments test only the walls whose
#define RT_CULL_WALL_CONE 1 // circumscribed ball meets the wave's cone (wall_cone_mask)
#endif
#ifndef RT_CULL_WALL_BINS  // 1: the cull kernels' primary segment tests only the walls whose
#define RT_CULL_WALL_BINS 1 // pixel box meets the tile (KParams::nwbox; spheres keep the cone)
#endif
/* Slab planes: RT_CLU_FAST forms (lo - o) / d as fma(lo, 1/d, -o/d) with o/d rounded once
 * per ray.  Its error along the ray, 2^-24 |o| |d| / |d_axis| per plane, scales with the
 * same 1 / |d_axis| as the box margin's slack (margin |d| / |d_axis|), so for origins within
 * clu_oinf (100 x the extent, margin 1e-3 x the extent) the widened box still contains the
 * balls' slabs.  d_axis = 0: NaN plane terms drop out of the min / max (no constraint),
 * which is conservative. */
/* RT_CLU_SLAB_FMA (default RT_CLU_FAST; 0 in rt_trace_ao.hip only): 1 = the fma form.  With a
 * direction component that is EXACTLY 0 and an origin off 0 on that axis, o/d = +-inf, and
 * fma(lo, +-inf, -+inf) is -+inf for one plane of a box that straddles 0 and NaN for the other:
 * the box is rejected although the ray may run through it (not conservative, unlike the NaN
 * case above).  Pixel and bounce rays do not have exact zeros; a caller's ray may, and so may
 * the probe directions of rt_render_ao (rt_ao_directions' first vector has y == 0), whose unit
 * forms (lo - o) * (1/d) instead. */
#ifndef RT_CLU_SLAB_FMA
#define RT_CLU_SLAB_FMA RT_CLU_FAST
#endif
struct SlabRay {
    f3 o, inv, oi;  // origin, 1/d, o/d (fma form)
};
__device__ __forceinline__ SlabRay slab_ray(const f3 o, const f3 d) {
    SlabRay r;
    r.o = o;
    r.inv = F3(1.0f / d.x, 1.0f / d.y, 1.0f / d.z);
    r.oi = F3(o.x * r.inv.x, o.y * r.inv.y, o.z * r.inv.z);
    return r;
}
__device__ __forceinline__ void slab_tt(const Clu32& B, const SlabRay& s, float& tn, float& tf) {
    float x1, x2, y1, y2, z1, z2;
    if (RT_CLU_SLAB_FMA) {
        x1 = fmaf(B.lo[0], s.inv.x, -s.oi.x), x2 = fmaf(B.hi[0], s.inv.x, -s.oi.x);
        y1 = fmaf(B.lo[1], s.inv.y, -s.oi.y), y2 = fmaf(B.hi[1], s.inv.y, -s.oi.y);
        z1 = fmaf(B.lo[2], s.inv.z, -s.oi.z), z2 = fmaf(B.hi[2], s.inv.z, -s.oi.z);
    } else {
        x1 = (B.lo[0] - s.o.x) * s.inv.x, x2 = (B.hi[0] - s.o.x) * s.inv.x;
        y1 = (B.lo[1] - s.o.y) * s.inv.y, y2 = (B.hi[1] - s.o.y) * s.inv.y;
        z1 = (B.lo[2] - s.o.z) * s.inv.z, z2 = (B.hi[2] - s.o.z) * s.inv.z;
    }
    tn = fmaxf(fmaxf(fminf(x1, x2), fminf(y1, y2)), fmaxf(fminf(z1, z2), 0.0f));
    tf = fminf(fminf(fmaxf(x1, x2), fmaxf(y1, y2)), fmaxf(z1, z2));
}
__device__ __forceinline__ float slab_t(const Clu32& B, const SlabRay& s) {
    float tn, tf;
    slab_tt(B, s, tn, tf);
    return tn <= tf ? tn : __builtin_inff();
}
/* The lane's candidate clusters as a bit mask: bit k = the cluster at rank k of the lane's
 * octant order (OCT) or cluster k, for the clusters whose box the lane's ray meets (every
 * cluster when !near).  RT_CLU_FAST: RT_CLU_UNROLL boxes per iteration (the clusters array holds
 * room for a multiple of four records; the rest are masked off by c < nclu). */
template <bool OCT, bool WIDE>
__device__ __forceinline__ uint64_t clusters_mask(const KParams& p, const SlabRay& s, bool alive,
                                                  bool near, int oct) {
    // rank of cluster c in the lane's octant order: byte `oct` of Clu32::rank
    const uint32_t sel = (uint32_t)oct | 0x0c0c0c00u;  // v_perm_b32: byte 0 <- byte oct, rest 0
    using M = typename std::conditional<WIDE, uint64_t, uint32_t>::type;
    M cm = 0;
    const int n4 = (p.nclu + 3) & ~3;
    for (int c0 = 0; c0 < n4; c0 += RT_CLU_UNROLL) {
        Clu32 Bs[RT_CLU_UNROLL];  // wave-uniform: one batch of scalar loads
#if RT_CLU_SLOAD
        // the compiler cannot prove that nothing in the cull kernels writes the boxes (the
        // DPP asm, the LDS stack), so it loads them through the vector memory path, one VMEM
        // round trip per iteration; read here as two s_load_dwordx8 instead (reads through
        // the scalar cache; the scene is constant while a kernel runs)
        static_assert(RT_CLU_UNROLL == 2 && sizeof(Clu32) == 32, "two 32-byte boxes per batch");
        {
            typedef int v8i __attribute__((ext_vector_type(8)));
            v8i r0, r1;
            const Clu32* q = p.clu + c0;
            asm volatile("s_load_dwordx8 %0, %2, 0x0\n\ts_load_dwordx8 %1, %2, 0x20\n\t"
                         "s_waitcnt lgkmcnt(0)"
                         : "=s"(r0), "=s"(r1)
                         : "s"(q)
                         : "memory");
            Bs[0] = __builtin_bit_cast(Clu32, r0);
            Bs[1] = __builtin_bit_cast(Clu32, r1);
        }
#else
#pragma unroll
        for (int u = 0; u < RT_CLU_UNROLL; ++u) Bs[u] = p.clu[c0 + u];
#endif
#pragma unroll
        for (int u = 0; u < RT_CLU_UNROLL; ++u) {
            // one box at a time (a handful of VGPRs), not four interleaved
            if (RT_CLU_SCHED) __builtin_amdgcn_sched_barrier(0);
            const int c = c0 + u;
            const Clu32& B = Bs[u];
            float tn, tf;
            slab_tt(B, s, tn, tf);
            const bool in = alive && c < p.nclu && (!near || tn <= tf);
            uint32_t bit = (uint32_t)c;
            if (OCT) {
                const uint32_t lo = *reinterpret_cast<const uint32_t*>(B.rank);
                const uint32_t hi = *reinterpret_cast<const uint32_t*>(B.rank + 4);
                bit = __builtin_amdgcn_perm(hi, lo, sel);
            }
            cm |= (M)in << bit;
        }
    }
    return (uint64_t)cm;
}
__device__ __forceinline__ void clusters_scan(const KParams& p, const RayD& r, bool alive, HitD& h) {
    const f3 o = F3((float)r.o.x, (float)r.o.y, (float)r.o.z);
    const f3 d = F3((float)r.d.x, (float)r.d.y, (float)r.d.z);
    const SlabRay sr = slab_ray(o, d);
    const bool near = fmax3abs(o.x, o.y, o.z) <= p.clu_oinf;
    const int oct = clu_octant(d);
    uint64_t cm = 0;  // bit k: the cluster at rank k of this lane's octant order
    if (RT_CLU_FAST) {
        cm = p.nclu <= 32 ? clusters_mask<RT_CLU_OCT, false>(p, sr, alive, near, oct)
                          : clusters_mask<RT_CLU_OCT, true>(p, sr, alive, near, oct);
    } else {
        for (int c = 0; c < p.nclu; ++c) {  // wave-uniform: scalar loads of the box
            const bool in = !near || slab_t(p.clu[c], sr) < __builtin_inff();
            cm |= (uint64_t)(alive && in) << clu_bit<RT_CLU_OCT>(p.clu[c], oct, c);
        }
    }
    const float dax = p.clu_axis == 0 ? d.x : (p.clu_axis == 1 ? d.y : d.z);
    const bool rev = !RT_CLU_OCT && dax < 0.0f;
    while (__any(cm != 0)) {
        if (cm != 0) {
            DIAG(6);  // (diagnostic build) one walk step: lanes with a cluster left
            const int k = rev ? 63 - __builtin_clzll(cm) : __builtin_ctzll(cm);
            cm &= ~(1ull << k);
            const int c = RT_CLU_OCT ? (int)p.cord[oct * CLU_MAX + k] : k;
            const float t = near ? slab_t(p.clu[c], sr) : 0.0f;
            if ((double)t * r.dlen * (1.0 - 1e-3) <= h.dist) {
                DIAG(14);  // (diagnostic build) lanes whose cluster is not pruned
                // leaves of CLU_SIZE_D, or CLU_SIZE for the scenes that need more than
                // CLU_MAX of those (unrolled as one CLU_SIZE loop: a runtime trip count made
                // the PATH64 cull kernel spill, A/B +10..17%)
                const CluSph* cs = p.csph + c * p.clu_ls;
#pragma unroll
                for (int k = 0; k < CLU_SIZE; ++k) {
                    if (k == CLU_SIZE_D && p.clu_ls == CLU_SIZE_D) break;
                    const int s = cs[k].slot;
                    if (s >= 0) sphere_exact<false>(cs[k].c, s, r, h, &p);
                }
            }
        }
    }
}

template <bool MIXED, bool CULL, bool CLU>
__device__ __forceinline__ HitD scan_d(const KParams& p, const RayD& r, bool alive,
                                       bool primary, bool binned, uint64_t keep) {
    HitD h = no_hit();
    if (CULL) h.dist = dbl_max_s();  // the deep kernels (see dbl_max_s)
    if (CULL) {
        // walls first: their distances then bound the sphere tests
        RayF rf;
        if (MIXED) rf = make_rayf(r);
        const f3 co = F3((float)r.o.x, (float)r.o.y, (float)r.o.z);
        const f3 cd = F3((float)r.d.x, (float)r.d.y, (float)r.d.z);
        const Cone cn = (RT_EYE_CONE && primary) ? wave_cone_eye(co, cd, alive)
                                                 : wave_cone(co, cd, alive);
        if (RT_WALLS_FIRST) {
            uint64_t wm = ~0ull;  // walls to test (bit w = wall w; walls past 63: all)
            if (RT_CULL_WALL_BINS && primary && binned)
                wm = keep;  // the primary segment: the walls' pixel boxes
            else if (RT_CULL_WALL_CONE && cn.on && p.nW > 0 && p.nW <= 64)
                wm = wall_cone_mask(p, cn);  // the bounces: the wave's cone
            if (alive) {
                if (wm != ~0ull)
                    walls_d_kept<MIXED>(p, r, rf, h, wm);
                else
                    walls_d<MIXED, false, RT_WALL_SLOAD>(p, r, rf, h);
            }
        }
        // a wide cone (live rays pointing everywhere) culls little: each lane its own clusters
        // (every precision since round 3: with the recursion stack in LDS the fp64-colour
        // kernels have the registers for it — A/B c5 F64 -44%, MIXED -36%, c3 -9..15%; in
        // round 2 it cost c3 F64 +40%)
        const bool clusters = RT_CLUSTERS && CLU && p.nclu > 0 && cn.cos_t < p.clu_cos;
#if RT_DIAG
        if (alive) DIAG(0);  // wave-level segments of the cull kernels (tools/diag_run.py --cull)
        if (clusters && alive) DIAG(4);
#endif
        if (clusters) clusters_scan(p, r, alive, h);
        for (int c0 = 0; !clusters && c0 < p.nS; c0 += 64) {
            float lb;
            SphRec rec;
            uint64_t m = cull_chunk<true>(p, cn, c0, &lb, rec);
            // survivors in index order; each record comes out of the testing lane's
            // registers (v_readlane), no memory round trip
            while (m) {
                const int l = __builtin_ctzll(m);
                m &= m - 1;
                const double bound = (double)lane_f(lb, l);
                // exact skip: the sphere's distance is >= bound > this lane's best
                if (alive && bound <= h.dist) {
                    DIAG(12);  // (diagnostic build) one cone survivor tested
                    const int sidx = c0 + l;
                    const float Sf[4] = {lane_f(rec.f[0], l), lane_f(rec.f[1], l),
                                         lane_f(rec.f[2], l), lane_f(rec.f[3], l)};
                    if (!(MIXED && sphere_cull(Sf, rf))) {
                        if (RT_CULL_REC64_SCALAR) {
                            sphere_exact<false>(p.s64[sidx >> 2].v[sidx & 3], sidx, r, h, &p);
                        } else {
                            const double Sd[4] = {lane_d(rec.d[0], l), lane_d(rec.d[1], l),
                                                  lane_d(rec.d[2], l), lane_d(rec.d[3], l)};
                            sphere_exact<false>(Sd, sidx, r, h, &p);
                        }
                    }
                }
            }
        }
        if (!RT_WALLS_FIRST && alive) walls_d<MIXED>(p, r, rf, h);
    } else if (alive) {
        // primary, p.eye and p.bins are wave-uniform: one scan or another per wave (MIXED
        // keeps its fp32 cull in front of every test: no eye tables, A/B +1.5%)
        if (binned) {
            h = (!MIXED && primary && p.eye) ? closest_hit_bin<MIXED, true>(p, r, keep)
                                             : closest_hit_bin<MIXED, false>(p, r, keep);
        } else {
            h = (!MIXED && primary && p.eye) ? closest_hit_d<MIXED, true>(p, r)
                                             : closest_hit_d<MIXED, false>(p, r);
        }
    }
    return h;
}

#if RT_SHADOW
#include "rt_anyhit.h"

/* RT_FLAG_SHADOWS: is the light hidden from the hit h of ray r?  The segment from
 * sp = pos + col.normal * .0001 (main.cpp:111's start point: pos as main.cpp:99 forms it, a
 * sphere's world distance used as t; the normal un-normalised) to LIGHT_POS = (0,0,0), i.e.
 * direction LIGHT_POS - sp and limit T = 1, through the any-hit scan of the occlusion query —
 * the linear scan, or the cull kernels' cone / cluster walk over the lanes that have a hit.
 * Called converged (the cone's wave reductions need every lane present): lanes without a hit
 * carry a harmless ray and take part only through todo == false.  Exact fp64 in every
 * precision: pos and N are formed here again in fp64 whatever the caller shades in. */
template <bool CULL>
__device__ __forceinline__ bool light_blocked(const KParams& p, const RayD& r, const HitD& h,
                                              bool alive) {
    const bool open = alive && h.slot >= 0;
    if (!__any(open)) return false;  // wave-uniform
    d3 sp = D3(0.0, 0.0, 1.0);
    if (open) {
        const d3 pos = r.o + r.d * h.dist;
        d3 N;
        if (h.slot < p.nS) {
            const double* S = p.s64[h.slot >> 2].v[h.slot & 3];
            N = (r.o + r.d * h.pt) - D3(S[0], S[1], S[2]);
        } else {
            N = ld3(p.w64[h.slot - p.nS].n);
        }
        sp = pos + N * .0001;
    }
    const RayD sr = make_ray(sp, D3(0.0 - sp.x, 0.0 - sp.y, 0.0 - sp.z));
    bool todo = open;
    if (CULL)
        occluded_cull(p, sr, todo, 1.0);
    else
        occluded_linear(p, sr, todo, 1.0);
    return open && !todo;
}
#endif

#if RT_LIGHTS
#include "rt_anyhit.h"

/* Scene lights (rt_set_lights, rt_capi.h "Lights").  The lights units rename KParams to their
 * KParamsL, which carries the light records behind the frame's arguments (p.lights).
 *
 * lights_blocked: light_blocked for every light — bit l of the result = the segment from
 * sp = pos + col.normal * .0001 to light l's position is occluded (direction P_l - sp, T = 1,
 * rt_occluded's definition).  RT_FLAG_SHADOWS is a wave-uniform runtime branch: without it no
 * light ray is shot.  pos, N and sp are formed once, in fp64 whatever the caller shades in.
 * Called converged, as light_blocked. */
template <bool CULL>
__device__ __forceinline__ unsigned lights_blocked(const KParams& p, const RayD& r, const HitD& h,
                                                   bool alive) {
    if (!(p.flags & FLAG_SHADOWS)) return 0u;  // wave-uniform
    const bool open = alive && h.slot >= 0;
    if (!__any(open)) return 0u;  // wave-uniform
    d3 sp = D3(0.0, 0.0, 1.0);
    if (open) {
        const d3 pos = r.o + r.d * h.dist;
        d3 N;
        if (h.slot < p.nS) {
            const double* S = p.s64[h.slot >> 2].v[h.slot & 3];
            N = (r.o + r.d * h.pt) - D3(S[0], S[1], S[2]);
        } else {
            N = ld3(p.w64[h.slot - p.nS].n);
        }
        sp = pos + N * .0001;
    }
    unsigned dark = 0u;
    for (int l = 0; l < p.lights.n; ++l) {
        const d3 P = ld3(p.lights.l[l].pos);
        const RayD sr = make_ray(sp, D3(P.x - sp.x, P.y - sp.y, P.z - sp.z));
        bool todo = open;
        if (CULL)
            occluded_cull(p, sr, todo, 1.0);
        else
            occluded_linear(p, sr, todo, 1.0);
        dark |= (open && !todo) ? (1u << l) : 0u;
    }
    return dark;
}

/* Shading of one hit under the lights, fp64 (rt_capi.h's formula, one IEEE operation per
 * written operation): per light diffuse_shading and specular as shade_d forms them with
 * LIGHT_POS = P_l, s_l = diff*kd + spec*ks (+0.0 where bit l of dark is set), then per channel
 * acc = C_l * s_l summed in light order.  Returns acc + ka per channel: local = color * that,
 * the value the recursion stack keeps per level.  One light {(0,0,0), (1,1,1)} gives shade_d's
 * s in every channel (1.0 * s == s). */
template <bool INT_EXP>
__device__ __forceinline__ d3 shade_lights_d(const KParams& p, const DevMat& m, const d3 pos,
                                             const d3 nn, const d3 view, unsigned dark) {
    d3 acc = D3(0.0, 0.0, 0.0);
    for (int l = 0; l < p.lights.n; ++l) {
        const d3 P = ld3(p.lights.l[l].pos);
        const d3 ldir = normalize_e(D3(P.x - pos.x, P.y - pos.y, P.z - pos.z));  // P_l - pos
        const double lamb = dot(ldir, nn);
        const double diffuse = lamb > 0 ? lamb : 0;
        double res = dot(normalize_e(view + ldir), nn);
        res = res > 0 ? res : 0;
        const double spec = pow_e<INT_EXP>(res, m.ex);
        double s = diffuse * m.kd + spec * m.ks;
        if ((dark >> l) & 1u) s = 0.0;
        const d3 t = ld3(p.lights.l[l].col) * s;
        acc = l == 0 ? t : acc + t;
    }
    return D3(acc.x + m.ka, acc.y + m.ka, acc.z + m.ka);
}
/* The same for PATH64's fp32 colour (shade_f's formulas per light).  pos is the exact fp64 hit
 * position: P_l - pos is formed in fp64 and rounded once, so a light close to a surface costs
 * no more relative error than a distant one. */
__device__ __forceinline__ f3 shade_lights_f(const KParams& p, const DevMat32& m, const d3 pos,
                                             const f3 nn, const f3 nv, unsigned dark) {
    const float kd = m.kd, ks = m.ks, ex = m.ex;
    f3 acc = F3(0.f, 0.f, 0.f);
    for (int l = 0; l < p.lights.n; ++l) {
        const d3 P = ld3(p.lights.l[l].pos);
        const f3 ldir = fnormalize(tof(D3(P.x - pos.x, P.y - pos.y, P.z - pos.z)));
        const float lamb = fmaxf(fdot(ldir, nn), 0.0f);
        const float res = fmaxf(fdot(fnormalize(ldir - nv), nn), 0.0f);
        float s = fmaf(lamb, kd, fpow(res, ex) * ks);
        if ((dark >> l) & 1u) s = 0.0f;
        const float* C = p.lights.l[l].colf;
        acc = F3(fmaf(C[0], s, acc.x), fmaf(C[1], s, acc.y), fmaf(C[2], s, acc.z));
    }
    return F3(acc.x + m.ka, acc.y + m.ka, acc.z + m.ka);
}
__device__ __forceinline__ d3 mul3(const double* c, d3 v) { return D3(c[0] * v.x, c[1] * v.y, c[2] * v.z); }
__device__ __forceinline__ f3 mul3(const float* c, f3 v) { return F3(c[0] * v.x, c[1] * v.y, c[2] * v.z); }
#endif

#if RT_GLASS
/* Transmission (rt_set_transmission, rt_capi.h "Transmission").  The glass units rename KParams
 * to their KParamsG, which carries the table of per-slot records behind the light records
 * (p.glass.rec).  At a hit whose record has tau > 0 the path goes on with the ray that passes
 * through the object instead of the reflected one; fp64 in every precision, one IEEE operation
 * per written operation (this TU: -ffp-contract=off; sqrt_e, normalize_e and div_r round
 * correctly). */
struct NextRay {
    d3 o, d;
};
/* A wall is a thin pane: the ray goes on unbent from just behind the side it came to.  pos:
 * main.cpp:99's point, n: the stored normal. */
__device__ __forceinline__ NextRay glass_pane(const d3 pos, const d3 n, const d3 d) {
    const double f = dot(d, n);
    const d3 nf = f > 0 ? -n : n;
    return {pos - nf * .0001, d};
}
/* A sphere of centre c: refract in at P (scene.cpp:75's intersection point), follow the chord to
 * the far side Q in closed form — Sphere::intersect never reports the far root, and whatever lies
 * inside the ball is ignored — and refract out.  dh = normalize(d), nh = normalize(P - c).
 * ior >= 1, so entry never reflects totally; at the exit k2 == ci^2 in exact arithmetic and the
 * clamp only meets rounding. */
__device__ __forceinline__ NextRay glass_sphere(const d3 P, const d3 c, const d3 dh, const d3 nh,
                                                double ior) {
    const double ci = -dot(dh, nh);
    const double eta = 1.0 / ior;
    const double k = 1.0 - (eta * eta) * (1.0 - ci * ci);
    const d3 t = dh * eta + nh * (eta * ci - sqrt_e(k));
    const d3 m = c - P;
    const double s = (2.0 * dot(t, m)) / dot(t, t);
    const d3 Q = P + t * s;
    const d3 n2 = Q - c;
    const d3 n2h = normalize_e(n2);
    const d3 th = normalize_e(t);
    const double c2 = dot(th, n2h);
    const double k2 = 1.0 - (ior * ior) * (1.0 - c2 * c2);
    const double k2c = k2 > 0 ? k2 : 0.0;
    return {Q + n2 * .0001, th * ior + n2h * (sqrt_e(k2c) - ior * c2)};
}
/* The next ray of a transmissive hit (g.tau > 0) of ray r at slot: P = r.o + r.d * h.pt for a
 * sphere, pos = r.o + r.d * h.dist for a wall; N the record normal, nv and nn the normalised
 * direction and normal the shading step formed. */
__device__ __forceinline__ NextRay glass_next(const KParams& p, const DevGlass& g, const RayD& r,
                                              const HitD& h, const d3 pos, const d3 N, const d3 nv,
                                              const d3 nn) {
    if (h.slot < p.nS) {
        const double* S = p.s64[h.slot >> 2].v[h.slot & 3];
        return glass_sphere(r.o + r.d * h.pt, D3(S[0], S[1], S[2]), nv, nn, g.ior);
    }
    return glass_pane(pos, N, r.d);
}
#endif

/* ------------------------------------------------------------------------ */
/* epilogue: pixel store, segment count, occupancy targets                   */
/* ------------------------------------------------------------------------ */
/* RGBA8: clamp to [0,1] then truncate v*255, the in-range behaviour of
 * SDL_MapRGB(val*255) with its implicit double->Uint8 conversion (main.cpp:345). */
__device__ __forceinline__ unsigned q8(double v) {
    v = v > 0.0 ? v : 0.0;  // NaN -> 0
    v = v < 1.0 ? v : 1.0;
    return (unsigned)(v * 255.0);
}
/* RGBA8_WRAP: the reference's x86-64 bytes for every value — cvttsd2si of v*255 (int32,
 * toward zero; NaN and |v*255| >= 2^31 give 0x80000000), then the low byte. */
__device__ __forceinline__ unsigned q8_wrap(double v) {
    const double t = v * 255.0;
    const int i = (t > -2147483649.0 && t < 2147483648.0) ? (int)t : (int)0x80000000u;
    return (unsigned)i & 0xffu;
}

__device__ __forceinline__ void store_px(const KParams& p, size_t px, double cr, double cg,
                                         double cb) {
    if (p.outf == OUT_RGB_F32) {
        float* o = static_cast<float*>(p.out) + px * 3;
        o[0] = (float)cr;
        o[1] = (float)cg;
        o[2] = (float)cb;
    } else if (p.outf == OUT_RGB_F64) {
        double* o = static_cast<double*>(p.out) + px * 3;
        o[0] = cr;
        o[1] = cg;
        o[2] = cb;
    } else if (p.outf == OUT_RGBA8) {
        const unsigned v = q8(cr) | (q8(cg) << 8) | (q8(cb) << 16) | (255u << 24);
        static_cast<unsigned*>(p.out)[px] = v;
    } else {
        const unsigned v = q8_wrap(cr) | (q8_wrap(cg) << 8) | (q8_wrap(cb) << 16) | (255u << 24);
        static_cast<unsigned*>(p.out)[px] = v;
    }
}
__device__ __forceinline__ void store_pixel(const KParams& p, int r, int x, double cr, double cg,
                                            double cb) {
    store_px(p, (size_t)r * (size_t)p.W + (size_t)x, cr, cg, cb);
}

__device__ __forceinline__ void count_segments(const KParams& p, int segs) {
    if (p.segs == nullptr) return;
    for (int off = 32; off > 0; off >>= 1) segs += __shfl_xor(segs, off, 64);  // wave64 sum
    if ((threadIdx.x & 63) == 0) atomicAdd(p.segs, (unsigned long long)segs);
}

/* Occupancy target per instantiation (waves per SIMD; MI355X_MICROARCH.md: <= 128 VGPRs
 * for 4, <= 96 for 5).  The fp64-colour paths carry the most state. */
template <int PREC, bool SUN, bool INT_EXP, bool CULL, int MAXD>
constexpr int waves_per_eu() {
    // The register stack costs 2-5 VGPRs per level and the cull's per-lane records ~12, so
    // the target steps down with depth tier and cull.  Checked with `make asm`
    // (ScratchSize 0 for every no-sun integer-exponent variant; the rare sun +
    // non-integer-exponent deep fp64 variants run at 2 waves and may spill a little).
    const int tier = MAXD >= 16 ? 2 : (MAXD >= 10 ? 1 : 0);
    int w = 0;
    if (PREC == PREC_F64 && !CULL && !SUN && tier == 0) return 4;
    if (PREC == PREC_F32)
        // (cull kernels one wave more since the sphere clusters: A/B c5 -4%, c3 -1% vs 5)
        w = 5 - (tier > 0 ? 1 : 0) - ((SUN && tier == 2) ? 1 : 0) +
            ((CULL && !SUN && tier == 0) ? 1 : 0);
    else if (PREC == PREC_PATH64)
        // (5 waves: A/B c5 -7%, c3 -5% with 20 B of spills in the cull kernels; the sun
        // variants, whose spills would be 56-96 B, keep 4)
        w = RT_WPE_PATH64 - (tier == 2 ? 1 : 0) - (SUN ? 1 : 0) +
            ((CULL && !SUN && tier == 0) ? RT_WPE_PATH64_CULL_BONUS : 0);
    else
        w = (INT_EXP ? (SUN ? 3 : 4) : (SUN ? 2 : 3)) - (tier > 0 ? 1 : 0) -
            ((PREC == PREC_MIXED && CULL && MAXD >= 8) ? RT_WPE_MIXED_CULL_DROP : 0) +
            (CULL ? RT_WPE_CULL64_BONUS : 0);
    return w < 2 ? 2 : w;
}
/* The shadow kernels (RT_SHADOW) keep the hit, the ray and the recursion state live across
 * the light ray's scan: at their twins' targets the linear-scan kernels and the shallow PATH64
 * cull kernels spilled 40-300 B per lane (`make asm`), so those run one wave per SIMD lower. */
template <int PREC, bool CULL, int MAXD>
constexpr int shadow_waves(int w) {
#if RT_LIGHTS
    {  // the lights kernels carry the shadow kernels' state across the light loop: their
        // targets, capped by what the per-level colour stack in LDS admits (three values and
        // the material slot per level and lane, one wave per workgroup, 160 KB per CU)
        // (and one wave less for the shallow fp64-colour cull kernels, which spilled 68 B at 5)
        const int drop = !CULL ? 1 : ((PREC == PREC_PATH64 ? MAXD < 10 : MAXD < 8) ? 1 : 0);
        const int lds = MAXD * 64 * (3 * (PREC == PREC_PATH64 ? 4 : 8) + 4);
        const int cap = (160 * 1024 / lds + 3) / 4;
        const int t = w - drop < cap ? w - drop : cap;
        return t < 2 ? 2 : t;
    }
#endif
    if (!RT_SHADOW) return w;
    const int drop = !CULL ? 1 : ((PREC == PREC_PATH64 && MAXD < 10) ? 1 : 0);
    return w - drop < 2 ? 2 : w - drop;
}

