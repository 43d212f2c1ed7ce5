/*
 * rt_capi.h — the C-ABI drop-in boundary of the MI355X trace/shade path.
 *
 * The reference renders a frame with one C++ call,
 *     void rt_scene(std::vector<vec3> u, const std::vector<std::unique_ptr<SceneGeometry>>& scene,
 *                   const Camera& cam, std::vector<std::vector<RGB>>& frame_buffer);
 * (/root/reference/main.cpp:124-139), which walks every pixel through
 * recursive_ray_tracing (main.cpp:89-119) -> find_closest_hit (main.cpp:67-84) ->
 * the virtual SceneGeometry::intersect plugin (scene.h:57; Sphere::intersect
 * scene.cpp:40-78, Wall::intersect scene.cpp:4-35).
 *
 * This header is what a host program binds instead: plain C, plain pointers and
 * sizes, no C++ or torch types.  The C++ API mirror (include/rt/scene.h) flattens its
 * SceneGeometry objects into rt_prim records and calls these entry points; a cgo /
 * ctypes / N-API binding binds them directly.
 *
 * Conventions (the reference has no error returns; .at() throws — main.cpp:136):
 *   - every entry point returns int status, RT_OK == 0; rt_strerror() names it;
 *   - no exception crosses the boundary;
 *   - a ctx is used by one host thread at a time; calls on a ctx are serialised;
 *   - the caller owns every buffer passed in; the ctx owns its device copies.
 */
#ifndef RT_CAPI_H
#define RT_CAPI_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* Version 2 adds the multi-GPU frame operator (rt_multi_*) and RT_ERR_COMM; every version-1
 * entry point keeps its signature and meaning (the ABI grows additively).  The ray queries
 * (rt_hit, rt_trace_rays, rt_trace_rays_device, then rt_occluded, rt_occluded_device) arrived
 * within version 2: purely additive. */
#define RT_CAPI_VERSION 2

/* ---- status codes ------------------------------------------------------- */
enum rt_status {
    RT_OK = 0,
    RT_ERR_INVALID_ARG = 1,   /* null pointer, bad size, bad enum */
    RT_ERR_NO_DEVICE = 2,     /* no HIP device / device index out of range */
    RT_ERR_HIP = 3,           /* a HIP runtime call failed (rt_last_hip_error) */
    RT_ERR_OUT_OF_MEMORY = 4,
    RT_ERR_NO_SCENE = 5,      /* rt_render* before rt_set_scene */
    RT_ERR_UNSUPPORTED = 6,   /* depth / flag combination this build does not ship */
    RT_ERR_OUT_OF_RANGE = 7,  /* row band outside the image (reference: std::out_of_range) */
    RT_ERR_COMM = 8           /* an RCCL call failed (rt_multi_last_error names it) */
};

/* ---- scene records (reference scene.h:35-84) ---------------------------- */

/* Material — scene.h:35-49.  NOTE the reference constructor's positional order is
 * (color, metallic, ambient, diffuse, specular, specular_exponent) with defaults
 * .5/.1/.9/.4/50 (scene.h:48); the fields here are named, so order is irrelevant. */
typedef struct rt_material {
    double color[3];
    double ambient;
    double metallic;
    double diffuse;
    double specular;
    double specular_exponent;
} rt_material;

enum rt_prim_kind {
    RT_PRIM_SPHERE = 0,   /* Sphere, scene.h:75-84 */
    RT_PRIM_WALL = 1      /* Wall,   scene.h:62-73 */
};

/* One SceneGeometry object, flattened.  Fields hold the OBJECT STATE, i.e. what the
 * reference constructors store: Wall's normal is already normalised (scene.h:73
 * normalises in the initialiser list), position is the wall's corner (scene.cpp:30). */
typedef struct rt_prim {
    int32_t kind;          /* rt_prim_kind */
    int32_t reserved;      /* must be 0 */
    rt_material mat;
    double position[3];    /* Sphere::center | Wall::position */
    double normal[3];      /* Wall::normal (unit); ignored for spheres */
    double radius;         /* Sphere::radius */
    double length;         /* Wall::length */
    double width;          /* Wall::width */
} rt_prim;

/* The per-frame camera inputs of rt_scene (main.cpp:132-134): position plus the
 * Camera::init outputs image_top_left and the returned {pixel_delta_x, pixel_delta_y}
 * (scene.cpp:80-106).  They are passed explicitly (not recomputed from lookat)
 * because the reference never re-calls init() after a camera move (main.cpp:154),
 * so a moved camera keeps a stale image_top_left — a drop-in must reproduce that. */
typedef struct rt_camera {
    double position[3];
    double image_top_left[3];
    double pixel_delta_x[3];   /* u[0] in rt_scene */
    double pixel_delta_y[3];   /* u[1] in rt_scene */
    int32_t width;             /* cam.image_width */
    int32_t height;            /* cam.image_height */
} rt_camera;

/* ---- render options ----------------------------------------------------- */
enum rt_precision {
    RT_PREC_F64 = 0,     /* fp64 everywhere, op-for-op the reference's arithmetic (parity) */
    RT_PREC_F32 = 1,     /* fp32 everywhere (throughput; flips at discontinuities) */
    RT_PREC_MIXED = 2,   /* fp32 conservative cull + fp64 exact on survivors: output == F64 */
    RT_PREC_PATH64 = 3   /* F64's exact ray paths (hits, normals, reflections) + fp32 colour
                            arithmetic: no discontinuity flips, colours within ~1e-6 */
};

/* The reference's only post-step is SDL_MapRGB(format, val.x*255, ...) (main.cpp:345),
 * whose Uint8 parameters take the double by implicit conversion.  For 0 <= v*255 < 256
 * that truncates toward zero; above (local colour can reach color*1.4: diffuse .9 +
 * specular .4 + ambient .1) the conversion is undefined in C++, and the reference's
 * x86-64 build (g++ -O3: cvttsd2si, then the low byte) WRAPS modulo 256 — a highlight of
 * 1.084 displays as 20.  RT_OUT_RGBA8 deliberately deviates there and saturates at 255
 * (the tone-map epilogue); RT_OUT_RGBA8_WRAP reproduces the x86-64 bytes exactly
 * (tests/golden/surface.npz, recorded from that conversion compiled by g++). */
enum rt_out_format {
    RT_OUT_RGB_F32 = 0,  /* H x W x 3 float, row-major, linear unclamped RGB (12 B/px) */
    RT_OUT_RGB_F64 = 1,  /* H x W x 3 double (24 B/px) — exact drop-in for vector<vector<RGB>> */
    RT_OUT_RGBA8 = 2,    /* H x W x 4 uint8 (R,G,B,255): trunc(clamp(v,0,1)*255).  Equals
                            main.cpp:345 for in-range pixels; saturates (a deliberate
                            deviation) where the reference's conversion wraps */
    RT_OUT_RGBA8_WRAP = 3 /* H x W x 4 uint8 (R,G,B,255): (uint8)(int32)trunc(v*255), i.e.
                            main.cpp:345's bytes on x86-64 for every value, out-of-range
                            (wraps mod 256) and NaN (0) included */
};

enum rt_flags {
    RT_FLAG_SUN = 1u << 0,  /* build-defined sun term (SUN_COLOR/SUN_DIRECTION, main.cpp:18-19,
                               defined but unused by the reference); off = reference parity */
    RT_FLAG_SHADOWS = 1u << 1
    /* Hard shadows (off by default; off = reference parity, nothing changes).  At EVERY
     * accepted hit of recursive_ray_tracing — every level, the last included, for frames and
     * for ray-batch radiance — a ray is traced to the point light LIGHT_POS (main.cpp:14, the
     * origin):
     *   origin     sp = pos + col.normal * .0001   (main.cpp:111's start point: pos as
     *              main.cpp:99 forms it, the normal un-normalised)
     *   direction  sd = LIGHT_POS - sp = (0,0,0) - sp,  limit T = 1
     * The hit is SHADOWED iff that segment is occluded by rt_occluded's definition: some object
     * has c.distance > 0 and its parameter (a wall's t, a sphere's `projection`) is <= 1,
     * compared in fp64 on the exact values; the hit object itself takes part like any other.
     * A shadowed hit has diffuse_intensity = specular_intensity = 0, so local_color =
     * mat.color * mat.ambient.  Ray paths, the sky and the metallic lerp are untouched.
     * Shadow rays are not counted: d_segments / rt_stats::segments equal the unshadowed
     * frame's.  sp == 0 exactly is unspecified.
     * The decision runs on the exact fp64 path in every supported precision: RT_PREC_F64 and
     * RT_PREC_PATH64 decide with the same bits (PATH64 keeps its fp32 colour); RT_PREC_MIXED
     * is served by the F64 shadow kernels (output == F64).
     * RT_ERR_UNSUPPORTED, before any launch: RT_PREC_F32 with the flag; RT_FLAG_SUN |
     * RT_FLAG_SHADOWS; rt_tile_row_costs with the flag.
     * With the flag set RT_OPT_PIXEL_PAIRS is ignored, RT_OPT_FRAME_BATCH launches such
     * frames one at a time, RT_OPT_ROW_FEEDBACK neither samples nor reorders them, and
     * RT_OPT_SUPERSAMPLE works (every sample is shadowed, the resolve is unchanged).  Row
     * bands, rt_render_device_interleaved and rt_multi_* work as without it (pixels are
     * independent).  rt_trace_rays* with out == NULL, rt_occluded* and rt_frame_boxes ignore
     * the flag.  Other flag bits stay ignored. */
};

typedef struct rt_stats {
    double ms;             /* device time of the render (hipEvent), milliseconds */
    uint64_t segments;     /* closest-hit queries issued (only when counting was asked) */
} rt_stats;

typedef struct rt_ctx rt_ctx;

/* ---- lifecycle ---------------------------------------------------------- */
int rt_ctx_create(int device, rt_ctx** out);
int rt_ctx_destroy(rt_ctx* ctx);
const char* rt_strerror(int status);
const char* rt_last_hip_error(const rt_ctx* ctx);
int rt_capi_version(void);

/* ---- scene -------------------------------------------------------------- */
/* Copies n primitives (in scene order: index j is the reference's scene.at(j)) to the
 * device.  Replaces any previous scene.  n == 0 is a valid (empty) scene.  Waits first
 * for every render this ctx has enqueued, on its own stream and on caller streams
 * (rt_render_device), so frames in flight finish on the old scene. */
int rt_set_scene(rt_ctx* ctx, const rt_prim* prims, int32_t n);

/* ---- lights ------------------------------------------------------------- */
/* The reference has one white point light at the origin (#define LIGHT_POS point3(0, 0, 0),
 * main.cpp:14).  rt_set_lights replaces it by 1..RT_MAX_LIGHTS coloured point lights; the
 * reference's own shading functions take the light as a parameter (diffuse_shading(pos,
 * normal, light_pos), specular(pos, normal, light_pos, view_dir)).
 *
 * n == 0 (lights may be NULL) restores the reference's light: every later call routes and
 * behaves exactly as on a ctx that never had lights (the plain and shadow kernels, the same
 * bytes).  1 <= n <= RT_MAX_LIGHTS: the records are copied and apply to every launch enqueued
 * afterwards; frames already enqueued keep theirs (no synchronisation).  Valid before
 * rt_set_scene; the lights survive rt_set_scene.  RT_ERR_INVALID_ARG, with the state
 * unchanged: n < 0 or n > RT_MAX_LIGHTS, NULL lights with n > 0, a non-finite position or
 * colour component.  Colours are not clamped.
 *
 * Shading with lights set, at every accepted hit of recursive_ray_tracing, at every level,
 * for frames and for ray-batch radiance, with pos, col.normal, mat and the ray direction d as
 * main.cpp:99-104 has them; lights l = 0..n-1 in order, P_l = position, C_l = color:
 *   diff_l = diffuse_shading(pos, col.normal, P_l)
 *   spec_l = pow(specular(pos, col.normal, P_l, -d), mat.specular_exponent)
 *   s_l    = diff_l * mat.diffuse + spec_l * mat.specular
 *   with RT_FLAG_SHADOWS: s_l = +0.0 if the segment sp .. P_l is occluded, where
 *            sp = pos + col.normal * .0001, direction P_l - sp (component-wise), T = 1,
 *            by rt_occluded's definition (the hit object takes part like any other)
 *   per channel c:  t = C_l[c] * s_l;   acc[c] = (l == 0) ? t : acc[c] + t
 *   local[c] = mat.color[c] * (acc[c] + mat.ambient)
 * All fp64, one IEEE operation per written operation, nothing fused.  Ray paths, the sky, the
 * metallic lerp and the segment counts are untouched; light rays are not counted.  pos == P_l
 * or sp == P_l exactly is unspecified.  One light {(0,0,0), (1,1,1)} gives the reference's
 * bits (1.0 * s is s), and with the flag the bits of RT_FLAG_SHADOWS without lights.
 *
 * RT_PREC_F64 follows the definition operation for operation; RT_PREC_PATH64 has the same
 * fp64 paths and the same fp64 shadow decisions with fp32 colour arithmetic; RT_PREC_MIXED is
 * served by the F64 kernels.  RT_ERR_UNSUPPORTED, before any launch, while lights are set:
 * RT_PREC_F32, RT_FLAG_SUN, rt_tile_row_costs.  As for shadowed frames, RT_OPT_PIXEL_PAIRS is
 * ignored, RT_OPT_FRAME_BATCH launches such frames one at a time and RT_OPT_ROW_FEEDBACK
 * neither samples nor reorders them; RT_OPT_SUPERSAMPLE, row bands,
 * rt_render_device_interleaved and rt_multi_* work.  rt_trace_rays* with out == NULL,
 * rt_occluded* and rt_frame_boxes ignore the lights. */
#define RT_MAX_LIGHTS 8
typedef struct rt_light {        /* 48 bytes */
    double position[3];
    double color[3];             /* linear RGB factor of the light's contribution, unclamped */
} rt_light;
int rt_set_lights(rt_ctx* ctx, const rt_light* lights, int32_t n);

/* ---- transmission -------------------------------------------------------- */
/* Material::metallic hands part of a surface's colour to the reflected ray; a transmission
 * record hands it to a ray that goes THROUGH the object instead: a wall is a thin pane, a
 * sphere a solid ball of glass.  One record per scene object, in rt_set_scene's order.
 *
 * n is the current scene's object count or 0.  n == 0 (recs may be NULL) clears the records,
 * and so does a set whose every `transmission` is exactly 0: every later call routes and
 * behaves exactly as on a ctx that never had records (the same kernels, the same bytes).
 * rt_set_scene clears them too: they belong to the objects.  A set applies to every launch
 * enqueued afterwards; launches already enqueued keep theirs (no synchronisation).
 * RT_ERR_NO_SCENE: n > 0 before a scene is set.  RT_ERR_INVALID_ARG, with the state unchanged:
 * n neither the scene's count nor 0, NULL recs with n > 0, a non-finite field, transmission
 * outside [0, 1], ior outside [1, 4].
 *
 * Shading, at every accepted hit of recursive_ray_tracing on an object whose tau =
 * transmission > 0, at every level, for frames and for ray-batch radiance; o, d, col and mat as
 * main.cpp:91-104 has them.  `local` is computed exactly as without records (lights and
 * RT_FLAG_SHADOWS included; transmissive objects block light rays like any other) and is
 * returned when remaining_iterations <= 0.  Otherwise the next ray (o', d') replaces
 * main.cpp:111-113's reflected ray and the result is, per channel,
 *   local + tau * (traced(o', d', remaining - 1) - local)
 * vec.cpp:45-49's lerp with tau in metallic's place; the object's metallic is not used there.
 * All fp64, one IEEE operation per written operation, nothing fused; dot(u, v) = u.x*v.x +
 * u.y*v.y + u.z*v.z summed left to right.
 *
 * Wall (a thin pane), pos = main.cpp:99's point, n = col.normal:
 *   f = dot(d, n);  nf = (f > 0) ? -n : n;  o' = pos - nf * .0001;  d' = d (the same bits)
 *
 * Sphere with centre c and ior.  P = o + d * projection is scene.cpp:75's intersection point
 * (rt_render_ao's P), not main.cpp:99's pos:
 *   n = P - c;  dl = sqrt(dot(d, d));  dh = d / dl;  nl = sqrt(dot(n, n));  nh = n / nl
 *   ci = -dot(dh, nh);  eta = 1.0 / ior;  k = 1.0 - (eta * eta) * (1.0 - ci * ci)
 *   t = dh * eta + nh * (eta * ci - sqrt(k))                              (refracted in)
 *   m = c - P;  s = (2.0 * dot(t, m)) / dot(t, t);  Q = P + t * s         (the chord)
 *   n2 = Q - c;  l2 = sqrt(dot(n2, n2));  n2h = n2 / l2;  tl = sqrt(dot(t, t));  th = t / tl
 *   c2 = dot(th, n2h);  k2 = 1.0 - (ior * ior) * (1.0 - c2 * c2);  k2c = (k2 > 0) ? k2 : 0.0
 *   d' = th * ior + n2h * (sqrt(k2c) - ior * c2);  o' = Q + n2 * .0001    (refracted out)
 * ior >= 1, so entry never reflects totally; k2 == ci^2 in exact arithmetic, so the clamp only
 * meets rounding.  Whatever lies inside the sphere is ignored along the chord, which is not a
 * closest-hit query: segment counts stay one per accepted query.  A tangent hit (det == 0) is
 * unspecified.
 *
 * RT_PREC_F64 follows the text operation for operation; RT_PREC_PATH64 has the same fp64 path,
 * (o', d') included, with fp32 colour; RT_PREC_MIXED is served by the F64 kernels.
 * RT_ERR_UNSUPPORTED, before any launch, while records are set: RT_PREC_F32, RT_FLAG_SUN,
 * rt_tile_row_costs.  As for lit frames, RT_OPT_PIXEL_PAIRS is ignored, RT_OPT_FRAME_BATCH
 * launches one frame at a time and RT_OPT_ROW_FEEDBACK neither samples nor reorders;
 * RT_OPT_MIRROR_BINS is not applied (a ray that passed through a pane did not reflect off it).
 * RT_OPT_SUPERSAMPLE, row bands, rt_render_device_interleaved, rt_render_device_frames,
 * rt_multi_*, rt_set_lights and RT_FLAG_SHADOWS work.  rt_trace_rays* with out == NULL,
 * rt_occluded*, rt_render_aov*, rt_render_ao* and rt_frame_boxes ignore the records. */
typedef struct rt_transmission {   /* 16 bytes, one per scene object, rt_set_scene order */
    double transmission;           /* tau in [0, 1]; 0 = opaque: the reference's reflection step */
    double ior;                    /* index of refraction, finite, in [1, 4]; read for spheres only */
} rt_transmission;
int rt_set_transmission(rt_ctx* ctx, const rt_transmission* recs, int32_t n);

/* ---- tuning ------------------------------------------------------------- */
enum rt_option {
    RT_OPT_WAVE_CULL_MIN_SPHERES = 1, /* scenes with at least this many spheres use the
                                         wave-cooperative cull (default 24; 0 = always,
                                         INT32_MAX = never).  Output is identical. */
    RT_OPT_STATS_DEVICE_PTR = 2,      /* diagnostics: device address of 3 uint64 counters
                                         that renders add to ([0] wave culls, [1] spheres
                                         kept, [2] spheres considered); 0 = off */
    RT_OPT_EYE_TABLES = 3,            /* 1 (default): primary rays use per-frame tables of
                                         their camera-origin terms (small scenes); 0 = off.
                                         Output is identical. */
    RT_OPT_TILE_BINS = 4,             /* 1 (default): per-frame pixel boxes of every
                                         primitive let each 8x8 tile test only what its
                                         primary rays can hit (scenes of <= 64
                                         primitives); 0 = off.
                                         Output is identical. */
    RT_OPT_ROW_ORDER = 5,             /* 1 (default): tile rows are dispatched centre-out
                                         from the estimated heaviest row (scheduling only);
                                         0 = top to bottom.  Output is identical. */
    RT_OPT_MIRROR_BINS = 6,           /* 1 (default): bounces that follow the same wall
                                         chain across a wave use the boxes of the mirrored
                                         camera (needs RT_OPT_TILE_BINS); 0 = off.  Output
                                         is identical. */
    RT_OPT_BOX_CACHE = 7,             /* 1 (default): a render whose scene, camera, band and
                                         options equal the previous render's reuses its
                                         per-frame pixel boxes (host work only); 0 = always
                                         recompute.  Output is identical. */
    RT_OPT_ROW_FEEDBACK = 8,          /* N > 0 (default 32): every render records each
                                         tile's cost; every N frames (and at once for a new
                                         band or scene) a snapshot is copied back behind the
                                         kernel, and later renders of the same band dispatch
                                         tile rows heaviest-first by it, or in
                                         RT_OPT_ROW_MIX's order (scheduling only); 0 = off.  Setting it (any value) drops the order
                                         and any snapshot still in flight.  Output is
                                         identical. */
    RT_OPT_PIXEL_PAIRS = 9,           /* 1: RT_PREC_PATH64 renders without the wave cull
                                         trace two pixels per lane (16x8 pixels per
                                         wave); 0 (default) = one.  Output is identical. */
    RT_OPT_ROW_FEEDBACK_WARM = 10,    /* K >= 0 (default 0): after a new band or scene,
                                         RT_OPT_ROW_FEEDBACK takes K more snapshots back to
                                         back (each once the previous one has landed)
                                         before its interval applies.  Output is
                                         identical. */
    RT_OPT_WALL_ORDER = 11,           /* 1: the primary scan visits the walls nearest to
                                         the camera first (per frame), so a wall behind the
                                         best hit skips its bounds test; 0 (default) = scene
                                         order (measured: c2 +1% with the order).  Output is
                                         identical (wall ties compare scene indices). */
    RT_OPT_ROW_FEEDBACK_EMA = 14,     /* W in [0, 95] (default 0): the measured row order
                                         ranks tile rows by their cost smoothed over the
                                         band's snapshots, acc = W% acc + (100-W)% new;
                                         0 = the latest snapshot alone.  Output is
                                         identical. */
    RT_OPT_ROW_FEEDBACK_ISOLATE = 15, /* 1: a frame whose tile costs RT_OPT_ROW_FEEDBACK
                                         samples runs alone on the GPU (its stream waits for
                                         this ctx's frames on other streams, and their next
                                         frames wait for it), so the costs are not those of
                                         overlapping frames; 0 (default) = it overlaps like
                                         any frame (measured: the lost overlap costs more
                                         than cleaner costs gain).  Output is identical. */
    RT_OPT_ROW_MIX = 23,              /* How RT_OPT_ROW_FEEDBACK's measured order arranges
                                         the dispatch units.  0 = strictly heaviest first
                                         (by a unit's most expensive wave).  1 (default) =
                                         for the frames of an rt_render_device_frames call
                                         spread over two or more streams, the light units
                                         (work, the sum of a unit's wave costs, not above
                                         the mean) are merged between the heavy ones,
                                         lightest first and in proportion to the work
                                         dispatched, and the very lightest are held back
                                         for the end: heavy (VALU-bound) and light
                                         (issue-bound) waves share the SIMDs for the whole
                                         frame, and the next frame in flight fills the
                                         tail; frames rendered one at a time keep 0's order
                                         (measured at c2: the mixed order alone on the GPU
                                         is +15%, its tail exposed).  2 = the mixed order for
                                         every frame (diagnostic).  rt_order_units gives
                                         both orders on the host.  Output is identical. */
    RT_OPT_HOST_PIPELINE = 16,       /* 1 (default): rt_render_device_frames computes the
                                         next frames' kernel arguments (pixel boxes, mirror
                                         chains, eye tables) on a helper thread while the
                                         calling thread launches the current frame; 0 = one
                                         thread does both in turn.  The same launches in the
                                         same order: output is identical. */
    RT_OPT_FRAME_BATCH = 21,         /* B in [1, RT_MULTI_BATCH_MAX] (default 1): in
                                         rt_render_device_frames with the host pipeline,
                                         up to B consecutive frames on the same stream that
                                         write distinct buffers go to the GPU as ONE launch
                                         (frame = blockIdx.z; each frame's kernel arguments
                                         in a device table copied in front of the launch),
                                         so the host pays one launch per group instead of
                                         one per frame.  Frames sampled by
                                         RT_OPT_ROW_FEEDBACK, a change of the row order's
                                         grid, wave-cull scenes and RT_OPT_PIXEL_PAIRS launch
                                         one frame at a time.  On rt_multi_set_option: also
                                         a rank renders each RT_OPT_MULTI_BATCH batch's band
                                         frames (and the root its rows) in blocks of B
                                         consecutive frames per stream, over ceil(batch / B)
                                         streams, so each block is one launch.  Output is
                                         identical. */
    RT_OPT_MULTI_FRAMES = 17,        /* rt_multi_set_option only: F in [1, RT_MULTI_SLOTS]
                                         (default 2) band slots per rank — frames of a rank in
                                         flight on F render streams, so a small band's longest
                                         waves (a 1/8 band of config 4: tiles bouncing between
                                         facing walls) overlap F - 1 other frames.  Every
                                         handle of one exchange must use the same F.  The
                                         gathered frames are identical. */
    RT_OPT_MULTI_FAULT = 18,         /* rt_multi_set_option only, a test hook: 1 = the next
                                         frame (or batch) of this handle fails right after
                                         its part of the exchange was queued — the root's
                                         receives, a sender's send (the failure path of a
                                         real exchange on a one-GPU machine). */
    RT_OPT_MULTI_BATCH = 19,         /* rt_multi_set_option only: B in [1,
                                         RT_MULTI_BATCH_MAX] (default 1) frames per gather in
                                         rt_multi_render_device_frames, one process per rank
                                         (nlocal == 1) with contiguous or weighted bands: each
                                         rank renders B frames' bands back to back and sends
                                         them in ONE ncclSend; the root receives every rank's
                                         B bands in one group and scatters them into the B
                                         frames with one kernel.  The per-frame host work of
                                         the exchange (events, RCCL calls: ~20 us per frame,
                                         more than a 1/8 band's kernel) is paid once per B
                                         frames; a frame's rows reach the root when its batch
                                         completes, and a non-root rank's caller stream
                                         follows its batch's send.  A call batches when
                                         B > 1, nframes >= 2 and every camera has the same
                                         size (so every rank decides alike; every handle of
                                         one exchange must use the same B); the root then
                                         needs a DISTINCT frame buffer for each frame of a
                                         batch (min(B, nframes) of them: frames of one batch
                                         sharing a buffer could never be whole in it) and at
                                         most RT_MULTI_SLOTS distinct caller streams, else
                                         the call is refused before anything is enqueued
                                         (RT_ERR_UNSUPPORTED; with ranks in other processes
                                         the exchange is then broken, as the peers' sends of
                                         that call have no receives).  A buffer of an earlier
                                         batch is rendered into again only after that
                                         batch's gather into it completed, so every frame is
                                         whole in its buffer from its batch's end until the
                                         next frame written there (2 B buffers keep
                                         consecutive batches overlapped).  The frames are
                                         identical. */
    RT_OPT_MULTI_TIMEOUT_MS = 20,    /* rt_multi_set_option only: T >= 0 (default 120000)
                                         ms that rt_multi_sync waits for this process's
                                         streams; it polls them (and RCCL's asynchronous
                                         error) and, when T passes or RCCL reports an error,
                                         breaks the exchange, aborts the communicators
                                         (ncclCommAbort) and returns RT_ERR_COMM instead of
                                         blocking forever on a peer that failed.  0 = no
                                         deadline. */
    RT_OPT_MULTI_LAYOUT = 13,        /* rt_multi_set_option only: 0 (default) = contiguous
                                         row bands (rt_band_rows); 1 = interleaved tile rows
                                         (rt_interleaved_rows): balanced when the frame's cost
                                         is concentrated in some rows (config 5); 2 =
                                         contiguous bands cut at tile rows so that each
                                         carries an equal share of the per-tile-row weights
                                         given to rt_multi_set_row_weights
                                         (rt_weighted_band_rows; equal bands while no weights
                                         cover the frame's tile rows).  The gathered frame is
                                         identical. */
    RT_OPT_SUPERSAMPLE = 22,         /* S in {1, 2, 4, 8} (default 1; anything else is
                                         RT_ERR_INVALID_ARG): rt_render, rt_render_device and
                                         rt_render_device_frames trace S x S rays per pixel
                                         and store their mean.  UNLIKE EVERY OTHER OPTION
                                         THIS ONE CHANGES THE OUTPUT.  cam, row0, nrows, the
                                         buffer and its format keep their meaning in output
                                         pixels: pixel (i, j) is the mean of pixels
                                         [i*S + b][j*S + a], a, b in [0, S), of the frame the
                                         same call renders for rt_supersample_camera(cam, S)
                                         (same depth, precision, flags).  Summation: each
                                         sample's colour widened to fp64, a balanced pairwise
                                         tree over the S columns (v = v[:, 0::2] + v[:, 1::2],
                                         log2 S times), then the same over the S rows, times
                                         1.0 / (S*S), then the format's conversion (the cast,
                                         or the RGBA8 quantisation of the mean: tone mapping
                                         after averaging).  The mean is formed inside the
                                         trace kernel; only width x height pixels are written.
                                         d_segments and stats->segments count every sample's
                                         segments.  RT_PREC_MIXED frames are rendered by the
                                         RT_PREC_F64 kernels (its contract is output == F64).
                                         RT_OPT_PIXEL_PAIRS is ignored and RT_OPT_ROW_FEEDBACK
                                         neither samples nor reorders such frames (centre-out
                                         order, or an rt_set_row_order over the tile rows of
                                         the S-times larger frame); RT_OPT_FRAME_BATCH
                                         launches them one at a time.  Not covered:
                                         rt_render_device_interleaved with nparts > 1 returns
                                         RT_ERR_UNSUPPORTED while S > 1, and
                                         rt_multi_set_option refuses S != 1 with
                                         RT_ERR_UNSUPPORTED.  rt_trace_rays*, rt_occluded*,
                                         rt_tile_row_costs and rt_frame_boxes ignore it. */
    RT_OPT_CLUSTER_COS = 12          /* C in [-2000, 2000] (default 400): in scenes that use
                                         the wave cull, a wave (any precision) whose live
                                         rays' cone has cos(half-angle) < C/1000 tests each
                                         lane's own ray against sphere clusters (boxes of
                                         <= 8 spheres) and runs the exact test on its own
                                         clusters only; -2000 = never (measured: c5 PATH64
                                         -36%, F64 -44%, c3 -4..15% at 300-500).  Output is
                                         identical. */
};
int rt_set_option(rt_ctx* ctx, int32_t option, int64_t value);

/* Explicit dispatch order of the tile rows (8 pixel rows each): perm is a permutation of
 * 0..n-1, used by every render whose band has exactly n tile rows, ahead of
 * RT_OPT_ROW_FEEDBACK; n = 0 clears it.  Scheduling only: output is identical.
 * RT_ERR_INVALID_ARG if perm is not a permutation or n > 2048. */
int rt_set_row_order(rt_ctx* ctx, const int16_t* perm, int32_t n);

/* ---- frame operators (replace rt_scene, main.cpp:124-139) --------------- */
/* Render rows [row0, row0+nrows) of the frame into caller-owned HOST memory `out`
 * (nrows*width pixels of `out_format`), synchronously.  depth = remaining_iterations
 * of recursive_ray_tracing (rt_scene passes the default 10, main.cpp:89/136).
 * stats may be NULL; stats->segments is filled only when count_segments != 0. */
int rt_render(rt_ctx* ctx, const rt_camera* cam, int32_t row0, int32_t nrows, int32_t depth,
              int32_t precision, uint32_t flags, int32_t out_format, void* out,
              int32_t count_segments, rt_stats* stats);

/* Same, but `d_out` is DEVICE memory and the launch is enqueued on `stream`
 * (a hipStream_t; NULL = the ctx's stream) without synchronising: the hot path as a
 * bench or a multi-GPU tiler drives it.  If d_segments != NULL it must point to one
 * device uint64 that receives += the segment count.  The launch signals a per-stream
 * event of the ctx that rt_set_scene / rt_ctx_destroy wait on (up to 16 streams are
 * tracked; a 17th retires the oldest by waiting on it).  Every entry point runs on the
 * ctx's device and leaves the caller's current device unchanged. */
int rt_render_device(rt_ctx* ctx, const rt_camera* cam, int32_t row0, int32_t nrows,
                     int32_t depth, int32_t precision, uint32_t flags, int32_t out_format,
                     void* d_out, uint64_t* d_segments, void* stream);

/* A batch of frames of the frame loop (main.cpp:250-375 renders one frame per iteration),
 * enqueued by one call: frame f (0 <= f < nframes) renders cams[f % ncams] into
 * d_outs[f % nouts] on streams[f % nstreams] (NULL entries = the ctx's stream), exactly
 * as nframes rt_render_device calls in that order would — each frame's own host work
 * (pixel boxes, row order) and launch — without the caller's per-call overhead.  No
 * synchronisation; stops at the first failing frame and returns its status. */
int rt_render_device_frames(rt_ctx* ctx, const rt_camera* cams, int32_t ncams, int32_t row0,
                            int32_t nrows, int32_t depth, int32_t precision, uint32_t flags,
                            int32_t out_format, void* const* d_outs, int32_t nouts,
                            void* const* streams, int32_t nstreams, int32_t nframes);

/* ---- ray queries (find_closest_hit, recursive_ray_tracing for caller rays) ---------- */
/* The reference's find_closest_hit(scene, ray) (main.cpp:67-84) and recursive_ray_tracing(
 * scene, ray, remaining) (main.cpp:89-119) take any ray, not only a camera's pixel rays:
 * picking, line-of-sight and collision probes, light probes, a host's own camera models.
 * These entry points run them on the device for a batch of n rays, one GPU lane per ray.
 *
 * rt_hit is the Collision find_closest_hit returns, as plain data.  A miss is main.cpp:70's
 * placeholder {DBL_MAX, {0,0,0}, -1, 0}, so whole record arrays compare bytewise. */
typedef struct rt_hit {          /* 40 bytes */
    double  distance;   /* the value find_closest_hit compares: world distance for a sphere,
                           parametric t for a wall (the reference's quirk, kept) */
    double  normal[3];  /* as Collision carries it: unnormalised point - centre for a sphere,
                           the stored normal for a wall */
    int32_t index;      /* SCENE index (rt_set_scene order), -1 = miss */
    int32_t reserved;   /* 0 */
} rt_hit;

/* origins, directions: n x 3 doubles, row-major; directions are NOT normalised (as in the
 * reference, where |d| scales a wall's parametric t).  out: n pixels of out_format, ray k's
 * radiance recursive_ray_tracing(scene, ray k, depth) at pixel k; hits: n records, the
 * closest hit of each ray's FIRST segment.  Either may be NULL (both: RT_ERR_INVALID_ARG).
 * With out == NULL the call is the pure find_closest_hit query: one segment per ray, no
 * shading, no bounce (depth and flags unused; the segment count is n).
 * Precisions: RT_PREC_F64 op for op; RT_PREC_PATH64 exact paths with fp32 colour (hit records
 * are the same bits in both); RT_PREC_MIXED is served by the F64 kernels (its contract is
 * "output == F64"); RT_PREC_F32 returns RT_ERR_UNSUPPORTED.  RT_FLAG_SUN as for frames.
 * n == 0: RT_OK, nothing launched; n < 0 or n > INT32_MAX: RT_ERR_INVALID_ARG; depth outside
 * 0..rt_max_depth(): RT_ERR_UNSUPPORTED as for frames; RT_ERR_NO_SCENE before rt_set_scene.
 * Scenes of RT_OPT_WAVE_CULL_MIN_SPHERES spheres or more cull per wave: by the cone of the
 * wave's 64 rays when they are coherent, else by each lane's own walk over the sphere
 * clusters (RT_OPT_CLUSTER_COS), so neighbouring rays of a batch should be neighbours in
 * space where the caller can arrange it.  The frame-only options (tile bins, eye tables,
 * mirror bins, row order, row feedback, frame batching) do not apply, and a ray call leaves
 * their cached state as it was.
 *
 * rt_trace_rays: host memory in and out, synchronous (staging buffers in the ctx; stats as
 * rt_render: ms = device time of the kernel, segments only when count_segments != 0). */
int rt_trace_rays(rt_ctx* ctx, const double* origins, const double* directions, int64_t n,
                  int32_t depth, int32_t precision, uint32_t flags, int32_t out_format,
                  void* out, rt_hit* hits, int32_t count_segments, rt_stats* stats);
/* The same with every buffer in DEVICE memory, enqueued on `stream` (NULL = the ctx's) without
 * synchronising; *d_segments (may be NULL) receives += the segment count.  Like
 * rt_render_device the launch signals the ctx's per-stream event that rt_set_scene and
 * rt_ctx_destroy wait on. */
int rt_trace_rays_device(rt_ctx* ctx, const double* d_origins, const double* d_directions, int64_t n,
                         int32_t depth, int32_t precision, uint32_t flags, int32_t out_format,
                         void* d_out, rt_hit* d_hits, uint64_t* d_segments, void* stream);

/* ---- occlusion queries (any hit on a segment) ---------------------------------------- */
/* Is anything on the segment from o to o + d * tmax?  The visibility / line-of-sight probe:
 * it stops at the first blocker, discards everything beyond tmax and returns one byte per ray.
 * (An rt_hit cannot answer it for |d| != 1: find_closest_hit ranks a sphere's world distance
 * against a wall's parametric t — the reference's quirk, kept there — so its record need not
 * be the first thing along the ray.)
 *
 * For ray k (origin o, direction d — NOT normalised; finite and non-zero as for rt_trace_rays —
 * and limit T = tmax[k]), occluded[k] = 1 iff some scene object j has, with the reference's
 * c = scene[j]->intersect(ray(d, o)),
 *   1. c.distance > 0 — find_closest_hit's own acceptance test (main.cpp:77), so a ray that
 *      starts inside a sphere is not blocked by that sphere, as in the reference; and
 *   2. param(c) <= T, where param is the hit's PARAMETER along the ray: a wall's c.distance
 *      (its t, scene.cpp:10); a sphere's `projection`, the value scene.cpp:77 multiplies by
 *      |d| to form c.distance.
 * Otherwise 0.  The comparison is the fp64 <= on those exact values (there is no precision
 * argument: the answer is exact); a NaN T and T <= 0 are never occluded; tmax == NULL means
 * +inf for every ray; an empty scene gives all zeros.  Hence, with tmax == NULL,
 * occluded[k] == (hits[k].index >= 0) for rt_trace_rays' record of the same ray, and with T
 * equal to the smallest param over the blockers the ray is occluded while the next double
 * towards 0 is not.  Between two points a and b: d = b - a, tmax = 1 (slightly less when b
 * itself lies on a surface).
 *
 * out: n bytes (1 = occluded, 0 = free); count: the number of occluded rays.  Either may be
 * NULL, not both (RT_ERR_INVALID_ARG).  n == 0: RT_OK, nothing launched, outputs untouched;
 * n < 0 or n > INT32_MAX: RT_ERR_INVALID_ARG; RT_ERR_NO_SCENE before rt_set_scene.
 * RT_OPT_WAVE_CULL_MIN_SPHERES and RT_OPT_CLUSTER_COS apply as for ray batches; the frame-only
 * options (RT_OPT_SUPERSAMPLE included) are ignored and their cached state is left as it was.
 *
 * rt_occluded: host memory in and out, synchronous (staging buffers in the ctx); stats->ms =
 * device time of the kernel, stats->segments = n. */
int rt_occluded(rt_ctx* ctx, const double* origins, const double* directions, const double* tmax,
                int64_t n, uint8_t* out, uint64_t* count, rt_stats* stats);
/* The same with every buffer in DEVICE memory, enqueued on `stream` (NULL = the ctx's) without
 * synchronising; *d_count += the occluded rays.  The launch signals the ctx's per-stream event
 * that rt_set_scene and rt_ctx_destroy wait on. */
int rt_occluded_device(rt_ctx* ctx, const double* d_origins, const double* d_directions,
                       const double* d_tmax, int64_t n, uint8_t* d_out, uint64_t* d_count,
                       void* stream);

/* ---- frame AOVs (the G-buffer of a frame's primary hits) ------------------------------ */
/* What a frame's PRIMARY rays hit, as per-pixel layers: the hit record, object index, depth,
 * surface normal and base colour that picking, outlines, compositing, depth cues and denoisers
 * want next to the colour.  Only the primary segment runs: no shading, no bounce, no lights.
 *
 * Pixel (row i, column j) of rows [row0, row0 + nrows) traces the ray of main.cpp:132-134:
 * origin o = cam.position, direction d = cam.position - ((image_top_left + pixel_delta_x * j)
 * + pixel_delta_y * i), NOT normalised.  With c = find_closest_hit(scene, ray(d, o))
 * (main.cpp:67-84) the layers are defined in fp64, one IEEE operation per written operation,
 * nothing fused; a float layer is that fp64 value converted with one round-to-nearest cast:
 *   hit     c as an rt_hit: the bytes rt_trace_rays(out = NULL) gives for that ray; a miss is
 *           {DBL_MAX, {0,0,0}, -1, 0}
 *   index   c.hit_object_index (rt_set_scene order), -1 = miss
 *   depth   the WORLD distance from the camera to the hit: c.distance for a sphere (already
 *           projection * |d|), c.distance * d.length() for a wall (vec.cpp:3-9:
 *           sqrt(x*x + y*y + z*z), summed left to right), +inf for a miss.  Unlike
 *           rt_hit.distance (world distance for spheres, parametric t for walls: the
 *           reference's quirk) one buffer is comparable across kinds.
 *   normal  c.normal.normalize() (vec.cpp:21-24: each component divided by sqrt(n.n)); a
 *           wall's is its stored normal divided by its own length again; (0,0,0) for a miss
 *   albedo  mat.color of the hit object; (0,0,0) for a miss
 * There is no precision argument, no flags and no depth: the answer is exact.  Buffers are
 * band-relative, row-major, nrows * width pixels, as for rt_render; a NULL layer is not written
 * and costs no stores; nothing outside the buffers is written.
 *
 * RT_ERR_INVALID_ARG for a NULL ctx, cam or buffers struct, for all five layers NULL or a
 * non-NULL `reserved`; RT_ERR_NO_SCENE before rt_set_scene; the band checks and their statuses
 * are rt_render's for the same cam, row0 and nrows.  All before any launch.  An empty scene is
 * valid: all misses.
 * Ignored: rt_set_lights, RT_OPT_SUPERSAMPLE (for the samples' AOVs pass
 * rt_supersample_camera's camera), RT_OPT_PIXEL_PAIRS, RT_OPT_FRAME_BATCH.  RT_OPT_TILE_BINS,
 * RT_OPT_EYE_TABLES, RT_OPT_WALL_ORDER, RT_OPT_WAVE_CULL_MIN_SPHERES and RT_OPT_CLUSTER_COS
 * serve the scan; the output is identical for every setting of them.  RT_OPT_ROW_FEEDBACK
 * neither samples nor reorders an AOV launch, and an AOV call leaves the feedback state, any
 * measured order and the box cache as they were: a following rt_render* gives the bytes and
 * launches it would have given without it. */
typedef struct rt_aov_buffers {  /* 48 bytes; a NULL layer is not written */
    rt_hit*  hit;      /* nrows*width records           (40 B/px) */
    int32_t* index;    /* nrows*width                   ( 4 B/px) */
    float*   depth;    /* nrows*width                   ( 4 B/px) */
    float*   normal;   /* nrows*width*3, row-major xyz  (12 B/px) */
    float*   albedo;   /* nrows*width*3                 (12 B/px) */
    void*    reserved; /* must be NULL */
} rt_aov_buffers;

/* rt_render_aov: the layers in HOST memory, synchronous (staging buffers in the ctx, like
 * rt_trace_rays); stats->ms = device time of the kernel, stats->segments = nrows * width. */
int rt_render_aov(rt_ctx* ctx, const rt_camera* cam, int32_t row0, int32_t nrows,
                  const rt_aov_buffers* out, rt_stats* stats);
/* The same with the layers in DEVICE memory (the struct itself on the host), enqueued on
 * `stream` (NULL = the ctx's) without synchronising.  Like rt_render_device the launch signals
 * the ctx's per-stream event that rt_set_scene and rt_ctx_destroy wait on. */
int rt_render_aov_device(rt_ctx* ctx, const rt_camera* cam, int32_t row0, int32_t nrows,
                         const rt_aov_buffers* d_out, void* stream);

/* ---- ambient occlusion (hemisphere probes at a frame's primary hits) ------------------- */
/* The reference's ambient term is a constant (mat.ambient), so creases, contacts and corners are
 * flat.  Ambient occlusion probes the hemisphere above each pixel's primary hit with short
 * any-hit segments and reports how many are blocked: a geometry layer for compositing and
 * denoisers, next to rt_render_aov's depth, normal and albedo.  One launch: the primary segment
 * of rt_render_aov, then the probes of rt_occluded, no ray buffer in between.
 *
 * Everything is fp64, one IEEE operation per written operation, nothing fused, dot products
 * x*x' + y*y' + z*z' summed left to right.  Pixel (row i, column j) has the primary ray (o, d)
 * of main.cpp:132-134 and c = find_closest_hit(scene, ray(d, o)): rt_render_aov's record.
 *   miss      count = 0.
 *   P         the TRUE point the pixel sees: o + d * c.distance for a wall; o + d * projection
 *             for a sphere (scene.cpp:75's intersection_point, the value c.normal + centre came
 *             from).  Deliberately not main.cpp:99's pos, which for |d| != 1 uses a sphere's
 *             world distance as a parameter and lands off the surface: the beauty frame keeps
 *             that quirk, a geometry layer must not (as the depth AOV is not rt_hit.distance).
 *             A tangent hit (det == 0 exactly) is unspecified.
 *   nf        the facing normal: n = c.normal, un-normalised as the record carries it;
 *             f = dot(d, n); nf = (f > 0) ? -n : n — a wall seen from behind is probed on the
 *             viewer's side.
 *   sp        the probes' origin, P + nf * .0001 (the reference's own offset, main.cpp:111).
 *   probe k   (0 <= k < ndirs) w_k = the caller's direction k; s = dot(w_k, nf);
 *             w = (s < 0) ? -w_k : w_k (s == 0 is not flipped).  The probe is occluded iff the
 *             segment sp .. sp + w * radius is occluded by rt_occluded's definition
 *             (c.distance > 0, parameter <= T = radius); the hit object takes part like any other.
 *   count     the number of occluded probes, 0..ndirs.
 *   ao        (float)((double)(ndirs - count) / (double)ndirs): the open fraction, 1.0f for a
 *             miss and where nothing is near.
 * Directions are NOT normalised: |w_k| scales what radius means, as |d| does for rt_occluded's
 * tmax; with unit directions the radius is a world distance.  There is no precision argument,
 * no flags and no depth: the answer is exact.  Buffers are band-relative, row-major, nrows *
 * width pixels, as for rt_render; a NULL layer is not written; nothing outside them is written.
 *
 * RT_ERR_INVALID_ARG for a NULL ctx, cam, params or buffers struct; both layers NULL; a non-NULL
 * or non-zero reserved field; dirs == NULL; ndirs outside 1..RT_AO_MAX_DIRS; a direction with a
 * non-finite component or all three zero; radius NaN or <= 0 (+inf is allowed).
 * RT_ERR_NO_SCENE before rt_set_scene; the band checks and their statuses are rt_render's for the
 * same cam, row0 and nrows.  All before any launch, the buffers untouched.  nrows == 0 is RT_OK:
 * nothing is launched and stats = {0, 0}.  An empty scene is valid: all misses.
 * Ignored, and left alone, exactly as by rt_render_aov: rt_set_lights, RT_OPT_SUPERSAMPLE,
 * RT_OPT_PIXEL_PAIRS, RT_OPT_FRAME_BATCH are ignored; RT_OPT_TILE_BINS, RT_OPT_EYE_TABLES,
 * RT_OPT_WALL_ORDER, RT_OPT_WAVE_CULL_MIN_SPHERES and RT_OPT_CLUSTER_COS serve the scans with
 * identical output; RT_OPT_ROW_FEEDBACK neither samples nor reorders the launch, and the call
 * leaves the feedback state, any measured order and the box cache as they were. */
#define RT_AO_MAX_DIRS 64
typedef struct rt_ao_params {      /* 32 bytes */
    const double* dirs;            /* ndirs x 3 doubles, row-major, HOST memory in BOTH entry points */
    int32_t ndirs;                 /* 1..RT_AO_MAX_DIRS */
    int32_t reserved;              /* must be 0 */
    double  radius;                /* the limit T of every probe (a PARAMETER along the probe's
                                      direction, as rt_occluded's tmax): > 0, +inf allowed */
    void*   reserved2;             /* must be NULL */
} rt_ao_params;
typedef struct rt_ao_buffers {     /* 24 bytes; a NULL layer is not written */
    uint8_t* count;                /* nrows*width: occluded probes of the pixel, 0..ndirs */
    float*   ao;                   /* nrows*width: open fraction, 1 = nothing near */
    void*    reserved;             /* must be NULL */
} rt_ao_buffers;

/* rt_render_ao: the layers in HOST memory, synchronous (staging buffers in the ctx, like
 * rt_render_aov); stats->ms = device time of the kernel, stats->segments = nrows * width (probes
 * are not counted, as shadow rays are not). */
int rt_render_ao(rt_ctx* ctx, const rt_camera* cam, int32_t row0, int32_t nrows,
                 const rt_ao_params* params, const rt_ao_buffers* out, rt_stats* stats);
/* The same with the layers in DEVICE memory, enqueued on `stream` (NULL = the ctx's) without
 * synchronising.  Both structs and dirs are HOST memory and are consumed before the call
 * returns (the directions travel in the kernel's arguments): the caller may overwrite or free
 * them at once, and a later call with other directions does not change a launch already
 * enqueued.  Like rt_render_device the launch signals the ctx's per-stream event that
 * rt_set_scene and rt_ctx_destroy wait on. */
int rt_render_ao_device(rt_ctx* ctx, const rt_camera* cam, int32_t row0, int32_t nrows,
                        const rt_ao_params* params, const rt_ao_buffers* d_out, void* stream);
/* A default direction set (host only, no ctx): for 1 <= n <= RT_AO_MAX_DIRS, n unit vectors of a
 * spherical Fibonacci set over the WHOLE sphere — z_k = 1 - (2k+1)/n, r = sqrt(1 - z*z),
 * phi = k * pi * (3 - sqrt(5)), vector (r cos phi, r sin phi, z) — which the flip folds onto each
 * pixel's hemisphere.  out: n x 3 doubles.  RT_ERR_INVALID_ARG otherwise.  Its bits depend on the
 * platform's libm. */
int rt_ao_directions(int32_t n, double* out);

/* ---- multi-GPU frame operator (BASELINE config 4) ----------------------- */
/* ONE frame split into contiguous row bands (rt_band_rows) over nranks ranks, one GPU each,
 * every band rendered by that rank's own rt_ctx, then gathered into the frame buffer of
 * rank 0 (the root) — the reference renders the frame on one CPU thread (main.cpp:124-139,
 * called at main.cpp:329); pixels are independent, so the gathered frame is bitwise the
 * one-GPU frame.  Two process models, one object:
 *   - one process drives every GPU: nlocal == nranks, first_rank 0, unique_id NULL
 *     (the communicator is made as ncclCommInitAll would; one host worker thread per extra
 *     device does that rank's per-frame host work and launches in parallel);
 *   - one process per GPU (torchrun-style): nlocal == 1, first_rank = this process's rank,
 *     unique_id = the RT_MULTI_ID_BYTES bytes rt_multi_unique_id returned on ONE process
 *     and shared with the others (ncclCommInitRank; blocks until every rank has joined).
 * Transports: RT_TRANSPORT_RCCL gathers with ncclSend/ncclRecv (rccl.h) over xGMI —
 * bands may differ in height by one row, so no padding; RT_TRANSPORT_COPY (one process
 * only) copies each band into the root's frame with hipMemcpyPeerAsync and also accepts
 * the same device more than once (several ranks on one GPU: the orchestration without
 * RCCL, e.g. on a one-GPU machine); RT_TRANSPORT_RCCL_LOOPBACK is RT_TRANSPORT_RCCL with
 * the root's own band also sent through RCCL (a self ncclSend/ncclRecv pair in the same
 * group as the other bands' receives) and a communicator even at one rank — so every RCCL
 * call of the gather (ncclCommInitRank, the group, send/recv, ncclCommGetAsyncError)
 * executes on a one-GPU machine; it costs one extra copy of the root's band.
 * Frames in flight: each non-root rank renders into one of RT_OPT_MULTI_FRAMES (<=
 * RT_MULTI_SLOTS) band buffers, each with its own render stream, while earlier frames' bands
 * are still being rendered or sent on its comm stream;
 * a band buffer is reused only after its send has completed (device-side event waits; the
 * host never blocks in rt_multi_render_device*).
 * Failures: argument checks every rank makes alike return their status and leave the
 * rt_multi usable.  A frame that fails after them leaves the exchange out of step when any
 * rank may have queued its part (a receive or a send): always with ranks in other processes
 * (they queue theirs whatever this process did), and with every rank in this process once
 * a local rank queued its part.  The rt_multi is then broken — every later frame returns
 * RT_ERR_COMM, rt_multi_sync aborts the communicator (ncclCommAbort) instead of waiting on
 * receives that cannot complete, and rt_multi_destroy aborts instead of destroying.  With
 * one process per GPU over RCCL the other processes are not told: their rt_multi_sync
 * polls their streams and RCCL's asynchronous error and gives up at its deadline
 * (RT_OPT_MULTI_TIMEOUT_MS: broken, communicator aborted, RT_ERR_COMM).  The mailbox
 * transports (THREADS, IPC) tell every peer at once: their waits return RT_ERR_COMM. */
#define RT_MULTI_ID_BYTES 128
#define RT_MULTI_SLOTS 4   /* band slots per rank (RT_OPT_MULTI_FRAMES uses 1..4, default 2) */
#define RT_MULTI_BATCH_MAX 16  /* frames per gather (RT_OPT_MULTI_BATCH) */
enum rt_transport {
    RT_TRANSPORT_RCCL = 0,
    RT_TRANSPORT_COPY = 1,
    RT_TRANSPORT_RCCL_LOOPBACK = 2,
    /* Rehearsal of the one-process-per-GPU model inside ONE process: every rank is its own
     * rt_multi handle (nlocal = 1, first_rank = its rank, the same unique_id, which keys an
     * in-process mailbox), each driven from its own thread as a separate process would drive
     * it, and each ncclSend/ncclRecv pair is a peer copy matched through the mailbox (the
     * root posts where the part lands and after which event; the sender's comm stream waits
     * for it, copies, and posts its completion event, which the root's comm stream waits
     * on).  Handles may share a device.  The host calls of a frame block until the peer's
     * matching post (RCCL's never block); a handle's failure or destroy ends the exchange
     * for all of them (RT_ERR_COMM, no hang). */
    RT_TRANSPORT_THREADS = 3,
    /* Rehearsal of the one-process-per-GPU model ACROSS processes, one per rank (nlocal = 1,
     * first_rank = its rank, the same unique_id — any RT_MULTI_ID_BYTES bytes the processes
     * share, e.g. random ones — naming a POSIX shared-memory mailbox; at most 64 ranks).
     * The THREADS protocol between processes: the root's staging buffers and every rank's
     * exchange events are shared once with hipIpcGetMemHandle / hipIpcGetEventHandle; a
     * sender's comm stream waits on the root's "ready" event, copies its part into the
     * root's staging buffer and records its "sent" event, on which the root's comm stream
     * waits before copying the part into the frame rows.  Processes may share a device (one
     * GPU).  rt_multi_create blocks until every rank has joined; the segment's name is
     * removed once all have.  A rank's failure ends the exchange for all of them
     * (RT_ERR_COMM); a peer process that exits is detected. */
    RT_TRANSPORT_IPC = 4
};
typedef struct rt_multi rt_multi;

/* A fresh communicator id (ncclGetUniqueId) for the one-process-per-GPU model. */
int rt_multi_unique_id(uint8_t id[RT_MULTI_ID_BYTES]);

/* devices[nlocal]: the HIP device of each local rank (global ranks first_rank ..
 * first_rank + nlocal - 1 of nranks).  RT_ERR_NO_DEVICE for a device index out of range,
 * RT_ERR_UNSUPPORTED for RT_TRANSPORT_RCCL with a device listed twice or
 * RT_TRANSPORT_COPY across processes, RT_ERR_COMM if RCCL fails. */
int rt_multi_create(const int32_t* devices, int32_t nlocal, int32_t nranks, int32_t first_rank,
                    const uint8_t* unique_id, int32_t transport, rt_multi** out);
int rt_multi_destroy(rt_multi* m);
const char* rt_multi_last_error(const rt_multi* m);

/* rt_set_scene / rt_set_option on every local rank's ctx (each rank keeps its own per-band
 * state: tile boxes, measured row order). */
int rt_multi_set_scene(rt_multi* m, const rt_prim* prims, int32_t n);
int rt_multi_set_option(rt_multi* m, int32_t option, int64_t value);
/* rt_set_lights on every local rank's ctx (every process of a multi-process operator calls it
 * with the same lights, as rt_multi_set_scene). */
int rt_multi_set_lights(rt_multi* m, const rt_light* lights, int32_t n);
/* rt_set_transmission on every local rank's ctx, likewise. */
int rt_multi_set_transmission(rt_multi* m, const rt_transmission* recs, int32_t n);

/* Enqueue one frame.  d_frame: on the process holding the root, DEVICE memory on the root's
 * device of height x width pixels of out_format (the root's band is rendered into it in
 * place, the other bands are received into their rows); NULL on other processes.  stream
 * (a hipStream_t on the root's device; NULL = the root ctx's stream): the frame's work
 * starts after the work already on it, and work enqueued on it later sees the complete
 * frame.  On a process without the root, a non-NULL stream (on that rank's device) waits for
 * the rank's band to have been sent.  No host synchronisation. */
int rt_multi_render_device(rt_multi* m, const rt_camera* cam, int32_t depth, int32_t precision,
                           uint32_t flags, int32_t out_format, void* d_frame, void* stream);

/* nframes frames as rt_multi_render_device calls in order would enqueue them: frame f
 * renders cams[f % ncams] into d_frames[f % nbufs] on streams[f % nstreams]. */
int rt_multi_render_device_frames(rt_multi* m, const rt_camera* cams, int32_t ncams,
                                  int32_t depth, int32_t precision, uint32_t flags,
                                  int32_t out_format, void* const* d_frames, int32_t nbufs,
                                  void* const* streams, int32_t nstreams, int32_t nframes);

/* Synchronous: the gathered frame in caller-owned HOST memory `out` (height x width pixels
 * of out_format) on the process holding the root (out may be NULL elsewhere).
 * stats->ms = device time from the start of the frame's work to the complete frame on the
 * root (render + gather); stats->segments is not counted (0). */
int rt_multi_render(rt_multi* m, const rt_camera* cam, int32_t depth, int32_t precision,
                    uint32_t flags, int32_t out_format, void* out, rt_stats* stats);

/* Waits for every frame this process enqueued; RT_ERR_COMM if RCCL reported an
 * asynchronous error. */
int rt_multi_sync(rt_multi* m);

/* Per-tile-row weights (n = tile rows of the frames to come, rt_tile_rows() pixel rows each)
 * for RT_OPT_MULTI_LAYOUT = 2, e.g. rt_tile_row_costs of one GPU's render of the frame.
 * Every rank must be given the same weights (one process per GPU: broadcast them).  n = 0
 * clears them.  Frames in flight keep the bands they started with. */
int rt_multi_set_row_weights(rt_multi* m, const float* weights, int32_t n);

/* Contiguous band of `rank` whose boundaries fall on tile rows: boundary r (0 < r < nranks)
 * is the tile row t whose prefix sum of weights[0..t) is nearest r/nranks of the total (ties
 * to the lower t; boundaries never decrease).  weights must hold one entry >= 0 per tile row
 * of `height` (n == ceil(height / rt_tile_rows())); otherwise RT_ERR_INVALID_ARG. */
int rt_weighted_band_rows(int32_t height, int32_t nranks, int32_t rank, const float* weights,
                          int32_t n, int32_t* row0, int32_t* nrows);

/* Measured cost of every tile row of the frame (synchronous): one render of the whole frame
 * by the stamped kernels, in which every wave records its shader cycles; costs[t] = the sum
 * over tile row t's waves in units of 32 cycles.  n must be ceil(height / rt_tile_rows()). */
int rt_tile_row_costs(rt_ctx* ctx, const rt_camera* cam, int32_t depth, int32_t precision,
                      uint32_t flags, float* costs, int32_t n);

/* Interleaved parts: the frame's tile rows (rt_tile_rows() = 8 pixel rows each; the last may be shorter)
 * dealt round-robin to nparts parts — part p owns tile rows p, p + nparts, p + 2 nparts, ...
 * — so every part gets a share of the frame's heavy and light rows (rt_multi's balanced
 * layout, RT_OPT_MULTI_LAYOUT).  *nrows = the part's pixel rows. */
int rt_interleaved_rows(int32_t height, int32_t nparts, int32_t part, int32_t* nrows);

/* rt_render_device for interleaved part `part` of `nparts`: out_frame_rows == 0 stores the
 * part's rows back to back in frame order (rt_interleaved_rows x width pixels in d_out);
 * != 0 stores every row at its frame row (d_out is the whole frame; the other parts' rows
 * are not touched).  nparts == 1 is the whole frame.  With RT_OPT_SUPERSAMPLE > 1 and
 * nparts > 1: RT_ERR_UNSUPPORTED. */
int rt_render_device_interleaved(rt_ctx* ctx, const rt_camera* cam, int32_t nparts, int32_t part,
                                 int32_t depth, int32_t precision, uint32_t flags,
                                 int32_t out_format, void* d_out, int32_t out_frame_rows,
                                 uint64_t* d_segments, void* stream);

/* ---- host helpers (restatements the host side of rt_scene needs) -------- */
/* Camera::init (scene.cpp:80-106) in fp64: fills cam from the Camera fields.
 * height = (int)(image_width / aspect_ratio) exactly as scene.cpp:82. */
int rt_camera_init(const double position[3], const double lookat[3], const double vup[3],
                   double vfov, double aspect_ratio, double image_width, rt_camera* cam);

/* The camera of RT_OPT_SUPERSAMPLE's S-times larger frame (host only, no device call):
 * pixel (j*S + a, i*S + b) of *out is sub-sample (a, b) of cam's pixel (j, i) on the regular
 * S x S grid of sub-pixel centres.  Per component k, in this order (outputs compare
 * bitwise): dxs = dx[k] / S, dys = dy[k] / S, h = (S - 1) * 0.5,
 * tl'[k] = (tl[k] - dxs * h) - dys * h, dx'[k] = dxs, dy'[k] = dys; position unchanged,
 * width' = width * S, height' = height * S.  S = 1 copies cam.  RT_ERR_INVALID_ARG for a
 * null pointer, S outside {1, 2, 4, 8}, or a product that overflows int32. */
int rt_supersample_camera(const rt_camera* cam, int32_t s, rt_camera* out);

/* Bytes per pixel of an output format (0 for an unknown format). */
int32_t rt_out_bytes_per_pixel(int32_t out_format);

/* Row band owned by `rank` of `nranks` when the frame is split into contiguous
 * blocks for multi-GPU tiling: [*row0, *row0 + *nrows). */
int rt_band_rows(int32_t height, int32_t nranks, int32_t rank, int32_t* row0, int32_t* nrows);

/* Diagnostics, host only (no device): the per-frame pixel boxes of the tile bins for a
 * scene and camera, as the linear-scan kernels would receive them (<= 64 primitives, else
 * *nbox = 0).  out receives 4 int16 per box {x0, x1, i0, i1} (inclusive pixel column and
 * frame row ranges; x0 > x1 = never hit): the *nbox primary boxes in material-slot order
 * (spheres in scene order, then walls in scene order, z-normal walls that can never be hit
 * dropped), then for each mirror level L = 1..*mir_depth the nW^L wall sequences (base-nW
 * number w1..wL) of *nbox boxes each.  RT_ERR_INVALID_ARG when cap (boxes) is too small
 * (*nbox and *mir_depth are still set). */
int rt_frame_boxes(const rt_prim* prims, int32_t n, const rt_camera* cam, int32_t row0,
                   int32_t nrows, int16_t* out, int32_t cap, int32_t* nbox, int32_t* mir_depth);

/* Diagnostics, host only (no device): the dispatch order RT_OPT_ROW_FEEDBACK derives from a
 * cost snapshot of n <= 2048 dispatch units (unit_max[u]: the unit's most expensive wave,
 * clamped to 65535; unit_sum[u]: the sum of its waves' costs), by the function the frame
 * loop uses.  mode 0 = heaviest first by unit_max, ties to the lower unit; mode 1 =
 * RT_OPT_ROW_MIX's mixed order.  perm receives n unit indices.  RT_ERR_INVALID_ARG for
 * n < 0, n > 2048, a null pointer or another mode. */
int rt_order_units(const uint32_t* unit_max, const uint32_t* unit_sum, int32_t n, int32_t mode,
                   int16_t* perm);

/* Diagnostics: the row feedback's reduction kernel on caller-supplied wave costs (host
 * array of gy rows of gx 16-bit costs): with 2^units_log2 dispatch units per row of
 * U = ceil(gx / 2^units_log2) waves, unit_max and unit_sum (host, gy << units_log2 words
 * each) receive every unit's maximum and sum.  Synchronous.  RT_ERR_INVALID_ARG for null
 * pointers, gy or gx outside [1, 65535], units_log2 outside [0, 3]. */
int rt_unit_costs(rt_ctx* ctx, const uint16_t* cost, int32_t gy, int32_t gx, int32_t units_log2,
                  uint32_t* unit_max, uint32_t* unit_sum);

/* Largest depth the kernels are compiled for (depth 0..rt_max_depth()). */
int32_t rt_max_depth(void);

/* Pixel rows per tile row of the kernels (the unit rt_interleaved_rows deals, 8). */
int32_t rt_tile_rows(void);

/* ---- diagnostics -------------------------------------------------------- */
/* Device self-test of the fp64 helpers the exact path relies on, over n seeded random
 * operands: test 0 = division with a shared refined reciprocal vs IEEE `/` (bitwise),
 * test 1 = integer-exponent pow by squaring vs pow() (within 128 ulp),
 * test 2 = the range-restricted sqrt sequence vs sqrt() (bitwise).
 * *mismatches receives the number of failures (0 expected). */
int rt_selftest(rt_ctx* ctx, int32_t test, uint64_t n, uint64_t seed, uint64_t* mismatches);

#ifdef __cplusplus
}
#endif
#endif /* RT_CAPI_H */
