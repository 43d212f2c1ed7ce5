/*
 * rt_device.h — device-side scene layout and launch arguments (internal; not ABI).
 *
 * HBM layout of one uploaded scene (one allocation, built by rt_set_scene; every
 * section 256-B aligned, sphere sections padded to a multiple of 4 records):
 *
 *   SphG32 [ceil(nS/4)]   4 spheres per 64 B  : cx[4] cy[4] cz[4] r[4]  fp32 (SoA)
 *   SphG64 [ceil(nS/4)]   4 spheres per 128 B : {cx, cy, cz, radius^2} fp64
 *   Wall32 [nW]           64 B  : P, n, X, Y, length, width            fp32
 *   Wall64 [nW]           128 B : P, n, X, Y, length, width            fp64
 *   int32  sph_j[nS]      scene index of each sphere (tie-break only)
 *   int32  wall_j[nW]     scene index of each wall (tie-break only)
 *   DevMat [nS + nW]      64 B, spheres first then walls, indexed by "material slot"
 *   DevMat32 [nS + nW]    32 B, fp32 copy for the fp32 colour paths
 *   double wnn[nW][4]     normalize(n) of each wall (32 B)
 *
 * The per-ray scan (find_closest_hit, main.cpp:67-84) runs one loop over sphere groups
 * and one over walls instead of a virtual call per primitive.  Every lane of a wave tests
 * the same primitive, so records are wave-uniform: a whole group of 4 spheres arrives
 * with one s_load_dwordx16 into scalar registers and feeds the VALU as scalar operands
 * (no LDS traffic, no VGPRs, one scalar-load latency per 4 spheres).  Spheres keep scene
 * order, so ties between spheres resolve by position in the array; a wall that ties the
 * current best compares scene indices (strict `<` in scene order == lowest index wins).
 * Ray-invariant work the reference redoes per test — the wall basis (scene.cpp:18-19)
 * and radius*radius (scene.cpp:51) — is computed once on the host with the same fp64
 * operations, so every value is bit-identical to the reference's.
 */
#ifndef RT_DEVICE_H
#define RT_DEVICE_H

#include <stdint.h>

namespace rt {

struct alignas(64) SphG32 {
    float c[4][4];   // [component cx, cy, cz, radius][sphere]: SoA so that two spheres'
                     // same component form an SGPR pair for packed fp32 (v_pk_*) math
};
struct alignas(128) SphG64 {
    double v[4][4];  // [sphere][cx, cy, cz, radius*radius]
};
struct alignas(64) Wall32 {
    float P[3], n[3], X[3], Y[3], len, wid, pad[2];
};
struct alignas(128) Wall64 {
    double P[3], n[3], X[3], Y[3], len, wid, pad[2];
};
struct alignas(64) DevMat {
    double color[3];
    double ka, km, kd, ks, ex;
};
static_assert(sizeof(SphG32) == 64 && sizeof(SphG64) == 128, "sphere group layout");
static_assert(sizeof(Wall32) == 64 && sizeof(Wall64) == 128, "wall layout");
struct alignas(32) DevMat32 {
    float color[3];
    float ka, km, kd, ks, ex;
};
static_assert(sizeof(DevMat) == 64, "material layout");
static_assert(sizeof(DevMat32) == 32, "material layout");

enum { PREC_F64 = 0, PREC_F32 = 1, PREC_MIXED = 2, PREC_PATH64 = 3 };
enum { OUT_RGB_F32 = 0, OUT_RGB_F64 = 1, OUT_RGBA8 = 2, OUT_RGBA8_WRAP = 3 };
enum { FLAG_SUN = 1, FLAG_SHADOWS = 2 };
// Host-internal bit of KParams::flags (never an rt_capi.h flag): the frame was prepared with
// scene lights set (rt_set_lights) and launches the lights kernels.
constexpr uint32_t FLAG_LIGHTS = 0x80000000u;
// The same for transmission records (rt_set_transmission): the frame launches the glass kernels.
constexpr uint32_t FLAG_GLASS = 0x40000000u;

// Pixel tile of one workgroup: RT_WAVES_PER_BLOCK waves (1, 2 or 4), each an 8x8 square.
// One wave per workgroup measured fastest (tools/ab.py: c5 -15..21%, c3 -7..12%, c2 -2%
// vs four): finer dispatch granularity at 3-5 waves/SIMD.
#ifndef RT_WAVES_PER_BLOCK
#define RT_WAVES_PER_BLOCK 1
#endif
constexpr int BLOCK = 64 * RT_WAVES_PER_BLOCK;
constexpr int TILE_W = RT_WAVES_PER_BLOCK >= 2 ? 16 : 8;
constexpr int TILE_H = RT_WAVES_PER_BLOCK >= 4 ? 16 : 8;

// Camera-origin ("eye") tables of the primary segment.  Every primary ray starts at the
// camera position, so the origin-only terms of both tests — Sphere::intersect's
// ray_sphere_vec and c (scene.cpp:45, 51) and Wall::intersect's numerator
// dot(position - origin, normal) (scene.cpp:10) — are the same for every pixel of a
// frame.  The host evaluates them once per render with the reference's fp64 operations
// (bit-identical values) and passes them in the kernel arguments, which the kernel reads
// with scalar loads: the primary test then costs the direction-dependent half only.
// Used by the F64/PATH64 linear-scan kernels when the scene fits (eye != 0); A/B at
// c2: -2..3%.  (The fp32 path measured slower with them.)
constexpr int EYE_MAX_S = 32;
constexpr int EYE_MAX_W = 16;

// Primary-ray tile bins.  Every primary ray starts at the camera o with direction
// d(x, i) = o - (TL + dx*x + dy*i) (main.cpp:132-133), so a point X = o + u*d(x, i) has
// pixel coordinates (x, i) = (p/u, q/u) where (u, p, q) = M^-1 (X - o), M = [o - TL, -dx,
// -dy]: a projective map.  Per frame the host projects each primitive's convex hull (a
// sphere's bounding cube, a wall's rectangle clipped to u >= eps) to a pixel bounding box
// widened by one pixel (rt_capi.cpp frame_boxes); the kernel ANDs its 8x8 tile against
// the boxes (one lane per primitive, one ballot) and the primary scan tests only the
// primitives whose box meets the tile.  A primitive outside the box by >= 1 pixel is
// missed by the exact ray by an angle ~1e12 times the reference's rounding, so the
// reference's own test rejects it too.  Scenes of <= 64 primitives.
constexpr int BIN_MAX_PRIMS = 64;
// Mirror bins.  A reflection off a plane is linear: the first-bounce ray of pixel (x, i)
// off wall w (origin pos + 1e-4 n, direction reflect(d, n), main.cpp:111-113) lies on the
// line from the camera mirrored in w's plane (shifted by 1e-4 n) with direction R d(x, i),
// R = I - 2 n n^T, again affine in (x, i); a chain of wall bounces composes the
// reflections.  So a wave whose live rays all followed the same wall sequence can cull
// the next segment with the pixel boxes of that virtual camera, computed per frame like
// the primary boxes for every sequence of up to MIR_MAX_DEPTH walls that some tile can
// follow.  Sequence (w1..wL) of level L: boxes at mbox[(off_L + q) * nbox ..], q the
// base-nW number w1..wL, off_L = nW + nW^2 + .. + nW^(L-1).
constexpr int MIR_MAX_DEPTH = 3;
#ifndef RT_MIR_MAX_BOXES
#define RT_MIR_MAX_BOXES 256
#endif
constexpr int MIR_MAX_BOXES = RT_MIR_MAX_BOXES;
struct PrimBox {
    int16_t x0, x1, i0, i1;  // inclusive pixel box (frame rows); x0 > x1 = never hit
};

// Sphere clusters for the cull kernels' wide-cone waves (rt_scan_dev.h clusters_scan).  The
// host splits the spheres at the median of the centres' widest axis until each leaf holds
// <= CLU_SIZE of them (rt_capi.cpp build_clusters); each leaf gets an fp32 box around its
// balls widened by a margin far above fp32 rounding, and a copy of its spheres' exact fp64
// records in leaf order.  A lane tests its own ray against the leaf boxes, then runs the
// exact test on the spheres of its own leaves only: a wave's iteration count is its worst
// lane's, not the union of its lanes' candidates (which is what the wave cone pays when the
// live rays point everywhere).
// Two leaf sizes, one cluster set each: the F32 kernels' walk (cheap sphere tests, so the
// box pass dominates) wants few leaves, the fp64 kernels' walk (exact fp64 tests) small ones
// (A/B round 4: leaves of 4 vs 8, c3 PATH64 -6%, c5 -0.5..0.9%, but F32 c5 +7.6%).  The fp64
// set falls back to CLU_SIZE leaves when its own would exceed CLU_MAX.
#ifndef RT_CLU_SIZE
#define RT_CLU_SIZE 8
#endif
#ifndef RT_CLU_SIZE_D
#define RT_CLU_SIZE_D 4
#endif
constexpr int CLU_SIZE = RT_CLU_SIZE;      // F32 kernels
constexpr int CLU_SIZE_D = RT_CLU_SIZE_D;  // fp64-path kernels (F64, MIXED, PATH64)
constexpr int CLU_MAX = 64;
static_assert(CLU_SIZE_D <= CLU_SIZE, "the fp64 walk's loop covers CLU_SIZE_D or CLU_SIZE");
struct alignas(32) Clu32 {
    float lo[3], hi[3];
    uint8_t rank[8];  // position of this cluster in the near-to-far order of each direction
                      // octant (bit 0/1/2 = d.x/d.y/d.z < 0): the host sorts the clusters by
                      // their centroid along the octant's diagonal
};
struct alignas(64) CluSph {
    double c[4];     // cx, cy, cz, radius^2 (the SphG64 record)
    float f[4];      // cx, cy, cz, radius (the SphG32 record, F32 kernels)
    int32_t slot;    // material slot = sphere index, -1 = padding
    int32_t pad[3];
};
static_assert(sizeof(Clu32) == 32 && sizeof(CluSph) == 64, "cluster layout");

// Dispatch order given explicitly: up to ROW_PERM_MAX units (tile rows of 8 pixel rows, or
// parts of them), int16 each, in the kernel arguments.
#ifndef RT_ROW_PERM_MAX
#define RT_ROW_PERM_MAX 2048
#endif
constexpr int ROW_PERM_MAX = RT_ROW_PERM_MAX;

struct KParams {
    const SphG32* s32;
    const SphG64* s64;
    const Wall32* w32;
    const Wall64* w64;
    const int32_t* sph_j;
    const int32_t* wall_j;
    const DevMat* mat;     // [nS + nW]
    const DevMat32* mat32; // [nS + nW]
    const double (*wnn)[4];  // [nW] normalize(wall normal) (vec.cpp:21, host), the normal
                             // every reflection / shading step normalises again
    int32_t nS, nW;
    int32_t int_exp;       // every specular exponent is an integer in [0, 1024]
    int32_t wave_cull;     // cull spheres per wave (rt_scan_dev.h) before the per-lane tests
    int32_t W, row0, nrows, depth;
    uint32_t flags;
    int32_t outf;
    double pos[3], tl[3], dx[3], dy[3];
    void* out;
    unsigned long long* segs;   // may be null
    unsigned long long* stats;  // diagnostic counters, may be null (rt_set_option)
    int32_t nbox;               // primitives with a PrimBox (nS + nW), 0 = tile bins off
    int32_t row_center;         // tile row dispatched first (rt_frame_dev.h tile_row), -1 = off
    uint16_t* tile_cost;        // per wave (workgroup row-major over the frame's tiles, then
                                // wave): shader cycles / 32, saturated; null = not recorded
    int32_t row_units_log2;     // each tile row split into 2^k dispatch units (k > 0 only
                                // with a row_perm over units: unit u = row (u >> k), part
                                // (u & (2^k - 1)) of ceil(tiles / 2^k) tiles)
    int32_t row_perm_n;         // dispatch units in row_perm (== the grid's rows), 0 = unused
    int16_t row_perm[ROW_PERM_MAX];  // dispatch order of tile rows (rt_frame_dev.h tile_row)
    PrimBox box[BIN_MAX_PRIMS]; // material-slot order: spheres, then walls (scenes with the
                                // wave cull: the walls' boxes only, box[w] = wall w)
    int32_t nwbox;              // wave-cull scenes: walls with a PrimBox in box[] (0 = off)
    int32_t mir_depth;          // wall-sequence levels with mirror boxes (0 = off)
    int32_t pairs;              // RT_OPT_PIXEL_PAIRS: PATH64 linear-scan frames trace two
                                // pixels per lane (16x8 pixels per wave)
    PrimBox mbox[MIR_MAX_BOXES];  // [sequence][slot j]: primitive j through the camera
                                  // mirrored along the sequence (see above)
    int32_t eye;                        // eye tables below valid
    int32_t wall_order_n;               // walls in wall_order (== nW), 0 = index order
    uint64_t wall_order;                // primary scan's wall visiting order, 4 bits per
                                        // wall slot, nearest to the camera first (host)
    double eye_s[EYE_MAX_S][4];         // sphere s: {oc.x, oc.y, oc.z, |oc|^2 - r^2}
    double eye_w[EYE_MAX_W];            // wall w: dot(P - pos, n)
    const Clu32* clu;      // [nclu] sphere-cluster boxes (cull kernels), see above
    const CluSph* csph;    // [nclu * clu_ls] their spheres in cluster order
    const uint8_t* cord;   // [8][CLU_MAX] cluster at each rank of each octant's order
    int32_t nclu;          // 0 = no clusters
    int32_t clu_ls;        // spheres per leaf record: CLU_SIZE_D or CLU_SIZE (F32: CLU_SIZE)
    int32_t clu_axis;      // axis of the first split (0..2): lanes walk clusters against it
    float clu_cos;         // wide-cone waves (cone cos(half-angle) < clu_cos) use clusters
    float clu_oinf;        // rays whose |origin|inf exceeds it test every cluster (the box
                           // margin covers fp32 rounding only for origins near the scene)
    // interleaved parts (rt_render_device_interleaved): tstride > 1 = the band is the
    // frame's tile rows tphase, tphase + tstride, ... (nrows = their pixel rows, row0 = 0);
    // frame_h = frame height; out_frame = store at frame rows instead of back to back
    int32_t tstride, tphase, frame_h, out_frame;
    // RT_OPT_SUPERSAMPLE: S = 2^ss_log2 (0 = off).  W, row0, nrows and the camera are the
    // S-times larger frame's; the kernel stores the mean of each S x S square of its pixels
    // at row (band row >> ss_log2), column (x >> ss_log2) of an output W >> ss_log2 wide
    // (rt_frame_dev.h ss_resolve).  Contiguous bands only.
    int32_t ss_log2;
};
// by-value kernel arguments of up to 16 KB arrive intact (tools/ubench/kernarg_size.hip,
// kernarg_stale.hip: consistent across back-to-back launches)
static_assert(sizeof(KParams) <= 16384, "kernel arguments over 16 KB");

// Host-side launchers (rt_trace.hip).  Return a hipError_t as int.  done_event (a
// hipEvent_t, may be null) is signalled by the kernel's own completion (hipExtLaunchKernel
// stop event: no separate marker packet, unlike a hipEventRecord behind the launch).
int launch_trace(const KParams& p, int prec, void* stream, void* done_event = nullptr);
// nframes frames of one band in ONE launch (grid.z = frame): d_tab = their KParams in device
// memory, p0 = a host copy of the first (grid, kernel choice: every frame must share its W,
// nrows, row_units_log2, depth, flags, precision and scene).  The linear-scan kernels only:
// hipErrorNotSupported for a wave-cull scene or RT_OPT_PIXEL_PAIRS.
int launch_trace_batch(const KParams* d_tab, const KParams& p0, int nframes, int prec, void* stream,
                       void* done_event);
int max_depth();
// A frame with FLAG_SHADOWS (rt_trace_shadow.hip): F64 (MIXED is served by it) and PATH64, one
// pixel or one sample per lane, no sun, no frame table, no cost stamps; hipErrorInvalidValue
// for anything else.
int launch_trace_shadow(const KParams& p, int prec, void* stream, void* done_event);

// Ray batches (rt_trace_rays*, rt_rays.hip): one lane per caller ray, ray blockIdx.x * BLOCK +
// threadIdx.x.  The scene, depth, flags, output format and pointer, segment counter and cull
// options travel in a KParams whose frame fields (camera, boxes, row order, eye tables) are
// unused; the rays themselves in RayArgs.
struct DevHit {  // == rt_hit (rt_capi.h)
    double distance;
    double normal[3];
    int32_t index, reserved;
};
static_assert(sizeof(DevHit) == 40, "rt_hit layout");
struct RayArgs {
    const double* org;  // [n][3]
    const double* dir;  // [n][3], not normalised
    DevHit* hits;       // [n] closest hit of each ray's first segment, may be null
    int32_t n;
    int32_t shade;      // 0: hits only (KParams::out unused): one segment per ray, no shading
};
// prec: PREC_F64 or PREC_PATH64 (anything else: hipErrorInvalidValue)
int launch_rays(const KParams& p, const RayArgs& ra, int prec, void* stream, void* done_event);
// The same with FLAG_SHADOWS (rt_rays_shadow.hip): radiance only (ra.shade), no sun.
int launch_rays_shadow(const KParams& p, const RayArgs& ra, int prec, void* stream, void* done_event);

// Scene lights (rt_set_lights): the records of the lights kernels (rt_trace_lights.hip,
// rt_rays_lights.hip), which take them by value behind their KParams, so a launch keeps the
// lights it was enqueued with and no other kernel's arguments change.  Wave-uniform, read
// through scalar loads.  colf: the colour rounded to fp32 for PATH64's colour arithmetic.
constexpr int MAX_LIGHTS = 8;
struct DevLight {
    double pos[3];
    double col[3];
    float colf[3];
    float pad;
};
static_assert(sizeof(DevLight) == 64, "light record layout");
struct LightArgs {
    DevLight l[MAX_LIGHTS];
    int32_t n;  // 1..MAX_LIGHTS in a launch (0 on a ctx without lights: the plain kernels)
    int32_t pad;
};
// A frame / a radiance batch with la.n >= 1 lights: F64 (MIXED is served by it) and PATH64, no
// sun; FLAG_SHADOWS in p.flags is a wave-uniform runtime branch of the same kernels.  The
// frame launcher has launch_trace_shadow's conditions otherwise.
int launch_trace_lights(const KParams& p, const LightArgs& la, int prec, void* stream, void* done_event);
int launch_rays_lights(const KParams& p, const RayArgs& ra, const LightArgs& la, int prec, void* stream,
                       void* done_event);

// Transmission (rt_set_transmission): one record per material slot (spheres, then walls, as
// KParams::mat), in a device table the ctx owns.  The glass kernels (rt_trace_glass.hip,
// rt_rays_glass.hip) are the lights kernels with another next-ray step at a hit whose tau > 0 (a
// pane passes the ray on, a sphere refracts it in, along the chord and out) and w in km's place
// in the unwind.  The table's pointer travels by value behind the light records.
struct DevGlass {
    double tau;  // rt_transmission::transmission; 0 = opaque: the reflection step
    double ior;  // spheres only
    double w;    // the unwind's weight: tau > 0 ? tau : the material's metallic
    float wf;    // w rounded to fp32 (PATH64's colour arithmetic)
    float pad;
};
static_assert(sizeof(DevGlass) == 32, "transmission record layout");
struct GlassArgs {
    const DevGlass* rec;  // [nS + nW]
};
// A frame / a radiance batch while records are set: launch_trace_lights' / launch_rays_lights'
// conditions; la holds at least one light (the host passes the reference's when none is set).
int launch_trace_glass(const KParams& p, const LightArgs& la, const GlassArgs& ga, int prec, void* stream,
                       void* done_event);
int launch_rays_glass(const KParams& p, const RayArgs& ra, const LightArgs& la, const GlassArgs& ga, int prec,
                      void* stream, void* done_event);

// Occlusion queries (rt_occluded*, rt_rays.hip k_ray_occluded): is anything on the segment
// o .. o + d * tmax of each caller ray?  Only the scene and cull fields of KParams are used.
struct OccArgs {
    const double* org;   // [n][3]
    const double* dir;   // [n][3], not normalised
    const double* tmax;  // [n] parametric limit of each ray, null = +inf for every ray
    uint8_t* out;        // [n] 1 = occluded, 0 = free; may be null
    unsigned long long* count;  // += occluded rays (one atomic per wave); may be null
    int32_t n;
};
int launch_occluded(const KParams& p, const OccArgs& oa, void* stream, void* done_event);

// Frame AOVs (rt_render_aov*, rt_trace_aov.hip k_aov): the primary segment of the frame p
// describes (camera, band, eye tables, wall order, primary boxes; one 8x8 tile per wave like the
// frame kernels), its hit written as per-pixel layers, band-relative and row-major.  The layer
// pointers travel by value behind the KParams; a null layer is not written (wave-uniform).
struct AovArgs {
    DevHit* hit;     // [nrows * W] find_closest_hit's record (k_ray_hits' bytes)
    int32_t* index;  // [nrows * W] scene index, -1 = miss
    float* depth;    // [nrows * W] world distance camera .. hit, +inf = miss
    float* normal;   // [nrows * W][3] normalize(record normal), 0 = miss
    float* albedo;   // [nrows * W][3] the hit material's colour, 0 = miss
};
int launch_aov(const KParams& p, const AovArgs& a, void* stream, void* done_event);

// Ambient occlusion frames (rt_render_ao*, rt_trace_ao.hip k_ao): k_aov's primary segment of the
// frame p describes, then ndirs any-hit probes at every hit.  The probe directions travel by
// value behind the KParams, so a launch keeps the directions it was enqueued with; they are
// wave-uniform and read through scalar loads.  A null layer is not written (wave-uniform).
constexpr int AO_MAX_DIRS = 64;  // == RT_AO_MAX_DIRS (rt_capi.h)
struct AoArgs {
    uint8_t* count;  // [nrows * W] occluded probes of the pixel, 0 = miss
    float* ao;       // [nrows * W] (ndirs - count) / ndirs, 1 = miss
    double radius;   // the probes' parametric limit, > 0 (+inf allowed)
    int32_t ndirs;   // 1..AO_MAX_DIRS
    int32_t pad;
    double dirs[AO_MAX_DIRS][3];  // the caller's directions, not normalised
};
int launch_ao(const KParams& p, const AoArgs& a, void* stream, void* done_event);

// Device self-test of the exact fp64 helpers against IEEE operations:
// which 0 = division (shared reciprocal), 1 = integer-exponent pow vs pow(),
// 2 = sqrt_e vs sqrt(); adds the number of mismatches (division, sqrt: bitwise;
// pow: > 128 ulp) to *d_bad.
int launch_selftest(int which, uint64_t n, uint64_t seed, unsigned long long* d_bad,
                    void* stream);
// Row feedback: with nu = gy << ul dispatch units, ustat[(r << ul) + q] = the largest and
// ustat[nu + (r << ul) + q] = the sum of cost[r * gx + q * U ..] over dispatch unit q of row r
// (U = ceil(gx / 2^ul)), for gy rows of gx wave costs.
int launch_unit_max_sum(const uint16_t* cost, int gy, int gx, int ul, uint32_t* ustat, void* stream);

}  // namespace rt

#endif
