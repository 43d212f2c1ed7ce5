/*
 * rt_host.h — the pure host half of the C-ABI (internal; not ABI): the packed scene, the
 * per-frame kernel arguments and the measured dispatch order.  Nothing here or in the units
 * behind it (rt_scene_pack.cpp, rt_frame_args.cpp, rt_row_order.cpp) includes a HIP header,
 * calls the runtime or sees an rt_ctx: they are fp64 / integer arithmetic on plain structs,
 * compiled as plain C++, and can be timed and sanitised without a device.
 */
#ifndef RT_HOST_H
#define RT_HOST_H

#include <cmath>
#include <cstddef>
#include <vector>

#include "../../include/rt_capi.h"
#include "rt_device.h"

#ifndef RT_CLUSTER_COS_DEFAULT  // build-time default of RT_OPT_CLUSTER_COS (x 1000)
#define RT_CLUSTER_COS_DEFAULT 400
#endif
#ifndef RT_WALL_ORDER_DEFAULT   // build-time default of RT_OPT_WALL_ORDER (A/B builds)
#define RT_WALL_ORDER_DEFAULT 0
#endif
#ifndef RT_PIXEL_PAIRS_DEFAULT  // build-time default of RT_OPT_PIXEL_PAIRS (A/B builds)
#define RT_PIXEL_PAIRS_DEFAULT 0
#endif

// everything internal to the host units: hidden, so the library exports the C-ABI only (the
// attribute covers one namespace body, so every unit that defines something in rth repeats it)
namespace rth __attribute__((visibility("hidden"))) {

/* vec.cpp restatements used to pack Wall invariants and by rt_camera_init (same fp64
 * operations). */
struct hv3 {
    double x, y, z;
};
inline hv3 hcross(hv3 u, hv3 v) {  // vec.cpp:15
    return {u.y * v.z - u.z * v.y, u.z * v.x - u.x * v.z, u.x * v.y - u.y * v.x};
}
inline hv3 hnormalize(hv3 v) {  // vec.cpp:21 (v / length())
    double l = std::sqrt(v.x * v.x + v.y * v.y + v.z * v.z);
    return {v.x / l, v.y / l, v.z / l};
}

/* ---- rt_scene_pack.cpp ---------------------------------------------------------------- */

/* One packed scene: the device image and the host copies the per-frame arguments read.
 * Written by pack_scene (rt_set_scene, on the caller's thread, with no frame in flight and
 * the helper thread idle); read-only afterwards, by the launching and the helper thread. */
struct SceneHost {
    int nS = 0, nW = 0, nP = 0;
    bool int_exp = true;
    size_t off_s64 = 0, off_w32 = 0, off_w64 = 0, off_sj = 0, off_wj = 0, off_mat = 0,
           off_mat32 = 0, off_wnn = 0, total = 0;
    struct CluSet {  // sphere clusters (rt_device.h) of one leaf size, nclu 0 = none
        size_t off_clu = 0, off_csph = 0, off_cord = 0;
        int nclu = 0, clu_axis = 0, ls = 0;
        float clu_oinf = 0.0f;
    } cset[2];  // [0]: the F32 kernels' (CLU_SIZE), [1]: the fp64 kernels' (CLU_SIZE_D)
    // the device image of the scene (rt_device.h layout), built in 256-byte aligned host
    // memory so its records (alignas 32-128) may be written through their own types
    struct alignas(256) Blk {
        char b[256];
    };
    std::vector<Blk> blocks;
    char* image() { return reinterpret_cast<char*>(blocks.data()); }
    std::vector<double> h_sph;  // nS x {cx, cy, cz, radius^2, radius}
    std::vector<double> h_wal;  // nW x {P, n, X, Y, length, width}
    std::vector<double> h_km;   // metallic of each material slot
};

/* rt_set_scene's host half: the device image of the scene (rt_device.h layout) and the
 * host copies the per-frame boxes and eye tables use. */
int pack_scene(const rt_prim* prims, int32_t n, SceneHost& sc);

/* rt_set_lights' host half: the checked records as the lights kernels take them
 * (rt::LightArgs).  n == 0 gives out.n == 0, the reference's light.  RT_ERR_INVALID_ARG, with
 * out untouched, for n outside 0..RT_MAX_LIGHTS, null lights with n > 0 or a non-finite
 * component. */
int pack_lights(const rt_light* lights, int32_t n, rt::LightArgs& out);

/* rt_set_transmission's host half: the checked records of scene sc as the glass kernels'
 * table, one rt::DevGlass per material slot (spheres, then walls; w = tau where tau > 0, else
 * the slot's metallic).  n == 0 or every transmission exactly 0 gives an empty out: no records.
 * RT_ERR_INVALID_ARG, with out untouched, for n neither 0 nor sc.nP, null recs with n > 0, a
 * non-finite field, transmission outside [0, 1] or ior outside [1, 4]. */
int pack_transmission(const rt_transmission* recs, int32_t n, SceneHost& sc, std::vector<rt::DevGlass>& out);

/* ---- rt_frame_args.cpp ---------------------------------------------------------------- */

/* The options a frame's arguments depend on.  Written by rt_set_option between calls;
 * read-only while a call runs, by the launching and the helper thread. */
struct FrameOptions {
    int wave_cull_min = 24;  // spheres from which the wave cull pays (tools/sweep.py)
    bool eye_tables = true;  // RT_OPT_EYE_TABLES
    float clu_cos = RT_CLUSTER_COS_DEFAULT / 1000.0f;  // RT_OPT_CLUSTER_COS
    bool wall_order = RT_WALL_ORDER_DEFAULT;  // RT_OPT_WALL_ORDER
    bool tile_bins = true;   // RT_OPT_TILE_BINS
    bool row_order = true;   // RT_OPT_ROW_ORDER
    bool mirror_bins = true; // RT_OPT_MIRROR_BINS
    bool pixel_pairs = RT_PIXEL_PAIRS_DEFAULT;  // RT_OPT_PIXEL_PAIRS
    bool box_cache_on = true;  // RT_OPT_BOX_CACHE
    int ss_log2 = 0;         // RT_OPT_SUPERSAMPLE: S = 2^ss_log2 rays per pixel side
    bool lights = false;     // rt_set_lights with n > 0: frames carry rt::FLAG_LIGHTS
    bool glass = false;      // rt_set_transmission with records: frames carry rt::FLAG_GLASS
    unsigned long long* d_stats = nullptr;  // RT_OPT_STATS_DEVICE_PTR (passed on, never read)
};

/* The per-frame boxes depend only on the scene, the camera, the row band and the options: a
 * render with the same inputs as the previous one reuses them (the host part of a frame is
 * ~60 us with mirror chains, more than the kernel at c2).  Read and written by make_params
 * alone, so by one thread at a time: the helper thread while a pipelined batch runs, the
 * launching thread otherwise. */
struct BoxCache {
    bool valid = false;
    unsigned long long scene_gen = 0;
    rt_camera cam{};
    int32_t row0 = 0, nrows = 0, wave_cull = 0, opts = 0;
    int32_t nbox = 0, nwbox = 0, row_center = 0, mir_depth = 0;
    size_t nmbox = 0;
    rt::PrimBox box[rt::BIN_MAX_PRIMS];
    rt::PrimBox mbox[rt::MIR_MAX_BOXES];
};

/* What a frame's arguments are computed from besides the camera: all read-only. */
struct FrameScene {
    const SceneHost& sc;
    const FrameOptions& opt;
    const void* base;              // the device scene (null: host-only use, rt_frame_boxes)
    unsigned long long scene_gen;  // bumped by every rt_set_scene (the box cache's key)
};

/* What the caller asks of every frame, ray or segment of a call. */
struct FrameReq {
    int32_t depth, precision;
    uint32_t flags;
    int32_t out_format;
};

/* rt_supersample_camera's arithmetic (rt_capi.h: the operation order is part of the ABI). */
int supersample_camera(const rt_camera* cam, int32_t s, rt_camera* out);

/* The frame the kernels trace for a render of rows [row0, row0 + nrows) of cam: the caller's
 * own, or with RT_OPT_SUPERSAMPLE the S-times larger one (rt_supersample_camera, rows
 * row0*S .. ).  Every internal step after the argument checks works on it. */
struct VirtFrame {
    rt_camera vcam;
    const rt_camera* cam;
    int32_t row0, nrows;
};
int virt_frame(int ss_log2, const rt_camera* cam, int32_t row0, int32_t nrows, VirtFrame& v);

/* The scene's part of the kernel arguments: the sections of the device image, the cluster
 * set of the precision, the scan choice (wave cull or linear). */
void scene_params(const FrameScene& fs, int32_t precision, rt::KParams& p);

/* Pixel boxes, row centre and mirror chains of one frame into p (p.wave_cull set). */
void frame_boxes(const SceneHost& sc, const FrameOptions& opt, const rt_camera* cam, int32_t row0,
                 int32_t nrows, rt::KParams& p);

/* Every kernel argument the host computes per frame; cam, row0, nrows: the frame the kernels
 * trace (virt_frame).  bc (may be null): the caller's box cache, read and updated. */
rt::KParams make_params(const FrameScene& fs, BoxCache* bc, const rt_camera* cam, int32_t row0,
                        int32_t nrows, const FrameReq& rq, void* d_out, unsigned long long* d_segs);

/* ---- rt_row_order.cpp ----------------------------------------------------------------- */

/* order_units' results and working vectors (no allocation in steady state). */
struct UnitOrder {
    std::vector<int16_t> perm;  // heaviest first, over dispatch units: 2^units_log2 per tile row
    std::vector<int16_t> mix;   // RT_OPT_ROW_MIX: perm with the light units merged in (mix_units)
    std::vector<float> acc;     // RT_OPT_ROW_FEEDBACK_EMA: per-unit smoothed maximum, for one band
    std::vector<uint32_t> work; // per-unit sum of the waves' costs (smoothed alike)
    std::vector<uint16_t> key;
    std::vector<int16_t> tmp, heavy, light;
};

/* Dispatch units per tile row (log2) of a grid of gy tile rows by gx waves. */
int units_log2(int gy, int gx);

/* o.perm and o.mix from the per-unit maxima and sums of a cost snapshot; acc_valid: o.acc and
 * o.work belong to the same band (smoothed with weight ema percent). */
void order_units(const uint32_t* umax, const uint32_t* usum, int nu, UnitOrder& o, bool acc_valid,
                 int ema);

}  // namespace rth

#endif
