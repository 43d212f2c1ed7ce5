/*
 * rt_frame_args.cpp — the kernel arguments the host computes per frame (pure host: no HIP,
 * no rt_ctx): the supersampled camera, the scene's sections, pixel boxes, mirror chains, the
 * row centre, eye tables and the wall order, from a packed scene (rt_scene_pack.cpp), the
 * device base pointer and the frame options.  This is the host's share of the hot path.
 */
#include <algorithm>
#include <cmath>
#include <cstring>
#include <vector>

#include "rt_host.h"

namespace rth __attribute__((visibility("hidden"))) {

int supersample_camera(const rt_camera* cam, int32_t s, rt_camera* out) {
    if (!cam || !out || (s != 1 && s != 2 && s != 4 && s != 8)) return RT_ERR_INVALID_ARG;
    const int64_t w = (int64_t)cam->width * s, h = (int64_t)cam->height * s;
    if (w > INT32_MAX || w < INT32_MIN || h > INT32_MAX || h < INT32_MIN) return RT_ERR_INVALID_ARG;
    if (s == 1) {
        if (out != cam) std::memcpy(out, cam, sizeof *out);
        return RT_OK;
    }
    rt_camera v = *cam;
    const double S = (double)s, hh = (S - 1.0) * 0.5;
    for (int k = 0; k < 3; k++) {
        const double dxs = cam->pixel_delta_x[k] / S, dys = cam->pixel_delta_y[k] / S;
        v.image_top_left[k] = (cam->image_top_left[k] - dxs * hh) - dys * hh;
        v.pixel_delta_x[k] = dxs;
        v.pixel_delta_y[k] = dys;
    }
    v.width = (int32_t)w;
    v.height = (int32_t)h;
    *out = v;
    return RT_OK;
}

int virt_frame(int ss_log2, const rt_camera* cam, int32_t row0, int32_t nrows, VirtFrame& v) {
    v.cam = cam;
    v.row0 = row0;
    v.nrows = nrows;
    if (!ss_log2) return RT_OK;
    const int st = supersample_camera(cam, 1 << ss_log2, &v.vcam);
    if (st != RT_OK) return st;
    v.cam = &v.vcam;
    v.row0 = row0 << ss_log2;   // <= height * S, which fits (checked above)
    v.nrows = nrows << ss_log2;
    return RT_OK;
}

namespace {

/* ---- primary-ray tile bins (rt_device.h PrimBox) -------------------------------------
 * A point X = o + u*d(x, i) of a primary ray has (u, u*x, u*i) = M^-1 (X - o) with
 * M = [o - TL, -dx, -dy] (columns), d(x, i) = o - (TL + dx*x + dy*i) (main.cpp:132-133).
 * The box of a convex hull is the box of its projected vertices (the map is projective,
 * convexity-preserving on u > 0), floor/ceil'd and widened by one pixel.  Conditions
 * that make the box a proof (DESIGN.md §3 "tile bins"):
 *   - a primitive is only boxed when the camera is clearly off it (sphere: |o - C| >
 *     r*sqrt(3) + delta; wall: |num| = |(P - o).n| > 1e-9 * scale, below which rounding of
 *     a near-grazing ray's t could be arbitrary), otherwise it keeps every tile;
 *   - hull entirely at u < 0: the line meets it behind the camera only (t < 0), never;
 *   - wall polygon clipped to u >= eps = |num| / (2 max|d|): hits at u < eps would lie
 *     closer to o than the wall's plane, impossible;
 *   - a sphere hull straddling u = 0 keeps every tile.
 * Outside the box by >= 1 pixel the exact ray misses the hull by an angle of ~1 pixel
 * while the reference's rounding moves a hit by ~1e-13 pixel (both scale alike with the
 * grazing angle), so the reference's test rejects the primitive as well. */
struct Proj {
    double r[3][3];  // rows of M^-1
    double o[3];
};
inline double dot3(const double* a, const double* b) { return a[0] * b[0] + a[1] * b[1] + a[2] * b[2]; }
inline void cross3(const double* a, const double* b, double* c) {
    c[0] = a[1] * b[2] - a[2] * b[1];
    c[1] = a[2] * b[0] - a[0] * b[2];
    c[2] = a[0] * b[1] - a[1] * b[0];
}
bool make_proj(const rt_camera* cam, Proj& P) {
    double e[3], c1[3], c2[3];
    for (int k = 0; k < 3; k++) {
        P.o[k] = cam->position[k];
        e[k] = cam->position[k] - cam->image_top_left[k];
        c1[k] = -cam->pixel_delta_x[k];
        c2[k] = -cam->pixel_delta_y[k];
    }
    double x12[3], x20[3], x01[3];
    cross3(c1, c2, x12);
    cross3(c2, e, x20);
    cross3(e, c1, x01);
    const double det = dot3(e, x12);
    if (!(std::fabs(det) > 0) || !std::isfinite(det)) return false;
    for (int k = 0; k < 3; k++) {
        P.r[0][k] = x12[k] / det;
        P.r[1][k] = x20[k] / det;
        P.r[2][k] = x01[k] / det;
    }
    return true;
}
inline double proj_u(const Proj& P, const double* X) {
    const double v[3] = {X[0] - P.o[0], X[1] - P.o[1], X[2] - P.o[2]};
    return dot3(P.r[0], v);
}
struct BoxAcc {
    double x0 = INFINITY, x1 = -INFINITY, i0 = INFINITY, i1 = -INFINITY;
    bool bad = false;
    void add(const Proj& P, const double* X) {
        const double v[3] = {X[0] - P.o[0], X[1] - P.o[1], X[2] - P.o[2]};
        const double u = dot3(P.r[0], v);
        const double x = dot3(P.r[1], v) / u, i = dot3(P.r[2], v) / u;
        if (!std::isfinite(x) || !std::isfinite(i) || !(u > 0)) bad = true;
        x0 = std::fmin(x0, x);
        x1 = std::fmax(x1, x);
        i0 = std::fmin(i0, i);
        i1 = std::fmax(i1, i);
    }
};

/* Boxes of every primitive (material-slot order) for the camera P (origin P.o). */
void boxes_for(const SceneHost& sc, const Proj& P, double dmax, int32_t width, int32_t row0,
               int32_t nrows, rt::PrimBox* out, bool spheres = true) {
    const double W = width, R0 = row0, R1 = row0 + nrows - 1;
    const rt::PrimBox all{-1, (int16_t)width, (int16_t)(row0 - 1), (int16_t)(row0 + nrows)};
    const rt::PrimBox none{1, 0, 1, 0};
    auto to_box = [&](const BoxAcc& b) -> rt::PrimBox {
        if (b.bad) return all;
        const double x0 = std::floor(b.x0) - 1, x1 = std::ceil(b.x1) + 1;
        const double i0 = std::floor(b.i0) - 1, i1 = std::ceil(b.i1) + 1;
        if (x0 > W - 1 || x1 < 0 || i0 > R1 || i1 < R0) return none;
        return rt::PrimBox{(int16_t)std::fmax(x0, -1.0), (int16_t)std::fmin(x1, W),
                           (int16_t)std::fmax(i0, R0 - 1), (int16_t)std::fmin(i1, R1 + 1)};
    };
    const double* o = P.o;
    const double oabs = std::fabs(o[0]) + std::fabs(o[1]) + std::fabs(o[2]);
    // Exact x (and i) extent of the ball: the pixels with p/u = x form the plane
    // (b - x a).(X - o) = 0 through o (a, b, c = rows of M^-1), and it meets the ball
    // |X - C| <= r iff |(b - x a).(C - o)| <= r |b - x a|, i.e. x lies between the roots of
    // (uc^2 - r^2 |a|^2) x^2 - 2 (pc uc - r^2 a.b) x + (pc^2 - r^2 |b|^2) = 0 (the ball wholly
    // in front, u0 > 0, makes the leading coefficient positive).  Rounding is covered by the
    // one-pixel widening of to_box, as for the other hulls.
    const double aa = dot3(P.r[0], P.r[0]), ab = dot3(P.r[0], P.r[1]), ac = dot3(P.r[0], P.r[2]),
                 bb = dot3(P.r[1], P.r[1]), cc = dot3(P.r[2], P.r[2]);
    const double na = std::sqrt(aa);
    for (int s = 0; s < (spheres ? sc.nS : 0); s++) {
        const double* S = &sc.h_sph[5 * s];
        const double r = S[4];
        const double v[3] = {S[0] - o[0], S[1] - o[1], S[2] - o[2]};
        const double delta = 1e-6 * (1 + oabs + std::fabs(S[0]) + std::fabs(S[1]) + std::fabs(S[2]) + r);
        rt::PrimBox b = all;
        if (std::sqrt(dot3(v, v)) > r * 1.7320508075688772 + delta && r > 1e-9 * std::sqrt(dot3(v, v))) {
            const double uc = dot3(P.r[0], v), pc = dot3(P.r[1], v), qc = dot3(P.r[2], v);
            const double u0 = uc - r * na, u1 = uc + r * na;
            if (u1 < 0) {
                b = none;
            } else if (u0 > 0) {
                const double r2 = r * r;
                const double A = uc * uc - r2 * aa;
                const double Bx = pc * uc - r2 * ab, Cx = pc * pc - r2 * bb;
                const double By = qc * uc - r2 * ac, Cy = qc * qc - r2 * cc;
                const double sx = std::sqrt(std::fmax(0.0, Bx * Bx - A * Cx));
                const double sy = std::sqrt(std::fmax(0.0, By * By - A * Cy));
                BoxAcc acc;
                acc.x0 = (Bx - sx) / A;
                acc.x1 = (Bx + sx) / A;
                acc.i0 = (By - sy) / A;
                acc.i1 = (By + sy) / A;
                acc.bad = !(A > 0) || !std::isfinite(acc.x0) || !std::isfinite(acc.x1) ||
                          !std::isfinite(acc.i0) || !std::isfinite(acc.i1);
                b = to_box(acc);
            }
        }
        out[s] = b;
    }
    for (int w = 0; w < sc.nW; w++) {
        const double* Wd = &sc.h_wal[14 * w];
        const double *Pw = Wd, *n = Wd + 3, *X = Wd + 6, *Y = Wd + 9;
        const double len = Wd[12], wid = Wd[13];
        const double pv[3] = {Pw[0] - o[0], Pw[1] - o[1], Pw[2] - o[2]};
        const double num = dot3(pv, n);
        const double scale = 1 + oabs + std::fabs(Pw[0]) + std::fabs(Pw[1]) + std::fabs(Pw[2]) + len + wid;
        rt::PrimBox b = all;
        if (std::fabs(num) > 1e-9 * scale && dmax > 0) {
            double V[4][3];  // P, P + len X, P + len X + wid Y, P + wid Y (cyclic)
            for (int k = 0; k < 3; k++) {
                V[0][k] = Pw[k];
                V[1][k] = Pw[k] + X[k] * len;
                V[2][k] = Pw[k] + X[k] * len + Y[k] * wid;
                V[3][k] = Pw[k] + Y[k] * wid;
            }
            double u[4], umax = -INFINITY;
            for (int c = 0; c < 4; c++) {
                u[c] = proj_u(P, V[c]);
                umax = std::fmax(umax, u[c]);
            }
            const double eps = 0.5 * std::fabs(num) / dmax;
            if (umax < eps) {
                b = none;  // every point behind the camera or closer than the wall's plane
            } else {
                BoxAcc acc;  // Sutherland-Hodgman against u >= eps
                for (int c = 0; c < 4; c++) {
                    const int c2 = (c + 1) & 3;
                    if (u[c] >= eps) acc.add(P, V[c]);
                    if ((u[c] >= eps) != (u[c2] >= eps)) {
                        const double t = (eps - u[c]) / (u[c2] - u[c]);
                        double Xc[3];
                        for (int k = 0; k < 3; k++) Xc[k] = V[c][k] + (V[c2][k] - V[c][k]) * t;
                        acc.add(P, Xc);
                    }
                }
                b = to_box(acc);
            }
        }
        out[sc.nS + w] = b;
    }
}

}  // namespace

void frame_boxes(const SceneHost& sc, const FrameOptions& opt, const rt_camera* cam, int32_t row0,
                 int32_t nrows, rt::KParams& p) {
    p.nbox = 0;
    p.nwbox = 0;
    p.mir_depth = 0;
    const int np = sc.nS + sc.nW;
    const bool cull_walls = p.wave_cull && sc.nW > 0 && sc.nW < rt::BIN_MAX_PRIMS;
    if (!opt.tile_bins || (p.wave_cull && !cull_walls) || np == 0 ||
        (!p.wave_cull && np > rt::BIN_MAX_PRIMS) || cam->width > 32000 || cam->height > 32000 ||
        nrows <= 0 || cam->width <= 0)
        return;
    Proj P;
    if (!make_proj(cam, P)) return;
    // largest |d| over the frame: d is affine in (x, i), so at a corner of the pixel grid
    double dmax = 0;
    for (int c = 0; c < 4; c++) {
        const double x = (c & 1) ? cam->width - 1 : 0, i = (c & 2) ? row0 + nrows - 1 : row0;
        double d[3];
        for (int k = 0; k < 3; k++)
            d[k] = cam->position[k] -
                   (cam->image_top_left[k] + cam->pixel_delta_x[k] * x + cam->pixel_delta_y[k] * i);
        dmax = std::fmax(dmax, std::sqrt(dot3(d, d)));
    }
    if (!(dmax > 0) || !std::isfinite(dmax)) return;
    if (p.wave_cull) {
        // scenes with the wave cull: the spheres keep the cone, the walls get boxes (box[w])
        std::vector<rt::PrimBox> all(np);
        boxes_for(sc, P, dmax, cam->width, row0, nrows, all.data(), false);
        for (int w = 0; w < sc.nW; w++) p.box[w] = all[sc.nS + w];
        p.nwbox = sc.nW;
        return;
    }
    boxes_for(sc, P, dmax, cam->width, row0, nrows, p.box);
    p.nbox = np;
    // dispatch order (rt_frame_dev.h tile_row): centre-out from the weighted median tile row
    // of the boxes' coverage, reflective primitives weighted up (their tiles bounce)
    if (opt.row_order) {
        const int nty = (nrows + 7) / 8;
        std::vector<double> prof(nty, 0.0);
        for (int j = 0; j < np; j++) {
            const rt::PrimBox& b = p.box[j];
            const int x0 = std::max<int>(b.x0, 0), x1 = std::min<int>(b.x1, cam->width - 1);
            const int i0 = std::max<int>(b.i0, row0), i1 = std::min<int>(b.i1, row0 + nrows - 1);
            if (x0 > x1 || i0 > i1) continue;
            const double wgt = (1.0 + 3.0 * sc.h_km[j]) * (x1 - x0 + 1);
            for (int t = (i0 - row0) / 8; t <= (i1 - row0) / 8; t++) prof[t] += wgt;
        }
        double tot = 0;
        for (double v : prof) tot += v;
        double acc = 0;
        for (int t = 0; t < nty && tot > 0; t++) {
            acc += prof[t];
            if (acc >= 0.5 * tot) {
                p.row_center = t;
                break;
            }
        }
    }
    // mirror bins (rt_device.h): cameras mirrored along wall chains, each reflection
    // shifted by the reference's 1e-4 * normal origin offset (main.cpp:111); rows of
    // (R M)^-1 = R * rows of M^-1.  Reflected directions are unit vectors, not the d's,
    // but |R d| = |d| keeps dmax.  Only chains some tile can follow are computed (their
    // "reach" — the intersection of the boxes along the chain, widened by a tile — is
    // non-empty); every other sequence keeps all primitives.
    const int nW = sc.nW;
    int depth = 0;
    for (long tot = 0, lvl = 1; depth < rt::MIR_MAX_DEPTH && nW > 0; depth++) {
        lvl *= nW;
        tot += lvl * np;
        if (tot > rt::MIR_MAX_BOXES) break;
    }
    if (!opt.mirror_bins || depth == 0) return;
    struct Node {
        Proj cam;
        rt::PrimBox reach;  // pixel region (incl. a tile of slack) where the chain can occur
    };
    const rt::PrimBox allb{-1, (int16_t)cam->width, (int16_t)(row0 - 1), (int16_t)(row0 + nrows)};
    auto meet = [](const rt::PrimBox& a, const rt::PrimBox& b) {
        rt::PrimBox r{std::max(a.x0, b.x0), std::min(a.x1, b.x1), std::max(a.i0, b.i0),
                      std::min(a.i1, b.i1)};
        return r;
    };
    auto empty = [](const rt::PrimBox& b) { return b.x0 > b.x1 || b.i0 > b.i1; };
    auto widen = [](rt::PrimBox b) {
        if (b.x0 > b.x1 || b.i0 > b.i1) return b;
        b.x0 = (int16_t)(b.x0 - 8);
        b.x1 = (int16_t)(b.x1 + 8);
        b.i0 = (int16_t)(b.i0 - 8);
        b.i1 = (int16_t)(b.i1 + 8);
        return b;
    };
    std::vector<Node> prev(1), cur;  // level 0: the camera itself, reach = the frame
    prev[0].cam = P;
    prev[0].reach = allb;
    std::vector<const rt::PrimBox*> prev_boxes(1, p.box);
    int off = 0;
    for (int L = 1; L <= depth; L++) {
        cur.assign(prev.size() * nW, Node{});
        std::vector<const rt::PrimBox*> cur_boxes(cur.size(), nullptr);
        for (size_t q0 = 0; q0 < prev.size(); q0++) {
            for (int w = 0; w < nW; w++) {
                const size_t q = q0 * nW + w;
                rt::PrimBox* out = p.mbox + (size_t)(off + q) * np;
                Node& nd = cur[q];
                nd.reach = empty(prev[q0].reach) ? prev[q0].reach
                                                 : meet(prev[q0].reach, widen(prev_boxes[q0][sc.nS + w]));
                if (empty(nd.reach)) {
                    for (int j = 0; j < np; j++) out[j] = allb;  // never followed: keep all
                    continue;
                }
                const double* Wd = &sc.h_wal[14 * w];
                const double *Pw = Wd, *n = Wd + 3;
                const Proj& pc = prev[q0].cam;
                const double op[3] = {pc.o[0] - Pw[0], pc.o[1] - Pw[1], pc.o[2] - Pw[2]};
                const double h = dot3(op, n);
                for (int k = 0; k < 3; k++) nd.cam.o[k] = (pc.o[k] - 2 * h * n[k]) + 1e-4 * n[k];
                for (int j = 0; j < 3; j++) {
                    const double rn = dot3(pc.r[j], n);
                    for (int k = 0; k < 3; k++) nd.cam.r[j][k] = pc.r[j][k] - 2 * rn * n[k];
                }
                boxes_for(sc, nd.cam, dmax, cam->width, row0, nrows, out);
                cur_boxes[q] = out;
            }
        }
        off += (int)cur.size();
        prev.swap(cur);
        prev_boxes.swap(cur_boxes);
    }
    p.mir_depth = depth;
}

void scene_params(const FrameScene& fs, int32_t precision, rt::KParams& p) {
    const SceneHost& sc = fs.sc;
    const char* base = static_cast<const char*>(fs.base);
    // section `off` of the device scene (null without one: rt_frame_boxes' host-only use)
    auto at = [base](size_t off) -> const char* { return base ? base + off : nullptr; };
    p.s32 = reinterpret_cast<const rt::SphG32*>(base);
    p.s64 = reinterpret_cast<const rt::SphG64*>(at(sc.off_s64));
    p.w32 = reinterpret_cast<const rt::Wall32*>(at(sc.off_w32));
    p.w64 = reinterpret_cast<const rt::Wall64*>(at(sc.off_w64));
    p.sph_j = reinterpret_cast<const int32_t*>(at(sc.off_sj));
    p.wall_j = reinterpret_cast<const int32_t*>(at(sc.off_wj));
    p.mat = reinterpret_cast<const rt::DevMat*>(at(sc.off_mat));
    p.mat32 = reinterpret_cast<const rt::DevMat32*>(at(sc.off_mat32));
    p.wnn = reinterpret_cast<const double(*)[4]>(at(sc.off_wnn));
    const auto& cs = sc.cset[precision == RT_PREC_F32 ? 0 : 1];
    p.clu = reinterpret_cast<const rt::Clu32*>(at(cs.off_clu));
    p.csph = reinterpret_cast<const rt::CluSph*>(at(cs.off_csph));
    p.cord = reinterpret_cast<const uint8_t*>(at(cs.off_cord));
    p.nclu = cs.nclu;
    p.clu_ls = cs.ls;
    p.clu_axis = cs.clu_axis;
    p.clu_cos = fs.opt.clu_cos;
    p.clu_oinf = cs.clu_oinf;
    p.nS = sc.nS;
    p.nW = sc.nW;
    p.int_exp = sc.int_exp ? 1 : 0;
    p.wave_cull = sc.nS >= fs.opt.wave_cull_min ? 1 : 0;
}

rt::KParams make_params(const FrameScene& fs, BoxCache* bc, const rt_camera* cam, int32_t row0,
                        int32_t nrows, const FrameReq& rq, void* d_out, unsigned long long* d_segs) {
    const SceneHost& sc = fs.sc;
    const FrameOptions& opt = fs.opt;
    rt::KParams p{};
    scene_params(fs, rq.precision, p);
    p.ss_log2 = opt.ss_log2;  // cam, row0, nrows: the S-times larger frame's (virt_frame)
    p.W = cam->width;
    p.row0 = row0;
    p.nrows = nrows;
    p.depth = rq.depth;
    // (the host-internal bit is never the caller's: other flag bits stay ignored)
    p.flags = (rq.flags & ~(rt::FLAG_LIGHTS | rt::FLAG_GLASS)) | (opt.lights ? rt::FLAG_LIGHTS : 0u) |
              (opt.glass ? rt::FLAG_GLASS : 0u);
    p.outf = rq.out_format;
    for (int k = 0; k < 3; k++) {
        p.pos[k] = cam->position[k];
        p.tl[k] = cam->image_top_left[k];
        p.dx[k] = cam->pixel_delta_x[k];
        p.dy[k] = cam->pixel_delta_y[k];
    }
    p.out = d_out;
    p.segs = d_segs;
    // (one sample per lane when resolving; no two-pixel shadow kernels)
    p.pairs = (opt.pixel_pairs && !opt.ss_log2 && !(rq.flags & RT_FLAG_SHADOWS) && !opt.lights && !opt.glass) ? 1 : 0;
    p.stats = opt.d_stats;
    // eye tables (rt_device.h) for the linear-scan kernels: the same fp64 operations, in
    // the same order, as sphere_exact / wall_exact on a ray starting at cam->position
    p.eye = (opt.eye_tables && !p.wave_cull && sc.nS <= rt::EYE_MAX_S && sc.nW <= rt::EYE_MAX_W) ? 1 : 0;
    if (p.eye) {
        const double* o = cam->position;
        for (int s = 0; s < sc.nS; s++) {
            const double* S = &sc.h_sph[5 * s];
            const double ox = o[0] - S[0], oy = o[1] - S[1], oz = o[2] - S[2];  // scene.cpp:45
            const double c = (ox * ox + oy * oy + oz * oz) - S[3];              // scene.cpp:51
            const double e[4] = {ox, oy, oz, c};
            for (int k = 0; k < 4; k++) p.eye_s[s][k] = e[k];
        }
        for (int w = 0; w < sc.nW; w++) {
            const double* P = &sc.h_wal[14 * w];
            const double* n = P + 3;
            p.eye_w[w] = (P[0] - o[0]) * n[0] + (P[1] - o[1]) * n[1] + (P[2] - o[2]) * n[2];  // scene.cpp:10
        }
    }
    // primary scan's wall order: nearest rectangle to the camera first, so the wall t-skip
    // (t > best) drops the bounds test of the walls it occludes.  Any order gives the
    // reference's winner (wall ties compare scene indices, rt_scan_dev.h wall_exact).
    p.wall_order_n = 0;
    p.wall_order = 0;
    if (opt.wall_order && sc.nW > 1 && sc.nW <= 16) {
        const double* o = cam->position;
        double key[16];
        int ord[16];
        for (int w = 0; w < sc.nW; w++) {
            const double* Wd = &sc.h_wal[14 * w];
            const double *Pw = Wd, *X = Wd + 6, *Y = Wd + 9;
            const double v[3] = {o[0] - Pw[0], o[1] - Pw[1], o[2] - Pw[2]};
            // closest point of the rectangle P + a X + b Y (a in [0, len], b in [0, wid])
            const double a = std::min(std::max(v[0] * X[0] + v[1] * X[1] + v[2] * X[2], 0.0), Wd[12]);
            const double b = std::min(std::max(v[0] * Y[0] + v[1] * Y[1] + v[2] * Y[2], 0.0), Wd[13]);
            double d2 = 0.0;
            for (int k = 0; k < 3; k++) {
                const double e = v[k] - a * X[k] - b * Y[k];
                d2 += e * e;
            }
            key[w] = std::isnan(d2) ? 1e300 : d2;
            ord[w] = w;
        }
        std::stable_sort(ord, ord + sc.nW, [&](int x, int y) { return key[x] < key[y]; });
        for (int k = 0; k < sc.nW; k++) p.wall_order |= (uint64_t)ord[k] << (4 * k);
        p.wall_order_n = sc.nW;
    }
    // per-frame boxes, or the previous render's when its inputs were the same
    // (transmission records: no mirror chains — a ray that passed a pane did not reflect off it)
    FrameOptions bopt = opt;
    if (opt.glass) bopt.mirror_bins = false;
    const int32_t opts = (bopt.tile_bins ? 1 : 0) | (bopt.row_order ? 2 : 0) | (bopt.mirror_bins ? 4 : 0);
    if (bc && opt.box_cache_on && bc->valid && bc->scene_gen == fs.scene_gen && bc->row0 == row0 &&
        bc->nrows == nrows && bc->wave_cull == p.wave_cull && bc->opts == opts &&
        std::memcmp(&bc->cam, cam, sizeof(rt_camera)) == 0) {
        p.nbox = bc->nbox;
        p.nwbox = bc->nwbox;
        p.row_center = bc->row_center;
        p.mir_depth = bc->mir_depth;
        std::memcpy(p.box, bc->box, sizeof p.box);
        std::memcpy(p.mbox, bc->mbox, bc->nmbox * sizeof(rt::PrimBox));
        return p;
    }
    frame_boxes(sc, bopt, cam, row0, nrows, p);
    if (!bc) return p;
    long nm = 0;
    for (long L = 1, lvl = 1; L <= p.mir_depth; L++) {
        lvl *= sc.nW;
        nm += lvl * p.nbox;
    }
    bc->valid = true;
    bc->scene_gen = fs.scene_gen;
    bc->cam = *cam;
    bc->row0 = row0;
    bc->nrows = nrows;
    bc->wave_cull = p.wave_cull;
    bc->opts = opts;
    bc->nbox = p.nbox;
    bc->nwbox = p.nwbox;
    bc->row_center = p.row_center;
    bc->mir_depth = p.mir_depth;
    bc->nmbox = (size_t)nm;
    std::memcpy(bc->box, p.box, sizeof p.box);
    std::memcpy(bc->mbox, p.mbox, bc->nmbox * sizeof(rt::PrimBox));
    return p;
}

}  // namespace rth
