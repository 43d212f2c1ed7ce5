/*
 * rt_scene_pack.cpp — rt_set_scene's host half (pure host: no HIP, no rt_ctx): the device
 * image of a scene in the layout of rt_device.h, its sphere clusters, and the host copies
 * the per-frame arguments (rt_frame_args.cpp) read.
 */
#include <algorithm>
#include <array>
#include <cmath>
#include <functional>
#include <vector>

#include "rt_host.h"

namespace rth __attribute__((visibility("hidden"))) {

namespace {

bool hnan(hv3 v) { return std::isnan(v.x) || std::isnan(v.y) || std::isnan(v.z); }

size_t align_up(size_t v, size_t a) { return (v + a - 1) / a * a; }

}  // namespace

int pack_scene(const rt_prim* prims, int32_t n, SceneHost& sc) {
    if (n < 0 || (n > 0 && !prims)) return RT_ERR_INVALID_ARG;
    struct Sph {
        double c[3], r;
        int32_t j;
    };
    struct Wal {
        double P[3], n[3], X[3], Y[3], len, wid;
        int32_t j;
    };
    std::vector<Sph> sph;
    std::vector<Wal> wal;
    for (int32_t j = 0; j < n; j++) {
        const rt_prim& q = prims[j];
        if (q.reserved != 0) return RT_ERR_INVALID_ARG;
        if (q.kind == RT_PRIM_SPHERE) {
            sph.push_back(Sph{{q.position[0], q.position[1], q.position[2]}, q.radius, j});
        } else if (q.kind == RT_PRIM_WALL) {
            const hv3 nrm{q.normal[0], q.normal[1], q.normal[2]};
            const hv3 X = hnormalize(hcross(nrm, hv3{0, 0, 1}));  // scene.cpp:18
            const hv3 Y = hnormalize(hcross(X, nrm));             // scene.cpp:19
            // A NaN basis (normal parallel to z) or NaN normal makes every projection NaN:
            // the reference can never report a hit for this wall, so it is not uploaded.
            if (hnan(X) || hnan(Y) || hnan(nrm)) continue;
            wal.push_back(Wal{{q.position[0], q.position[1], q.position[2]},
                              {nrm.x, nrm.y, nrm.z}, {X.x, X.y, X.z}, {Y.x, Y.y, Y.z},
                              q.length, q.width, j});
        } else {
            return RT_ERR_INVALID_ARG;
        }
    }
    const size_t nS = sph.size(), nW = wal.size(), ng = (nS + 3) / 4;
    const size_t off_s64 = align_up(ng * sizeof(rt::SphG32), 256);
    const size_t off_w32 = align_up(off_s64 + ng * sizeof(rt::SphG64), 256);
    const size_t off_w64 = align_up(off_w32 + nW * sizeof(rt::Wall32), 256);
    const size_t off_sj = align_up(off_w64 + nW * sizeof(rt::Wall64), 256);
    const size_t off_wj = align_up(off_sj + nS * sizeof(int32_t), 256);
    const size_t off_mat = align_up(off_wj + nW * sizeof(int32_t), 256);
    const size_t off_mat32 = align_up(off_mat + (nS + nW) * sizeof(rt::DevMat), 256);
    const size_t off_wnn = align_up(off_mat32 + (nS + nW) * sizeof(rt::DevMat32), 256);
    auto make_leaves = [&](int ls, std::vector<std::vector<int>>& leaves, int& clu_axis) {
        // sphere clusters (rt_device.h): leaves of <= ls spheres from binary splits at the
        // surface-area cut at a multiple of ls
        if (nS >= 2 * (size_t)ls && nS <= (size_t)ls * rt::CLU_MAX) {
            std::vector<int> all(nS);
            for (size_t s = 0; s < nS; s++) all[s] = (int)s;
            bool finite = true;
            for (const Sph& a : sph)
                finite = finite && std::isfinite(a.c[0]) && std::isfinite(a.c[1]) &&
                         std::isfinite(a.c[2]) && std::isfinite(a.r);
            std::function<void(std::vector<int>&, bool)> split = [&](std::vector<int>& ids, bool top) {
                if (ids.size() <= (size_t)ls) {
                    leaves.push_back(ids);
                    return;
                }
                // (the median of the centres' widest axis where no cut has a finite cost)
                double lo[3] = {HUGE_VAL, HUGE_VAL, HUGE_VAL}, hi[3] = {-HUGE_VAL, -HUGE_VAL, -HUGE_VAL};
                for (int i : ids)
                    for (int q = 0; q < 3; q++) {
                        lo[q] = std::min(lo[q], sph[i].c[q]);
                        hi[q] = std::max(hi[q], sph[i].c[q]);
                    }
                int ax = 0;
                for (int q = 1; q < 3; q++)
                    if (hi[q] - lo[q] > hi[ax] - lo[ax]) ax = q;
                size_t mid = ids.size() / 2;
                // surface-area split: over the three axes and the cut positions that keep the
                // leaf count at its minimum (multiples of CLU_SIZE), the one minimising
                // area(left box) * |left| + area(right box) * |right| (boxes of the balls)
                const size_t n = ids.size();
                double best = HUGE_VAL;
                for (int q = 0; q < 3; q++) {
                    std::vector<int> v(ids);
                    std::sort(v.begin(), v.end(), [&](int a, int b) {
                        return sph[a].c[q] < sph[b].c[q] || (sph[a].c[q] == sph[b].c[q] && a < b);
                    });
                    auto area = [&](size_t b0, size_t b1) {
                        double l[3] = {HUGE_VAL, HUGE_VAL, HUGE_VAL}, h[3] = {-HUGE_VAL, -HUGE_VAL, -HUGE_VAL};
                        for (size_t k = b0; k < b1; k++)
                            for (int z = 0; z < 3; z++) {
                                const double rr = std::fabs(sph[v[k]].r);
                                l[z] = std::min(l[z], sph[v[k]].c[z] - rr);
                                h[z] = std::max(h[z], sph[v[k]].c[z] + rr);
                            }
                        const double e0 = h[0] - l[0], e1 = h[1] - l[1], e2 = h[2] - l[2];
                        return 2 * (e0 * e1 + e1 * e2 + e2 * e0);
                    };
                    for (size_t k = (size_t)ls; k < n; k += (size_t)ls) {
                        const double c = area(0, k) * (double)k + area(k, n) * (double)(n - k);
                        if (c < best) {
                            best = c;
                            ax = q;
                            mid = k;
                        }
                    }
                }
                if (top) clu_axis = ax;
                std::nth_element(ids.begin(), ids.begin() + mid, ids.end(), [&](int a, int b) {
                    return sph[a].c[ax] < sph[b].c[ax] || (sph[a].c[ax] == sph[b].c[ax] && a < b);
                });
                std::vector<int> l(ids.begin(), ids.begin() + mid), r(ids.begin() + mid, ids.end());
                split(l, false);
                split(r, false);
            };
            if (finite) split(all, true);
            if (leaves.size() > (size_t)rt::CLU_MAX) leaves.clear();
        }
    };
    // set 0: the F32 kernels' leaves (CLU_SIZE); set 1: the fp64 kernels' (CLU_SIZE_D, or
    // CLU_SIZE when that needs more than CLU_MAX leaves)
    std::vector<std::vector<int>> leaves[2];
    int clu_axis[2] = {0, 0}, lsz[2] = {rt::CLU_SIZE, rt::CLU_SIZE_D};
    make_leaves(lsz[0], leaves[0], clu_axis[0]);
    make_leaves(lsz[1], leaves[1], clu_axis[1]);
    if (leaves[1].empty() && lsz[1] != lsz[0]) {
        leaves[1] = leaves[0];
        clu_axis[1] = clu_axis[0];
        lsz[1] = lsz[0];
    }
    size_t off = align_up(off_wnn + nW * 4 * sizeof(double), 256);
    for (int q = 0; q < 2; q++) {
        auto& cs = sc.cset[q];
        const size_t nclu = leaves[q].size();
        cs.nclu = (int)nclu;
        cs.clu_axis = clu_axis[q];
        cs.ls = lsz[q];
        cs.off_clu = off;
        // room for a multiple of four cluster records (the kernels read the boxes in batches)
        cs.off_csph = align_up(cs.off_clu + ((nclu + 3) & ~(size_t)3) * sizeof(rt::Clu32), 256);
        cs.off_cord = align_up(cs.off_csph + nclu * lsz[q] * sizeof(rt::CluSph), 256);
        off = align_up(cs.off_cord + 8 * rt::CLU_MAX, 256);
    }
    const size_t total = off + 256;
    sc.blocks.assign((total + 255) / 256, {});
    sc.total = total;
    char* const host = sc.image();
    auto* s32 = reinterpret_cast<rt::SphG32*>(host);
    auto* s64 = reinterpret_cast<rt::SphG64*>(host + off_s64);
    auto* w32 = reinterpret_cast<rt::Wall32*>(host + off_w32);
    auto* w64 = reinterpret_cast<rt::Wall64*>(host + off_w64);
    auto* sj = reinterpret_cast<int32_t*>(host + off_sj);
    auto* wj = reinterpret_cast<int32_t*>(host + off_wj);
    auto* mat = reinterpret_cast<rt::DevMat*>(host + off_mat);
    auto* mat32 = reinterpret_cast<rt::DevMat32*>(host + off_mat32);
    auto* wnn = reinterpret_cast<double(*)[4]>(host + off_wnn);
    auto put_mat = [&](size_t slot, const rt_material& m) {
        rt::DevMat& d = mat[slot];
        for (int k = 0; k < 3; k++) d.color[k] = m.color[k];
        d.ka = m.ambient;
        d.km = m.metallic;
        d.kd = m.diffuse;
        d.ks = m.specular;
        d.ex = m.specular_exponent;
        rt::DevMat32& f = mat32[slot];
        for (int k = 0; k < 3; k++) f.color[k] = (float)m.color[k];
        f.ka = (float)m.ambient;
        f.km = (float)m.metallic;
        f.kd = (float)m.diffuse;
        f.ks = (float)m.specular;
        f.ex = (float)m.specular_exponent;
    };
    for (size_t s = 0; s < nS; s++) {
        rt::SphG32& g = s32[s / 4];
        double* d = s64[s / 4].v[s % 4];
        for (int k = 0; k < 3; k++) {
            g.c[k][s % 4] = (float)sph[s].c[k];
            d[k] = sph[s].c[k];
        }
        g.c[3][s % 4] = (float)sph[s].r;
        d[3] = sph[s].r * sph[s].r;  // scene.cpp:51
        sj[s] = sph[s].j;
        put_mat(s, prims[sph[s].j].mat);
    }
    for (int set = 0; set < 2; set++) {
        auto& cset = sc.cset[set];
        const size_t nclu = (size_t)cset.nclu, ls = (size_t)cset.ls;
        const std::vector<std::vector<int>>& lv = leaves[set];
        auto* clu = reinterpret_cast<rt::Clu32*>(host + cset.off_clu);
        auto* csph = reinterpret_cast<rt::CluSph*>(host + cset.off_csph);
        double clu_scale = 1.0;
        std::vector<std::array<double, 3>> cen(nclu);
        for (size_t c = 0; c < nclu; c++) {
            double lo[3] = {HUGE_VAL, HUGE_VAL, HUGE_VAL}, hi[3] = {-HUGE_VAL, -HUGE_VAL, -HUGE_VAL};
            double scale = 1.0;
            for (size_t k = 0; k < ls; k++) {
                rt::CluSph& cs = csph[c * ls + k];
                cs.slot = -1;
                if (k >= lv[c].size()) continue;
                const int si = lv[c][k];
                for (int q = 0; q < 4; q++) cs.c[q] = s64[si / 4].v[si % 4][q];
                for (int q = 0; q < 4; q++) cs.f[q] = s32[si / 4].c[q][si % 4];
                cs.slot = si;
                for (int q = 0; q < 3; q++) {
                    const double rr = std::fabs(sph[si].r);
                    lo[q] = std::min(lo[q], sph[si].c[q] - rr);
                    hi[q] = std::max(hi[q], sph[si].c[q] + rr);
                    scale = std::max(scale, std::fabs(sph[si].c[q]) + rr);
                }
            }
            // margin: far above the fp32 rounding of the box, the ray and the slab arithmetic
            // (~1e-6 relative), so a ray the exact test finds hitting a ball enters the box
            const double m = 1e-3 * scale;
            clu_scale = std::max(clu_scale, scale);
            for (int q = 0; q < 3; q++) cen[c][q] = 0.5 * (lo[q] + hi[q]);
            for (int q = 0; q < 3; q++) {
                clu[c].lo[q] = (float)(lo[q] - m);
                clu[c].hi[q] = (float)(hi[q] + m);
            }
        }
        // near-to-far cluster order per direction octant: by the box centre along the octant's
        // diagonal (any order is exact; this one lets the lanes' pruning start from near hits)
        auto* cord = reinterpret_cast<uint8_t*>(host + cset.off_cord);
        for (int o = 0; o < 8 && nclu > 0; o++) {
            const double sx = (o & 1) ? -1.0 : 1.0, sy = (o & 2) ? -1.0 : 1.0, sz = (o & 4) ? -1.0 : 1.0;
            std::vector<int> ord(nclu);
            for (size_t c = 0; c < nclu; c++) ord[c] = (int)c;
            std::stable_sort(ord.begin(), ord.end(), [&](int a, int b) {
                return sx * cen[a][0] + sy * cen[a][1] + sz * cen[a][2] <
                       sx * cen[b][0] + sy * cen[b][1] + sz * cen[b][2];
            });
            for (size_t k = 0; k < nclu; k++) {
                cord[o * rt::CLU_MAX + k] = (uint8_t)ord[k];
                clu[ord[k]].rank[o] = (uint8_t)k;
            }
        }
        // origins up to 100x the scene's extent: fp32 errors of the slab test ~1e-5 x scale,
        // 100x below the box margin
        cset.clu_oinf = (float)(100.0 * clu_scale);
    }
    for (size_t w = 0; w < nW; w++) {
        const Wal& a = wal[w];
        for (int k = 0; k < 3; k++) {
            w64[w].P[k] = a.P[k];
            w64[w].n[k] = a.n[k];
            w64[w].X[k] = a.X[k];
            w64[w].Y[k] = a.Y[k];
            w32[w].P[k] = (float)a.P[k];
            w32[w].n[k] = (float)a.n[k];
            w32[w].X[k] = (float)a.X[k];
            w32[w].Y[k] = (float)a.Y[k];
        }
        w64[w].len = a.len;
        w64[w].wid = a.wid;
        w32[w].len = (float)a.len;
        w32[w].wid = (float)a.wid;
        wj[w] = a.j;
        put_mat(nS + w, prims[a.j].mat);
        const hv3 nn = hnormalize(hv3{a.n[0], a.n[1], a.n[2]});  // N.normalize(), vec.cpp:21
        wnn[w][0] = nn.x;
        wnn[w][1] = nn.y;
        wnn[w][2] = nn.z;
    }

    sc.nS = (int)nS;
    sc.nW = (int)nW;
    sc.nP = n;
    sc.int_exp = true;
    for (size_t k = 0; k < nS + nW; k++) {
        const double e = mat[k].ex;
        if (!(e >= 0.0 && e <= 1024.0 && e == std::floor(e))) sc.int_exp = false;
    }
    sc.h_km.assign(nS + nW, 0.0);
    for (size_t k = 0; k < nS + nW; k++) sc.h_km[k] = mat[k].km;
    sc.h_sph.assign(5 * nS, 0.0);
    for (size_t s = 0; s < nS; s++) {
        for (int k = 0; k < 4; k++) sc.h_sph[5 * s + k] = s64[s / 4].v[s % 4][k];
        sc.h_sph[5 * s + 4] = sph[s].r;
    }
    sc.h_wal.assign(14 * nW, 0.0);
    for (size_t w = 0; w < nW; w++) {
        for (int k = 0; k < 3; k++) {
            sc.h_wal[14 * w + k] = w64[w].P[k];
            sc.h_wal[14 * w + 3 + k] = w64[w].n[k];
            sc.h_wal[14 * w + 6 + k] = w64[w].X[k];
            sc.h_wal[14 * w + 9 + k] = w64[w].Y[k];
        }
        sc.h_wal[14 * w + 12] = w64[w].len;
        sc.h_wal[14 * w + 13] = w64[w].wid;
    }
    sc.off_s64 = off_s64;
    sc.off_w32 = off_w32;
    sc.off_w64 = off_w64;
    sc.off_sj = off_sj;
    sc.off_wj = off_wj;
    sc.off_mat = off_mat;
    sc.off_mat32 = off_mat32;
    sc.off_wnn = off_wnn;
    return RT_OK;
}

int pack_lights(const rt_light* lights, int32_t n, rt::LightArgs& out) {
    static_assert(RT_MAX_LIGHTS == rt::MAX_LIGHTS, "the kernels' light table");
    if (n < 0 || n > RT_MAX_LIGHTS || (n > 0 && !lights)) return RT_ERR_INVALID_ARG;
    for (int32_t l = 0; l < n; l++)
        for (int k = 0; k < 3; k++)
            if (!std::isfinite(lights[l].position[k]) || !std::isfinite(lights[l].color[k]))
                return RT_ERR_INVALID_ARG;
    rt::LightArgs la{};
    for (int32_t l = 0; l < n; l++)
        for (int k = 0; k < 3; k++) {
            la.l[l].pos[k] = lights[l].position[k];
            la.l[l].col[k] = lights[l].color[k];
            la.l[l].colf[k] = (float)lights[l].color[k];
        }
    la.n = n;
    out = la;
    return RT_OK;
}

int pack_transmission(const rt_transmission* recs, int32_t n, SceneHost& sc, std::vector<rt::DevGlass>& out) {
    if ((n != 0 && n != sc.nP) || (n > 0 && !recs)) return RT_ERR_INVALID_ARG;
    bool any = false;
    for (int32_t j = 0; j < n; j++) {
        const double tau = recs[j].transmission, ior = recs[j].ior;
        if (!std::isfinite(tau) || !std::isfinite(ior)) return RT_ERR_INVALID_ARG;
        if (tau < 0.0 || tau > 1.0 || ior < 1.0 || ior > 4.0) return RT_ERR_INVALID_ARG;
        any = any || tau != 0.0;
    }
    std::vector<rt::DevGlass> tab;
    if (any) {
        // material-slot order: spheres, then walls, each with its scene index (pack_scene)
        const int32_t* sj = reinterpret_cast<const int32_t*>(sc.image() + sc.off_sj);
        const int32_t* wj = reinterpret_cast<const int32_t*>(sc.image() + sc.off_wj);
        tab.resize((size_t)sc.nS + (size_t)sc.nW);
        for (size_t k = 0; k < tab.size(); k++) {
            const rt_transmission& r = recs[k < (size_t)sc.nS ? sj[k] : wj[k - (size_t)sc.nS]];
            rt::DevGlass& g = tab[k];
            g.tau = r.transmission;
            g.ior = r.ior;
            g.w = r.transmission > 0.0 ? r.transmission : sc.h_km[k];
            g.wf = (float)g.w;
            g.pad = 0.0f;
        }
    }
    out.swap(tab);
    return RT_OK;
}

}  // namespace rth
