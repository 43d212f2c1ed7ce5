"""Expected radiance with transmission records (rt_set_transmission), shared by the test_glass_*
files.

lights_fixture.trace generalised by rt_capi.h's "Transmission" step: at an accepted hit on an
object whose tau > 0, with iterations remaining, the next ray is the one that passes through the
object and the unwind weighs with tau in metallic's place.  `local`, the light rays and the
fragility of their decisions are lights_fixture's; without lights the list is lights_fixture.ONE,
which gives the reference's bits.  The passage itself is numpy / `math` fp64 scalars, one IEEE
operation per written operation, dot products summed left to right:

    wall    f = dot(d, n); nf = -n if f > 0 else n; o' = pos - nf * .0001; d' = d
    sphere  P = o + d * projection   (occluded_fixture.sphere_projection: scene.cpp:75's point)
            refract in at P, follow the chord to Q, refract out (the header's formulas)

With every tau == 0 the result is lights_fixture.trace's bit for bit (test_glass_host.py).
"""
import ctypes as C
import functools
import math

import numpy as np

import lights_fixture as lfx
import occluded_fixture as ofx
import shadow_fixture as sfx
from rtamd import capi, scenes


def _dot(u, v):
    return u[0] * v[0] + u[1] * v[1] + u[2] * v[2]


def pane_step(pos, n, d):
    """-> (o', d') through a wall hit at pos (main.cpp:99) with the stored normal n."""
    f = _dot(d, n)
    nf = -n if f > 0 else n
    return pos - nf * .0001, d.copy()


def sphere_step(o, d, proj, c, ior):
    """-> (o', d', k2, ci) through the sphere of centre c entered at P = o + d * proj."""
    P = o + d * proj
    n = P - c
    dl = math.sqrt(_dot(d, d))
    dh = d / dl
    nl = math.sqrt(_dot(n, n))
    nh = n / nl
    ci = -_dot(dh, nh)
    eta = 1.0 / ior
    k = 1.0 - (eta * eta) * (1.0 - ci * ci)
    t = dh * eta + nh * (eta * ci - math.sqrt(k))
    m = c - P
    s = (2.0 * _dot(t, m)) / _dot(t, t)
    Q = P + t * s
    n2 = Q - c
    l2 = math.sqrt(_dot(n2, n2))
    n2h = n2 / l2
    tl = math.sqrt(_dot(t, t))
    th = t / tl
    c2 = _dot(th, n2h)
    k2 = 1.0 - (ior * ior) * (1.0 - c2 * c2)
    k2c = k2 if k2 > 0 else 0.0
    dn = th * ior + n2h * (math.sqrt(k2c) - ior * c2)
    return Q + n2 * .0001, dn, k2, ci


class Traced(lfx.Traced):
    """lights_fixture.Traced, and per ray: passes (transmissive hits followed), sphere_pass /
    pane_pass (of which spheres / panes), after_bounce (a glass sphere was entered after an
    opaque hit); over the whole trace: k2_min and dnorm_max = max | |d'| - 1 | of the sphere
    passages."""

    def __init__(self, n, depth, nl):
        super().__init__(n, depth, nl)
        self.passes = np.zeros(n, np.int32)
        self.sphere_pass = np.zeros(n, np.int32)
        self.pane_pass = np.zeros(n, np.int32)
        self.after_bounce = np.zeros(n, bool)
        self.k2_min = math.inf
        self.dnorm_max = 0.0


def records(trans, n):
    """trans (None, or per scene object a (tau, ior) pair or 0) -> [(tau, ior)] * n."""
    out = []
    for j in range(n):
        t = trans[j] if trans else 0
        out.append((float(t), 1.0) if isinstance(t, (int, float)) else (float(t[0]), float(t[1])))
    return out


def trace(orc, prims, origins, directions, depth, lights, shadows, trans, want_fragile=True):
    o = np.ascontiguousarray(origins, np.float64).reshape(-1, 3).copy()
    d = np.ascontiguousarray(directions, np.float64).reshape(-1, 3).copy()
    Ps = [np.array(p, np.float64) for p, _ in lights]
    Cs = [np.array(c, np.float64) for _, c in lights]
    rec = records(trans, len(prims))
    n, nl = len(o), len(lights)
    res = Traced(n, depth, nl)
    bounced = np.zeros(n, bool)
    live = np.arange(n)
    levels = []  # per level: (ray ids, local colour [m, 3], weight [m])
    leaf = np.zeros((n, 3))
    arr = orc.prim_array(prims)
    dp = C.POINTER(C.c_double)
    cdist, cn = C.c_double(), np.empty(3)
    for k in range(depth + 1):
        if len(live) == 0:
            break
        idx = np.empty(len(live), np.int32)
        dist = np.empty(len(live))
        nrm = np.empty((len(live), 3))
        for q, r in enumerate(live):
            idx[q] = orc.lib.orc_find_closest_hit(arr, len(prims), o[r].ctypes.data_as(dp),
                                                  d[r].ctypes.data_as(dp), C.byref(cdist),
                                                  cn.ctypes.data_as(dp))
            dist[q] = cdist.value
            nrm[q] = cn
        res.hits[live, k] = idx
        miss = idx < 0
        for r in live[miss]:
            leaf[r] = orc.out_color(d[r])
        live, idx, dist, nrm = live[~miss], idx[~miss], dist[~miss], nrm[~miss]
        if len(live) == 0:
            break
        pos = o[live] + d[live] * dist[:, None]                    # main.cpp:99
        start = pos + nrm * .0001                                   # main.cpp:111
        blocked = np.zeros((len(live), nl), np.uint8)
        if shadows:
            for l in range(nl):
                blocked[:, l], frag = lfx._light_level(orc, prims, start, Ps[l], want_fragile)
                res.fragile[live] |= frag
            res.shadow[live, k] = blocked
        local = np.empty((len(live), 3))
        wgt = np.empty(len(live))
        for q, r in enumerate(live):
            m = prims[int(idx[q])].mat
            acc = None
            for l in range(nl):
                if blocked[q, l]:
                    s = 0.0
                else:
                    di = orc.diffuse_shading(pos[q], nrm[q], Ps[l])
                    sp = math.pow(orc.specular(pos[q], nrm[q], Ps[l], -d[r]), m.specular_exponent)
                    s = di * m.diffuse + sp * m.specular
                t = Cs[l] * s
                acc = t if l == 0 else acc + t
            local[q] = np.array(m.color[:]) * (acc + m.ambient)
            tau = rec[int(idx[q])][0]
            wgt[q] = tau if tau > 0 else m.metallic
        if k >= depth:                                              # remaining_iterations <= 0
            leaf[live] = local
            break
        levels.append((live.copy(), local, wgt))
        for q, r in enumerate(live):
            j = int(idx[q])
            tau, ior = rec[j]
            if tau > 0:
                res.passes[r] += 1
                if prims[j].kind == capi.RT_PRIM_WALL:
                    res.pane_pass[r] += 1
                    o[r], d[r] = pane_step(pos[q], nrm[q], d[r])
                else:
                    res.sphere_pass[r] += 1
                    res.after_bounce[r] |= bounced[r]
                    proj, _ = ofx.sphere_projection(prims[j], o[r], d[r])
                    c = np.array(prims[j].position[:], np.float64)
                    o[r], d[r], k2, _ = sphere_step(o[r], d[r], float(proj[0]), c, ior)
                    res.k2_min = min(res.k2_min, k2)
                    res.dnorm_max = max(res.dnorm_max, abs(math.sqrt(_dot(d[r], d[r])) - 1.0))
            else:
                bounced[r] = True
                d[r] = orc.reflect(d[r], nrm[q])                    # main.cpp:112
                o[r] = start[q]
    rgb = leaf
    for ids, local, wgt in reversed(levels):                        # vec.cpp:45-49 via main.cpp:117
        rgb[ids] = local + wgt[:, None] * (rgb[ids] - local)
    res.rgb = rgb
    return res


# ---- scene G: hand-built; every material keeps the constructor defaults but colour and metallic
def scene_g():
    M, S, W = scenes.Material, scenes.Sphere, scenes.Wall
    grey = lambda g: M((g, g, g))
    return [
        S(M((.9, .95, 1), .3), (2.0, -.5, 0), 1.0),
        S(M((.6, 1, .7), .5), (1.6, 1.0, .3), .5),
        S(M((1, .3, .2), .6), (6, -1, .5), .8),
        S(M((.2, .4, 1), .2), (5.5, 1.5, -.3), .6),
        S(M((1, .9, .2), 0.0), (7, .3, 1.2), .5),
        W(grey(.7), (3, 4, -1), (0, -1, 0), 8, 4),
        W(grey(.5), (3, -4, -1), (0, 1, 0), 8, 4),
        W(grey(.4), (10, -4, -1), (-1, 0, 0), 8, 4),
        W(M((.8, .9, 1)), (1.0, .3, -.8), (-1, 0, 0), 1.5, 1.5),
    ]


TRANS_G = [(.9, 1.5), (.7, 1.33), 0, 0, 0, 0, 0, 0, (.6, 1)]


def trans_sl(ns, nw):
    """Scenes S and L: spheres with index % 4 != 3 get (.85, 1.5); wall ns + 1 gets (.6, 1)."""
    t = [(.85, 1.5) if j % 4 != 3 else 0 for j in range(ns)] + [0] * nw
    t[ns + 1] = (.6, 1)
    return t


CAM_A13 = dict(sfx.CAM_A, image_width=13)
# name -> (scene key, camera, depth)
CASES = {
    "G": ("G", sfx.CAM_A, sfx.DEPTH_S),
    "G13": ("G", CAM_A13, sfx.DEPTH_S),
    "SA": ("S", sfx.CAM_A, sfx.DEPTH_S),
    "SB": ("S", sfx.CAM_B, sfx.DEPTH_S),
    "L": ("L", sfx.CAM_B, sfx.DEPTH_L),
}
LIGHTS = dict(lfx.SETS, NONE=lfx.ONE)   # no lights set: the reference's light


@functools.lru_cache(maxsize=None)
def scene(key):
    """-> (prims, transmission records) of scene G, S or L."""
    if key == "G":
        return scenes.to_prims(scene_g()), TRANS_G
    ns, nw = {"S": (8, 4), "L": (64, 6)}[key]
    return sfx.scene_prims(ns, nw), trans_sl(ns, nw)


@functools.lru_cache(maxsize=None)
def case(name, lights="NONE", shadows=False, glass=True):
    """-> (prims, trans, cam, depth, Traced) of a named frame, computed once per process;
    glass=False: the same frame with every object opaque."""
    import oracle as orc_mod
    key, cam_args, depth = CASES[name]
    prims, trans = scene(key)
    cam = capi.camera_init(**cam_args)
    o, d = sfx.camera_rays(cam)
    tr = trace(orc_mod.Oracle(), prims, o, d, depth, LIGHTS[lights], shadows, trans if glass else None)
    return prims, trans, cam, depth, tr


@functools.lru_cache(maxsize=None)
def ray_case(lights="NONE", shadows=False):
    """The 1,536 scaled pixel rays of camera A on scene G (|d| from 0.25 to 4, so main.cpp:99's
    off-surface pos and the true P differ) -> (prims, trans, o, d, depth, Traced)."""
    import oracle as orc_mod
    prims, trans = scene("G")
    o, d = sfx.scaled_rays(capi.camera_init(**sfx.CAM_A))
    tr = trace(orc_mod.Oracle(), prims, o, d, sfx.DEPTH_S, LIGHTS[lights], shadows, trans)
    return prims, trans, o, d, sfx.DEPTH_S, tr


def coverage(tr, prims, trans):
    """Shares of the primary rays that hit a glass sphere / a pane, and of the rays that pass two
    or more transmissive objects."""
    rec = records(trans, len(prims))
    first = tr.hits[:, 0]
    glass = np.array([rec[j][0] > 0 if j >= 0 else False for j in first])
    wall = np.array([prims[j].kind == capi.RT_PRIM_WALL if j >= 0 else False for j in first])
    return (float((glass & ~wall).mean()), float((glass & wall).mean()), float((tr.passes >= 2).mean()))
