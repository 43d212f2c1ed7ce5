"""Expected radiance under scene lights (rt_set_lights), shared by the test_lights_* files.

shadow_fixture.trace generalised to a list of coloured point lights, following rt_capi.h's
"Lights" definition.  The oracle's exported functions do find_closest_hit, diffuse_shading,
specular, out_color and reflect; pos, sp, pow, the accumulation over the lights and the lerp are
numpy / libm fp64, one IEEE operation per written operation:

    diff_l = diffuse_shading(pos, col.normal, P_l)
    spec_l = pow(specular(pos, col.normal, P_l, -d), mat.specular_exponent)
    s_l    = diff_l * mat.diffuse + spec_l * mat.specular       (+0.0 where light l is hidden)
    t = C_l[c] * s_l;  acc[c] = t for l == 0, else acc[c] + t
    local[c] = mat.color[c] * (acc[c] + mat.ambient)

With shadows on, every accepted hit asks occluded_fixture about the segment from
sp = pos + col.normal * .0001 towards every light: direction P_l - sp, T = 1.

A ray is FRAGILE as in shadow_fixture, per light: at some hit of its path the decision for some
light changes under T in {1 - 1e-9, 1 + 1e-9} or under a displacement of sp by +-1e-9 along one
axis (direction recomputed).
"""
import ctypes as C
import functools
import math

import numpy as np

import occluded_fixture as ofx
import shadow_fixture as sfx
from rtamd import capi

FRAGILE_EPS = sfx.FRAGILE_EPS

ONE = [((0, 0, 0), (1, 1, 1))]
K2 = [((1, -2, 2.5), (1, .8, .6)), ((6, 1.5, 3), (.3, .5, 1))]
K4 = K2 + [((0, 0, 0), (.5, .5, .5)), ((9, -3, .5), (.6, .2, .2))]
K8 = K4 + [((4, 0, 2.9), (.2, .2, .2)), ((1, 3.5, 1), (.1, .3, .1)), ((7, -2, 2.95), (.25, .1, .3)),
           ((-1, 1, -.5), (.3, .3, .1))]
SETS = {"ONE": ONE, "K2": K2, "K4": K4, "K8": K8}


class Traced:
    """rgb [n, 3]; hits [n, depth + 1] scene index per level (-1 miss, -2 path over);
    shadow [n, depth + 1, nlights] (1 = that light is hidden from that level's hit);
    fragile [n] bool."""

    def __init__(self, n, depth, nl):
        self.rgb = np.zeros((n, 3))
        self.hits = np.full((n, depth + 1), -2, np.int32)
        self.shadow = np.zeros((n, depth + 1, nl), np.uint8)
        self.fragile = np.zeros(n, bool)


def _light_level(orc, prims, sp, P, want_fragile):
    """-> (blocked uint8[m], fragile bool[m]) of the segments sp .. P."""
    T = ofx.expected_params(orc, prims, sp, P - sp)
    blocked = ofx.expected_occluded(T, 1.0)
    fragile = np.zeros(len(sp), bool)
    if want_fragile:
        for t in (1.0 - FRAGILE_EPS, 1.0 + FRAGILE_EPS):
            fragile |= ofx.expected_occluded(T, t) != blocked
        for ax in range(3):
            for sgn in (-1.0, 1.0):
                q = sp.copy()
                q[:, ax] += sgn * FRAGILE_EPS
                fragile |= ofx.expected_occluded(ofx.expected_params(orc, prims, q, P - q), 1.0) != blocked
    return blocked, fragile


def trace(orc, prims, origins, directions, depth, lights, shadows, want_fragile=True):
    o = np.ascontiguousarray(origins, np.float64).reshape(-1, 3).copy()
    d = np.ascontiguousarray(directions, np.float64).reshape(-1, 3).copy()
    Ps = [np.array(p, np.float64) for p, _ in lights]
    Cs = [np.array(c, np.float64) for _, c in lights]
    n, nl = len(o), len(lights)
    res = Traced(n, depth, nl)
    live = np.arange(n)
    levels = []  # per level: (ray ids, local colour [m, 3], metallic [m])
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
                blocked[:, l], frag = _light_level(orc, prims, start, Ps[l], want_fragile)
                res.fragile[live] |= frag
            res.shadow[live, k] = blocked
        local = np.empty((len(live), 3))
        km = np.empty(len(live))
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
            km[q] = m.metallic
        if k >= depth:                                              # remaining_iterations <= 0
            leaf[live] = local
            break
        levels.append((live.copy(), local, km))
        for q, r in enumerate(live):
            d[r] = orc.reflect(d[r], nrm[q])                        # main.cpp:112
        o[live] = start
    rgb = leaf
    for ids, local, km in reversed(levels):                         # vec.cpp:45-49 via main.cpp:117
        rgb[ids] = local + km[:, None] * (rgb[ids] - local)
    res.rgb = rgb
    return res


def trace_frame(orc, prims, cam, depth, lights, shadows, want_fragile=True):
    o, d = sfx.camera_rays(cam)
    return trace(orc, prims, o, d, depth, lights, shadows, want_fragile)


@functools.lru_cache(maxsize=None)
def case(name, lights, shadows, depth=None):
    """-> (prims, cam, depth, Traced) of the named shadow_fixture frame under the named light
    set, computed once per process."""
    import oracle as orc_mod
    ns, nw, cam_args, dep = sfx.CASES[name]
    dep = dep if depth is None else depth
    prims = sfx.scene_prims(ns, nw)
    cam = capi.camera_init(**cam_args)
    return prims, cam, dep, trace_frame(orc_mod.Oracle(), prims, cam, dep, SETS[lights], shadows)


@functools.lru_cache(maxsize=None)
def ray_case(lights, shadows):
    """The 1,536 scaled pixel rays of camera B on scene S -> (prims, o, d, depth, Traced)."""
    import oracle as orc_mod
    prims = sfx.scene_prims(8, 4)
    o, d = sfx.scaled_rays(capi.camera_init(**sfx.CAM_B))
    return prims, o, d, sfx.DEPTH_S, trace(orc_mod.Oracle(), prims, o, d, sfx.DEPTH_S, SETS[lights],
                                           shadows)
