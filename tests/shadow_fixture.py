"""Expected radiance with RT_FLAG_SHADOWS, shared by the test_shadows_* files.

recursive_ray_tracing (main.cpp:89-119) restated level by level for arbitrary rays.  The
oracle's exported functions do find_closest_hit, diffuse_shading, specular, out_color and
reflect; pos, the shadow ray's origin, pow, local_color and the lerp are numpy / libm fp64, one
IEEE operation per reference operation (rt_oracle.c trace()).  With shadows on, every accepted
hit asks occluded_fixture about the segment sp .. LIGHT_POS:

    sp = pos + col.normal * .0001     (main.cpp:111's start point)
    sd = LIGHT_POS - sp = -sp,  T = 1

and a blocked hit has diffuse_intensity = specular_intensity = 0.

A ray is FRAGILE when, at some hit of its path, the decision changes under T in {1 - 1e-9,
1 + 1e-9} or under a displacement of sp by +-1e-9 along one axis (direction recomputed): about
1e5 times any rounding difference between an implementation and this file.
"""
import ctypes as C
import functools
import math

import numpy as np

import occluded_fixture as ofx
from rtamd import capi, scenes

FRAGILE_EPS = 1e-9


class Traced:
    """rgb [n, 3]; hits [n, depth + 1] scene index per level (-1 miss, -2 path over);
    shadow [n, depth + 1] (1 = that level's hit is shadowed); blocker_kinds [n, depth + 1]
    bit 0 = a sphere blocks, bit 1 = a wall blocks; fragile [n] bool."""

    def __init__(self, n, depth):
        self.rgb = np.zeros((n, 3))
        self.hits = np.full((n, depth + 1), -2, np.int32)
        self.shadow = np.zeros((n, depth + 1), np.uint8)
        self.blocker_kinds = np.zeros((n, depth + 1), np.uint8)
        self.fragile = np.zeros(n, bool)


def _shadow_level(orc, prims, sp, want_fragile):
    """-> (blocked uint8[m], kinds uint8[m], fragile bool[m]) for the shadow origins sp."""
    T = ofx.expected_params(orc, prims, sp, -sp)
    blocked = ofx.expected_occluded(T, 1.0)
    is_sph = np.array([p.kind != capi.RT_PRIM_WALL for p in prims])
    with np.errstate(invalid="ignore"):
        hit = T <= 1.0
    kinds = (np.any(hit[:, is_sph], axis=1).astype(np.uint8) |
             (np.any(hit[:, ~is_sph], axis=1).astype(np.uint8) << 1))
    fragile = np.zeros(len(sp), bool)
    if want_fragile:
        for t in (1.0 - FRAGILE_EPS, 1.0 + FRAGILE_EPS):
            fragile |= ofx.expected_occluded(T, t) != blocked
        for ax in range(3):
            for sgn in (-1.0, 1.0):
                q = sp.copy()
                q[:, ax] += sgn * FRAGILE_EPS
                fragile |= ofx.expected_occluded(ofx.expected_params(orc, prims, q, -q), 1.0) != blocked
    return blocked, kinds, fragile


def trace(orc, prims, origins, directions, depth, shadows, want_fragile=True):
    o = np.ascontiguousarray(origins, np.float64).reshape(-1, 3).copy()
    d = np.ascontiguousarray(directions, np.float64).reshape(-1, 3).copy()
    n = len(o)
    res = Traced(n, depth)
    live = np.arange(n)
    # per level: (ray ids, local colour [m, 3], metallic [m])
    levels = []
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
        blocked = np.zeros(len(live), np.uint8)
        if shadows:
            blocked, kinds, frag = _shadow_level(orc, prims, start, want_fragile)
            res.shadow[live, k] = blocked
            res.blocker_kinds[live, k] = kinds
            res.fragile[live] |= frag
        local = np.empty((len(live), 3))
        km = np.empty(len(live))
        for q, r in enumerate(live):
            m = prims[int(idx[q])].mat
            if blocked[q]:
                di = sp = 0.0
            else:
                di = orc.diffuse_shading(pos[q], nrm[q], (0.0, 0.0, 0.0))          # main.cpp:102
                sp = math.pow(orc.specular(pos[q], nrm[q], (0.0, 0.0, 0.0), -d[r]),
                              m.specular_exponent)                                # main.cpp:103
            s = di * m.diffuse + sp * m.specular + m.ambient                       # main.cpp:104
            local[q] = np.array(m.color[:]) * s
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


def camera_rays(cam):
    """Pixel rays of rt_scene (main.cpp:132-134): origin the camera, direction
    position - pixel_center, un-normalised; row-major [H * W, 3]."""
    pos = np.array(cam.position[:])
    tl = np.array(cam.image_top_left[:])
    dx = np.array(cam.pixel_delta_x[:])
    dy = np.array(cam.pixel_delta_y[:])
    x = np.arange(cam.width, dtype=np.float64)[None, :, None]
    i = np.arange(cam.height, dtype=np.float64)[:, None, None]
    pc = (tl + dx * x) + dy * i
    d = (pos - pc).reshape(-1, 3)
    return np.broadcast_to(pos, d.shape).copy(), d


def trace_frame(orc, prims, cam, depth, shadows, want_fragile=True):
    o, d = camera_rays(cam)
    return trace(orc, prims, o, d, depth, shadows, want_fragile)


def scaled_rays(cam, seed=77):
    """The pixel rays of cam, each direction multiplied by a seeded factor in [0.25, 4]."""
    o, d = camera_rays(cam)
    f = np.random.default_rng(seed).uniform(0.25, 4.0, size=len(d))
    return o, d * f[:, None]


CAM_A = dict(position=(0, 0, 0), lookat=(-1, 0, 0), vup=(0, 0, -1), vfov=90, aspect_ratio=1.5,
             image_width=48)
CAM_B = dict(CAM_A, position=(4, -2, -1), lookat=(0, 0, 0))
CAM_B13 = dict(CAM_B, image_width=13)
DEPTH_S, DEPTH_L = 3, 6
# name -> (spheres, walls, camera, depth): scene S at cameras A, B and the 13-wide B (partial
# tiles), scene L (64 spheres: the wave-cull kernels) at camera B
CASES = {
    "A": (8, 4, CAM_A, DEPTH_S),
    "B": (8, 4, CAM_B, DEPTH_S),
    "B13": (8, 4, CAM_B13, DEPTH_S),
    "L": (64, 6, CAM_B, DEPTH_L),
}


@functools.lru_cache(maxsize=None)
def scene_prims(n_spheres, n_walls):
    return scenes.to_prims(scenes.synthetic_scene(n_spheres, n_walls, seed=1234))


@functools.lru_cache(maxsize=None)
def case(name, shadows):
    """-> (prims, cam, depth, Traced) of one named frame, computed once per process."""
    import oracle as orc_mod
    ns, nw, cam_args, depth = CASES[name]
    prims = scene_prims(ns, nw)
    cam = capi.camera_init(**cam_args)
    return prims, cam, depth, trace_frame(orc_mod.Oracle(), prims, cam, depth, shadows)


@functools.lru_cache(maxsize=None)
def ray_case(shadows):
    """The 1,536 scaled pixel rays of camera B on scene S -> (prims, o, d, depth, Traced)."""
    import oracle as orc_mod
    prims = scene_prims(8, 4)
    o, d = scaled_rays(capi.camera_init(**CAM_B))
    return prims, o, d, DEPTH_S, trace(orc_mod.Oracle(), prims, o, d, DEPTH_S, shadows)


def discontinuity_mask(hits, H, W):
    """Pixels whose 3x3 neighbourhood holds more than one hit-index sequence."""
    seq = hits.reshape(H, W, -1)
    m = np.zeros((H, W), bool)
    for di in (-1, 0, 1):
        for dj in (-1, 0, 1):
            if di == 0 and dj == 0:
                continue
            a = seq[max(0, di):H + min(0, di), max(0, dj):W + min(0, dj)]
            b = seq[max(0, -di):H + min(0, -di), max(0, -dj):W + min(0, -dj)]
            m[max(0, di):H + min(0, di), max(0, dj):W + min(0, dj)] |= np.any(a != b, axis=-1)
    return m
