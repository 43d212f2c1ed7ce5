"""Expected results of the occlusion query (rt_occluded), shared by the test_occluded_* files.

For ray k and primitive j the reference's Collision c = scene[j]->intersect(ray) blocks the
segment o .. o + d * T when c.distance > 0 (find_closest_hit's acceptance, main.cpp:77) and
its parameter along the ray is <= T:

  * a wall's parameter is c.distance itself (its t, scene.cpp:10): taken from the oracle's
    orc_wall_intersect;
  * a sphere's is `projection`, which scene.cpp:77 multiplies by |d| and does not return: the
    arithmetic of scene.cpp:45-76 is restated here in numpy fp64, vectorised over rays, one
    IEEE operation per reference operation (dot products as x*x + y*y + z*z left to right, no
    fused multiply-add).  test_occluded_host.py pins projection * sqrt(a) to the oracle's
    returned distance bit for bit.
"""
import ctypes as C

import numpy as np

from rtamd import capi

BOX_LO, BOX_HI = [-2, -5, -2], [9, 5, 3]   # the golden rays' origin box (make_golden.py)


def _dot(u, v):
    return u[:, 0] * v[:, 0] + u[:, 1] * v[:, 1] + u[:, 2] * v[:, 2]


def sphere_projection(prim, o, d):
    """Sphere::intersect's (projection, a) for every ray; projection is NaN where det < 0."""
    o = np.asarray(o, np.float64).reshape(-1, 3)
    d = np.asarray(d, np.float64).reshape(-1, 3)
    center = np.array(prim.position[:], np.float64)
    radius = float(prim.radius)
    oc = o - center                                   # scene.cpp:45
    a = _dot(d, d)                                    # :47
    b = 2 * _dot(d, oc)                               # :49
    c = _dot(oc, oc) - radius * radius                # :51
    det = b * b - 4 * a * c                           # :53
    with np.errstate(all="ignore"):
        sq = np.sqrt(np.where(det < 0, 0.0, det))
        p1 = (-b + sq) / (2 * a)                      # :70
        p2 = (-b - sq) / (2 * a)                      # :71
        proj = np.where(p1 < p2, p1, p2)              # :72
        proj = np.where(det == 0, (-b - sq) / a, proj)  # :65
        proj = np.where(det < 0, np.nan, proj)        # :58
    return proj, a


def expected_params(oracle, prims, o, d):
    """T[n, nprims]: the parameter of each accepted hit (c.distance > 0), else NaN."""
    o = np.ascontiguousarray(o, np.float64).reshape(-1, 3)
    d = np.ascontiguousarray(d, np.float64).reshape(-1, 3)
    n = len(o)
    T = np.full((n, len(prims)), np.nan)
    dp = C.POINTER(C.c_double)
    dist, nrm, hit = C.c_double(), (C.c_double * 3)(), C.c_int()
    for j, prim in enumerate(prims):
        if prim.kind == capi.RT_PRIM_WALL:
            for k in range(n):
                oracle.lib.orc_wall_intersect(C.byref(prim), o[k].ctypes.data_as(dp),
                                              d[k].ctypes.data_as(dp), C.byref(dist), nrm,
                                              C.byref(hit))
                if dist.value > 0:
                    T[k, j] = dist.value
        else:
            proj, a = sphere_projection(prim, o, d)
            with np.errstate(all="ignore"):
                ok = proj * np.sqrt(a) > 0            # c.distance > 0 (scene.cpp:77)
            T[ok, j] = proj[ok]
    return T


def expected_occluded(T, tmax):
    """uint8[n]: 1 where some accepted parameter is <= the ray's limit (NaN compares false)."""
    tmax = np.broadcast_to(np.asarray(tmax, np.float64), (T.shape[0],))
    with np.errstate(invalid="ignore"):
        return np.any(T <= tmax[:, None], axis=1).astype(np.uint8)


def drawn_limits(n, seed):
    """Per-ray limits from {0.25, 1, 3, 10, inf}, seeded."""
    rng = np.random.default_rng(seed)
    return rng.choice(np.array([0.25, 1.0, 3.0, 10.0, np.inf]), size=n)


def point_pairs(n, seed):
    """Seeded random point pairs in the fixture's box -> (o = a, d = b - a); tmax = 1."""
    rng = np.random.default_rng(seed)
    a = rng.uniform(BOX_LO, BOX_HI, size=(n, 3))
    b = rng.uniform(BOX_LO, BOX_HI, size=(n, 3))
    return a, b - a
