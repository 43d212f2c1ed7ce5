"""Expected frame AOVs (rt_render_aov), shared by the test_aov_* files.

The expectation uses the oracle's exports and numpy only.  Pixel (i, j)'s ray is
shadow_fixture.camera_rays' (main.cpp:132-134); its record is the oracle's find_closest_hit
(a miss: main.cpp:70's placeholder {DBL_MAX, (0,0,0), -1}); the other layers follow from the
record in numpy fp64, one IEEE operation per written operation, then one cast to float32:

  index   the record's
  depth   sphere: distance;  wall: distance * sqrt(d.x*d.x + d.y*d.y + d.z*d.z);  miss: +inf
  normal  n / sqrt(n.x*n.x + n.y*n.y + n.z*n.z) per component;  miss: 0
  albedo  the hit object's mat.color;  miss: 0
"""
import ctypes as C
import functools

import numpy as np

import shadow_fixture as sfx
from rtamd import capi

DBL_MAX = np.finfo(np.float64).max
LAYERS = ("hit", "index", "depth", "normal", "albedo")


def _len(v):
    """vec3::length (vec.cpp:3-9) of every row: the squares summed left to right."""
    return np.sqrt(v[:, 0] * v[:, 0] + v[:, 1] * v[:, 1] + v[:, 2] * v[:, 2])


def closest_hits(orc, prims, o, d):
    """The oracle's find_closest_hit per ray as a HIT_DTYPE array."""
    o = np.ascontiguousarray(o, np.float64).reshape(-1, 3)
    d = np.ascontiguousarray(d, np.float64).reshape(-1, 3)
    hits = np.zeros(len(o), capi.HIT_DTYPE)
    hits["distance"], hits["index"] = DBL_MAX, -1
    arr = orc.prim_array(prims)
    dp = C.POINTER(C.c_double)
    dist, nrm = C.c_double(), np.empty(3)
    for k in range(len(o)):
        idx = orc.lib.orc_find_closest_hit(arr, len(prims), o[k].ctypes.data_as(dp),
                                           d[k].ctypes.data_as(dp), C.byref(dist),
                                           nrm.ctypes.data_as(dp))
        if idx >= 0:
            hits[k] = (dist.value, nrm, idx, 0)
    return hits


def layers_of(prims, hits, d):
    """{layer: array} of flat per-ray layers from the records and the ray directions."""
    n = len(hits)
    idx = hits["index"]
    hit = idx >= 0
    is_wall = np.array([p.kind == capi.RT_PRIM_WALL for p in prims] + [False], bool)[idx]  # [-1]: miss
    color = np.array([p.mat.color[:] for p in prims] + [[0.0, 0.0, 0.0]], np.float64)[idx]
    depth = np.full(n, np.inf)
    depth[hit] = hits["distance"][hit]
    w = hit & is_wall
    depth[w] = hits["distance"][w] * _len(d[w])
    normal = np.zeros((n, 3))
    nv = hits["normal"][hit]
    normal[hit] = nv / _len(nv)[:, None]
    albedo = np.zeros((n, 3))
    albedo[hit] = color[hit]
    return dict(hit=hits.copy(), index=idx.astype(np.int32), depth=depth.astype(np.float32),
                normal=normal.astype(np.float32), albedo=albedo.astype(np.float32))


def expected(orc, prims, cam):
    """{layer: [H, W(, 3)] array} for the whole frame of cam, plus "kind" [H, W]: -1 miss,
    0 sphere, 1 wall."""
    o, d = sfx.camera_rays(cam)
    hits = closest_hits(orc, prims, o, d)
    out = {k: v.reshape((cam.height, cam.width) + v.shape[1:])
           for k, v in layers_of(prims, hits, d).items()}
    kinds = np.array([1 if p.kind == capi.RT_PRIM_WALL else 0 for p in prims] + [-1], np.int8)
    out["kind"] = kinds[out["index"]]
    return out


def counts(exp):
    """(misses, sphere hits, wall hits) of an expected frame."""
    k = exp["kind"]
    return int((k == -1).sum()), int((k == 0).sum()), int((k == 1).sum())


# primary-hit counts of shadow_fixture.CASES (CPU oracle): what each case exercises
COUNTS = {"A": (937, 156, 443), "B": (956, 4, 576), "B13": (65, 0, 39), "L": (929, 205, 402)}

# The views case: views.npz's scene "tilt" (tilted walls) from its smallest view, "inside"
# (32 x 24), with the camera moved after Camera::init the way the reference's key handler moves
# it: position changes, image_top_left stays where init put it.
VIEWS_SCENE, VIEWS_VIEW = "tilt", "inside"
VIEWS_MOVE = (-0.75, 0.5, 0.25)


@functools.lru_cache(maxsize=None)
def views_camera():
    from views_fixture import Views
    v = Views()
    cam = v.camera(VIEWS_VIEW)
    for k in range(3):
        cam.position[k] += VIEWS_MOVE[k]
    return v.prims(VIEWS_SCENE), cam


@functools.lru_cache(maxsize=None)
def case(name):
    """-> (prims, cam, expected) of a named case (shadow_fixture.CASES or "views"), computed
    once per process; read only."""
    import oracle as orc_mod
    if name == "views":
        prims, cam = views_camera()
    else:
        ns, nw, cam_args, _ = sfx.CASES[name]
        prims, cam = sfx.scene_prims(ns, nw), capi.camera_init(**cam_args)
    return prims, cam, expected(orc_mod.Oracle(), prims, cam)


def same_bytes(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()
