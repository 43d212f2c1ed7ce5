"""CPU-side checks of the occlusion query (rt_occluded, rt_occluded_device): declarations,
exports and bindings, the argument check that needs no device, and the expected-result
fixture (tests/occluded_fixture.py) pinned to the oracle's per-primitive intersections and to
the reference's recorded closest hits (tests/golden/ray_hits.npz)."""
import ctypes as C
import os
import re
import subprocess

import numpy as np

from conftest import GOLDEN, REPO, scene_by_name
from occluded_fixture import expected_occluded, expected_params, sphere_projection
from rtamd import capi, scenes

NAMES = ("rt_occluded", "rt_occluded_device")
SCENES = ("default", "s8w4", "s64w6")


def test_header_declares_both_entry_points():
    text = open(os.path.join(REPO, "include", "rt_capi.h")).read()
    assert "#define RT_CAPI_VERSION 2" in text
    for name in NAMES:
        assert re.search(r"\bint " + name + r"\(rt_ctx\*", text), name


def test_library_exports_and_bindings():
    lib = capi.load()
    out = subprocess.run(["nm", "-D", "--defined-only", capi.LIB_PATH], capture_output=True,
                         text=True, check=True).stdout
    exported = set(re.findall(r" T (rt_[a-z0-9_]+)$", out, flags=re.M))
    assert set(NAMES) <= exported
    assert set(NAMES) <= {n for n, _, _ in capi.SIGNATURES}
    for name in NAMES:
        assert getattr(lib, name).restype is C.c_int
    assert callable(capi.Renderer.occluded) and callable(capi.Renderer.occluded_device)


def test_null_ctx_rejected_without_device():
    lib = capi.load()
    o = (C.c_double * 3)(0, 0, 0)
    d = (C.c_double * 3)(1, 0, 0)
    out, cnt = (C.c_uint8 * 1)(7), C.c_uint64(9)
    assert lib.rt_occluded(None, o, d, None, 1, out, C.byref(cnt), None) == capi.RT_ERR_INVALID_ARG
    assert lib.rt_occluded_device(None, None, None, None, 1, None, None,
                                  None) == capi.RT_ERR_INVALID_ARG
    assert out[0] == 7 and cnt.value == 9


def test_sphere_restatement_bit_exact_vs_oracle(oracle, golden_rays):
    """projection * sqrt(a) of the numpy restatement is the oracle's Sphere::intersect distance
    bit for bit wherever that distance is > 0, for every golden ray and every sphere."""
    checked = 0
    for name in SCENES:
        prims = scenes.to_prims(scene_by_name(name))
        o, d = golden_rays[f"{name}__o"], golden_rays[f"{name}__d"]
        for prim in prims:
            if prim.kind != capi.RT_PRIM_SPHERE:
                continue
            proj, a = sphere_projection(prim, o, d)
            with np.errstate(all="ignore"):
                mine = proj * np.sqrt(a)
            for k in range(len(o)):
                dist, _, hit = oracle.sphere_intersect(prim, o[k], d[k])
                if dist > 0:
                    assert hit == 1
                    assert np.float64(dist).tobytes() == mine[k].tobytes(), (name, k)
                    checked += 1
                else:
                    assert not (mine[k] > 0), (name, k)
    assert checked > 100   # accepted sphere hits among the golden rays


def test_no_limit_equals_the_references_recorded_hits(oracle, golden_rays):
    """With T = +inf a ray is occluded exactly where the reference's find_closest_hit recorded
    a hit (ray_hits.npz)."""
    hits = np.load(os.path.join(GOLDEN, "ray_hits.npz"))
    for name in SCENES:
        prims = scenes.to_prims(scene_by_name(name))
        T = expected_params(oracle, prims, golden_rays[f"{name}__o"], golden_rays[f"{name}__d"])
        exp = expected_occluded(T, np.inf)
        assert np.array_equal(exp, (hits[f"{name}__index"] >= 0).astype(np.uint8)), name
        assert 0 < exp.sum() < len(exp)
        # the limits that are never occluded
        for t in (np.nan, 0.0, -1.0):
            assert not expected_occluded(T, t).any()
