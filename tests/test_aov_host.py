"""CPU-side checks of the frame AOVs (rt_render_aov, rt_render_aov_device): declarations,
exports and bindings, the argument check that needs no device, and the expected-result fixture
(tests/aov_fixture.py) pinned to the primary-hit counts it is meant to exercise, to its own
definitions and to the reference's recorded closest hits (tests/golden/ray_hits.npz)."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import aov_fixture as afx
from conftest import GOLDEN, REPO, scene_by_name
from rtamd import capi, scenes

NAMES = ("rt_render_aov", "rt_render_aov_device")
CASES = ("A", "B", "B13", "L", "views")


def test_header_declares_entry_points_and_struct():
    text = open(os.path.join(REPO, "include", "rt_capi.h")).read()
    assert "#define RT_CAPI_VERSION 2" in text
    for name in NAMES:
        assert re.search(r"\bint " + name + r"\(rt_ctx\*", text), name
    m = re.search(r"typedef struct rt_aov_buffers \{(.*?)\} rt_aov_buffers;", text, flags=re.S)
    assert m
    fields = re.findall(r"^\s*[a-z0-9_]+\*\s+([a-z]+);", m.group(1), flags=re.M)
    assert fields == ["hit", "index", "depth", "normal", "albedo", "reserved"]
    assert [f for f, _ in capi.rt_aov_buffers._fields_] == fields
    assert C.sizeof(capi.rt_aov_buffers) == 48
    assert capi.HIT_DTYPE.itemsize == C.sizeof(capi.rt_hit) == 40


def test_library_exports_and_bindings():
    lib = capi.load()
    out = subprocess.run(["nm", "-D", "--defined-only", capi.LIB_PATH], capture_output=True,
                         text=True, check=True).stdout
    exported = set(re.findall(r" T (rt_[a-z0-9_]+)$", out, flags=re.M))
    assert set(NAMES) <= exported
    assert set(NAMES) <= {n for n, _, _ in capi.SIGNATURES}
    for name in NAMES:
        assert getattr(lib, name).restype is C.c_int
    assert callable(capi.Renderer.render_aov) and callable(capi.Renderer.render_aov_device)
    assert tuple(capi.AOV_LAYERS) == afx.LAYERS


def test_null_ctx_rejected_without_device():
    lib = capi.load()
    cam = capi.camera_init(**afx.sfx.CAM_B13)
    idx = np.full(4, 7, np.int32)
    dep = np.full(4, 7.0, np.float32)
    bufs = capi.rt_aov_buffers(index=idx.ctypes.data, depth=dep.ctypes.data)
    st = capi.rt_stats()
    assert lib.rt_render_aov(None, C.byref(cam), 0, 1, C.byref(bufs), C.byref(st)) == capi.RT_ERR_INVALID_ARG
    assert lib.rt_render_aov_device(None, C.byref(cam), 0, 1, C.byref(bufs), None) == capi.RT_ERR_INVALID_ARG
    assert (idx == 7).all() and (dep == 7.0).all()


@pytest.mark.parametrize("name", CASES)
def test_fixture_counts_and_definitions(name):
    """The cases exercise what they are meant to, and the fixture's layers are the issue's
    definitions: depth == distance bit for bit on sphere hits, depth = t * |d| on walls, unit
    normals within 1 float ulp, inf / zeros / -1 on misses."""
    prims, cam, exp = afx.case(name)
    miss, sph, wall = afx.counts(exp)
    if name in afx.COUNTS:
        assert (miss, sph, wall) == afx.COUNTS[name]
    else:
        from views_fixture import Views
        tilted = Views().tilted_walls(afx.VIEWS_SCENE)
        assert miss > 100 and int(np.isin(exp["index"], tilted).sum()) > 100
        fresh = capi.camera_init(**Views().cam_args(afx.VIEWS_VIEW))
        assert tuple(fresh.image_top_left[:]) == tuple(cam.image_top_left[:])   # stale on purpose
        assert tuple(fresh.position[:]) != tuple(cam.position[:])
    assert miss + sph + wall == cam.width * cam.height
    k, hit = exp["kind"], exp["hit"]
    assert afx.same_bytes(exp["index"], hit["index"])
    s, w, m = k == 0, k == 1, k == -1
    assert afx.same_bytes(exp["depth"][s], hit["distance"][s].astype(np.float32))
    _, d = afx.sfx.camera_rays(cam)
    dlen = np.sqrt((d * d).sum(axis=1)).reshape(k.shape)
    assert np.allclose(exp["depth"][w], hit["distance"][w] * dlen[w], rtol=1e-6)
    assert np.isposinf(exp["depth"][m]).all() and np.isfinite(exp["depth"][~m]).all()
    assert (exp["depth"][~m] > 0).all()
    n2 = (exp["normal"].astype(np.float64) ** 2).sum(axis=-1)
    assert (np.abs(np.sqrt(n2[~m]) - 1.0) <= np.finfo(np.float32).eps).all()
    for layer in ("normal", "albedo"):
        assert not exp[layer][m].any() and not np.signbit(exp[layer][m]).any()
    assert (exp["index"][m] == -1).all() and (hit["distance"][m] == afx.DBL_MAX).all()
    colors = np.array([p.mat.color[:] for p in prims], np.float32)
    assert afx.same_bytes(exp["albedo"][~m], colors[exp["index"][~m]])


def test_fixture_hits_equal_the_references_recorded_hits(oracle, golden_rays):
    """The fixture's records for the golden rays are the reference's own (ray_hits.npz): index,
    distance and normal bit for bit, so the expectation rests on the reference."""
    rec = np.load(os.path.join(GOLDEN, "ray_hits.npz"))
    nhit = 0
    for name in ("default", "s8w4", "s64w6"):
        prims = scenes.to_prims(scene_by_name(name))
        hits = afx.closest_hits(oracle, prims, golden_rays[f"{name}__o"], golden_rays[f"{name}__d"])
        assert np.array_equal(hits["index"], rec[f"{name}__index"])
        assert afx.same_bytes(hits["distance"], rec[f"{name}__dist"])
        assert afx.same_bytes(hits["normal"], rec[f"{name}__normal"])
        assert not hits["reserved"].any()
        nhit += int((hits["index"] >= 0).sum())
    assert nhit > 100
