"""CPU-side checks of ambient occlusion frames (rt_render_ao, rt_render_ao_device,
rt_ao_directions): declarations, struct sizes, exports and bindings, the default direction set's
properties, the argument checks that need no device, and the expected-result fixture
(tests/ao_fixture.py): the coverage condition of every (case, direction set, radius) the GPU
tests use, and lone convex scenes, where nothing can be occluded."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import ao_fixture as aofx
from conftest import REPO
from rtamd import capi, scenes

NAMES = ("rt_render_ao", "rt_render_ao_device", "rt_ao_directions")


def test_header_declares_entry_points_and_structs():
    text = open(os.path.join(REPO, "include", "rt_capi.h")).read()
    assert "#define RT_CAPI_VERSION 2" in text
    assert re.search(r"^#define RT_AO_MAX_DIRS 64$", text, flags=re.M) and capi.RT_AO_MAX_DIRS == 64
    for name in NAMES[:2]:
        assert re.search(r"\bint " + name + r"\(rt_ctx\*", text), name
    assert re.search(r"\bint rt_ao_directions\(int32_t n, double\* out\);", text)
    for struct, binding, fields, size in (
            ("rt_ao_params", capi.rt_ao_params, ["dirs", "ndirs", "reserved", "radius", "reserved2"], 32),
            ("rt_ao_buffers", capi.rt_ao_buffers, ["count", "ao", "reserved"], 24)):
        m = re.search(r"typedef struct " + struct + r" \{(.*?)\} " + struct + ";", text, flags=re.S)
        assert m, struct
        got = re.findall(r"^\s*(?:const )?[a-z0-9_]+\*?\s+([a-z0-9]+);", m.group(1), flags=re.M)
        assert got == fields, (struct, got)
        assert [f for f, _ in binding._fields_] == fields
        assert C.sizeof(binding) == size
    assert capi.rt_ao_params.radius.offset == 16 and capi.rt_ao_buffers.ao.offset == 8


def test_library_exports_and_bindings():
    lib = capi.load()
    out = subprocess.run(["nm", "-D", "--defined-only", capi.LIB_PATH], capture_output=True,
                         text=True, check=True).stdout
    exported = set(re.findall(r" T (rt_[a-z0-9_]+)$", out, flags=re.M))
    assert set(NAMES) <= exported
    assert set(NAMES) <= {n for n, _, _ in capi.SIGNATURES}
    for name in NAMES:
        assert getattr(lib, name).restype is C.c_int
    assert callable(capi.Renderer.render_ao) and callable(capi.Renderer.render_ao_device)
    assert callable(capi.ao_directions)
    assert dict(capi.AO_LAYERS) == {"count": np.uint8, "ao": np.float32}
    assert tuple(capi.AO_LAYERS) == ("count", "ao")


@pytest.mark.parametrize("n", [1, 2, 3, 16, 63, 64])
def test_directions_are_a_spread_set_of_unit_vectors(n):
    d = capi.ao_directions(n)
    assert d.shape == (n, 3) and d.dtype == np.float64 and np.isfinite(d).all()
    assert (np.abs(np.sqrt((d * d).sum(axis=1)) - 1.0) <= 1e-15).all()
    assert d.any(axis=1).all()                      # no (0, 0, 0)
    k = np.arange(n)
    assert np.allclose(d[:, 2], 1 - (2 * k + 1) / n, rtol=0, atol=1e-15)   # the z ladder
    phi = k * np.pi * (3 - np.sqrt(5))
    r = np.sqrt(1 - d[:, 2] ** 2)
    assert np.allclose(d[:, 0], r * np.cos(phi), atol=1e-12) and np.allclose(d[:, 1], r * np.sin(phi), atol=1e-12)
    # the set covers the whole sphere evenly: its mean is short (the z ladder sums to 0 exactly,
    # the spiral's x and y cancel up to O(1 / sqrt(n)))
    assert np.linalg.norm(d.mean(axis=0)) <= 1.0 / n + (0.05 if n >= 16 else 1.0)
    if n >= 16:
        assert len(np.unique(np.round(d, 12), axis=0)) == n


def test_direction_count_outside_range_refused():
    lib = capi.load()
    buf = np.full(3 * 66, 7.0)
    p = buf.ctypes.data_as(C.POINTER(C.c_double))
    for n in (0, -1, 65, 2**31 - 1, -2**31):
        assert lib.rt_ao_directions(n, p) == capi.RT_ERR_INVALID_ARG
    assert lib.rt_ao_directions(4, None) == capi.RT_ERR_INVALID_ARG
    assert (buf == 7.0).all()
    with pytest.raises(capi.RTError):
        capi.ao_directions(65)
    assert lib.rt_ao_directions(64, p) == capi.RT_OK and (buf[192:] == 7.0).all()


def test_null_ctx_rejected_without_device():
    lib = capi.load()
    cam = capi.camera_init(**aofx.afx.sfx.CAM_B13)
    cnt = np.full(4, 7, np.uint8)
    ao = np.full(4, 7.0, np.float32)
    dirs = capi.ao_directions(4)
    prm = capi.rt_ao_params(dirs.ctypes.data_as(C.POINTER(C.c_double)), 4, 0, 1.0, None)
    bufs = capi.rt_ao_buffers(count=cnt.ctypes.data, ao=ao.ctypes.data)
    st = capi.rt_stats()
    assert lib.rt_render_ao(None, C.byref(cam), 0, 1, C.byref(prm), C.byref(bufs),
                            C.byref(st)) == capi.RT_ERR_INVALID_ARG
    assert lib.rt_render_ao_device(None, C.byref(cam), 0, 1, C.byref(prm), C.byref(bufs),
                                   None) == capi.RT_ERR_INVALID_ARG
    assert (cnt == 7).all() and (ao == 7.0).all()


@pytest.mark.parametrize("name,k", aofx.GPU_CASES)
def test_coverage_condition(name, k):
    """Every (case, direction set, radius) of the GPU tests exercises partial occlusion, both
    kinds of blocker and — in the views case — walls seen from behind."""
    e = aofx.case(name, k)
    nhit = int(e.hitmask.sum())
    assert nhit > 30
    for radius in aofx.RADII:
        c = e.coverage(radius)
        print("ao coverage", name, "K", k, "radius", radius, "hit pixels", nhit,
              "0<count<K %.3f" % c["partial"], "sphere / wall blockers", c["sphere_blockers"],
              c["wall_blockers"], "behind", c["behind"], "histogram", c["hist"].tolist())
        assert c["hist"].sum() == nhit
        assert c["partial"] >= 0.05
        assert c["sphere_blockers"] > 0 and c["wall_blockers"] > 0
        if name == "views":
            assert c["behind"] > 0
        lay = e.layers(radius)
        assert (lay["count"][~e.hitmask] == 0).all() and (lay["ao"][~e.hitmask] == 1.0).all()
        assert lay["count"].max() <= k and lay["ao"].dtype == np.float32
    # a longer probe sees no less
    assert (e.count(aofx.RADII[0]) <= e.count(aofx.RADII[1])).all()


def _prim_sphere():
    p = scenes.to_prims(scenes.synthetic_scene(1, 0, seed=1234))
    assert len(p) == 1 and p[0].kind != capi.RT_PRIM_WALL
    return p


def _prim_wall():
    p = [q for q in scenes.to_prims(scenes.synthetic_scene(0, 4, seed=1234))
         if q.kind == capi.RT_PRIM_WALL][:1]
    assert len(p) == 1
    return p


def test_lone_convex_scenes_are_open_everywhere():
    """A lone sphere and a lone wall (seen from either side) occlude nothing: the probes leave
    the surface into the viewer's half space and the hit object itself never blocks them."""
    dirs = capi.ao_directions(16)
    sph = _prim_sphere()
    c = np.array(sph[0].position[:])
    pos = c + float(sph[0].radius) * np.array([3.0, 0.4, 0.2])
    # (main.cpp:133: a pixel's ray points from the pixel through the camera, away from lookat)
    cam = capi.camera_init(position=tuple(pos), lookat=tuple(2 * pos - c), vup=(0, 0, -1),
                           vfov=60, aspect_ratio=1.5, image_width=24)
    e = aofx.build(sph, cam, dirs)
    assert e.hitmask.sum() > 20 and not e.count(np.inf).any()
    wall = _prim_wall()
    P, n = np.array(wall[0].position[:]), np.array(wall[0].normal[:])
    seen = []
    for side in (1.0, -1.0):
        mid = P   # a corner of the wall: half of the frame sees it, the rest misses
        pos = mid + side * 3.0 * n / np.linalg.norm(n) + [0.1, 0.2, 0.3]
        cam = capi.camera_init(position=tuple(pos), lookat=tuple(2 * pos - mid), vup=(0.3, 0.2, -1),
                               vfov=60, aspect_ratio=1.5, image_width=24)
        e = aofx.build(wall, cam, dirs)
        assert e.hitmask.sum() > 20 and not e.count(np.inf).any()
        seen.append(bool((e.f > 0).all()) if len(e.f) else None)
    assert sorted(seen) == [False, True]   # once from the front, once from behind
