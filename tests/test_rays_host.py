"""CPU-side checks of the ray-query additions to the C-ABI (rt_hit, rt_trace_rays,
rt_trace_rays_device): record layout, exports, argument checks that need no device, and the
oracle's find_closest_hit pinned bit for bit to the reference's own (tests/golden/
ray_hits.npz, recorded by tests/golden/make_ray_hits.py from the reference's compiled
find_closest_hit for the rays of rays.npz)."""
import ctypes as C
import os
import re
import subprocess

import numpy as np

from conftest import GOLDEN, REPO, scene_by_name
from rtamd import capi, scenes


def test_rt_hit_layout():
    assert C.sizeof(capi.rt_hit) == 40
    assert capi.rt_hit.distance.offset == 0
    assert capi.rt_hit.normal.offset == 8
    assert capi.rt_hit.index.offset == 32
    assert capi.rt_hit.reserved.offset == 36
    dt = capi.HIT_DTYPE
    assert dt.itemsize == 40
    assert [dt.fields[k][1] for k in ("distance", "normal", "index", "reserved")] == [0, 8, 32, 36]
    # a numpy record array is an array of rt_hit
    a = np.zeros(3, dt)
    a["distance"] = [1.5, 2.5, 3.5]
    a["index"] = [7, -1, 2]
    a["normal"][1] = (1.0, 2.0, 3.0)
    h = (capi.rt_hit * 3).from_buffer_copy(a.tobytes())
    assert [x.distance for x in h] == [1.5, 2.5, 3.5] and [x.index for x in h] == [7, -1, 2]
    assert list(h[1].normal) == [1.0, 2.0, 3.0]


def test_header_declares_the_record_and_both_entry_points():
    text = open(os.path.join(REPO, "include", "rt_capi.h")).read()
    assert re.search(r"typedef struct rt_hit \{", text)
    assert "#define RT_CAPI_VERSION 2" in text
    for name in ("rt_trace_rays", "rt_trace_rays_device"):
        assert re.search(r"\bint " + name + r"\(rt_ctx\*", text), name


def test_library_exports_both_entry_points():
    lib = capi.load()
    assert hasattr(lib, "rt_trace_rays") and hasattr(lib, "rt_trace_rays_device")
    out = subprocess.run(["nm", "-D", "--defined-only", capi.LIB_PATH], capture_output=True,
                         text=True, check=True).stdout
    exported = set(re.findall(r" T (rt_[a-z0-9_]+)$", out, flags=re.M))
    assert {"rt_trace_rays", "rt_trace_rays_device"} <= exported
    bound = {n for n, _, _ in capi.SIGNATURES}
    assert {"rt_trace_rays", "rt_trace_rays_device"} <= bound


def test_null_ctx_rejected_without_device():
    lib = capi.load()
    o = (C.c_double * 3)(0, 0, 0)
    d = (C.c_double * 3)(1, 0, 0)
    rgb = (C.c_double * 3)()
    assert lib.rt_trace_rays(None, o, d, 1, 0, capi.RT_PREC_F64, 0, capi.RT_OUT_RGB_F64,
                             C.cast(rgb, C.c_void_p), None, 0, None) == capi.RT_ERR_INVALID_ARG
    assert lib.rt_trace_rays_device(None, None, None, 1, 0, capi.RT_PREC_F64, 0,
                                    capi.RT_OUT_RGB_F64, None, None, None,
                                    None) == capi.RT_ERR_INVALID_ARG


def test_oracle_find_closest_hit_bit_exact_vs_reference(oracle, golden_rays):
    """The oracle's hit record equals the reference's on all 1,200 fixture rays — index,
    distance and normal bit for bit, every miss placeholder included (as
    test_rays_bit_exact pins the oracle's radiance)."""
    hits = np.load(os.path.join(GOLDEN, "ray_hits.npz"))
    nhit = 0
    for name in ("default", "s8w4", "s64w6"):
        prims = scenes.to_prims(scene_by_name(name))
        o, d = golden_rays[f"{name}__o"], golden_rays[f"{name}__d"]
        idx, dist, nrm = hits[f"{name}__index"], hits[f"{name}__dist"], hits[f"{name}__normal"]
        assert len(o) == len(idx) == 400
        for k in range(len(o)):
            gi, gd, gn = oracle.find_closest_hit(prims, o[k], d[k])
            assert gi == int(idx[k]), (name, k)
            assert np.float64(gd).tobytes() == dist[k].tobytes(), (name, k)
            assert np.asarray(gn, np.float64).tobytes() == nrm[k].tobytes(), (name, k)
        miss = idx < 0
        assert (dist[miss] == np.finfo(np.float64).max).all()
        assert not nrm[miss].any() and not np.signbit(nrm[miss]).any()
        nhit += int((~miss).sum())
    assert nhit > 100   # the fixture exercises hits, not only the placeholder
