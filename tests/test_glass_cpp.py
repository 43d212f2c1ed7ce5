"""Transmission records through the C++ mirror (include/rt/scene.h) and the headless frame loop:
rt_scene and rt_radiance with RtSceneOptions::transmission give the C-ABI's bytes under
rt_set_transmission, with and without RT_FLAG_SHADOWS; an empty vector takes the records away
again; a vector of the wrong size throws; rt_frames --glass renders a different picture."""
import os
import subprocess

import numpy as np
import pytest

import glass_fixture as gfx
from conftest import REPO, has_gpu
from rtamd import capi

pytestmark = [pytest.mark.gpu,
              pytest.mark.skipif(not has_gpu(), reason="needs a HIP device")]

LIB = os.path.join(REPO, "ray-tracer-from-scratch_amd", "lib")
BIN = os.path.join(REPO, "tests", "cpp", "glass_main")
RT_FRAMES = os.path.join(REPO, "ray-tracer-from-scratch_amd", "bin", "rt_frames")
SH = capi.RT_FLAG_SHADOWS


@pytest.fixture(scope="module")
def glass_main():
    src = os.path.join(REPO, "tests", "cpp", "glass_main.cpp")
    if not os.path.exists(BIN) or os.path.getmtime(BIN) < os.path.getmtime(src):
        subprocess.run(["g++", "-std=c++17", "-O2", "-I", os.path.join(REPO, "include"), src,
                        "-o", BIN, "-L", LIB, "-lrt_host", "-lrt_amd", f"-Wl,-rpath,{LIB}"],
                       check=True)
    return BIN


@pytest.mark.parametrize("flags", [0, SH])
def test_rt_scene_with_records_equals_the_capi_frame(glass_main, flags):
    W, H = 44, 33
    raw = subprocess.run([glass_main, "render", str(W), str(H), str(flags)], capture_output=True,
                         check=True).stdout
    v = np.frombuffer(raw, dtype=np.float64)
    n = H * W * 3
    assert v.size == 12 + 2 * n
    cam = capi.rt_camera()
    for k in range(3):
        cam.position[k], cam.image_top_left[k] = v[k], v[3 + k]
        cam.pixel_delta_x[k], cam.pixel_delta_y[k] = v[6 + k], v[9 + k]
    cam.width, cam.height = W, H
    prims, trans = gfx.scene("G")
    with capi.Renderer(0) as r:
        r.set_scene(prims)
        plain, _ = r.render(cam, 3, capi.RT_PREC_F64, flags, capi.RT_OUT_RGB_F64)
        r.set_transmission(trans)
        want, _ = r.render(cam, 3, capi.RT_PREC_F64, flags, capi.RT_OUT_RGB_F64)
    assert v[12:12 + n].tobytes() == want.tobytes()
    assert v[12 + n:].tobytes() == plain.tobytes()
    assert want.tobytes() != plain.tobytes()


def test_rt_radiance_honours_the_records(glass_main):
    prims, trans = gfx.scene("G")
    for flags in (0, SH):
        out = subprocess.run([glass_main, "radiance", str(flags)], capture_output=True, text=True,
                             check=True).stdout
        rows = np.array([[float.fromhex(x) for x in ln.split()] for ln in out.strip().splitlines()])
        assert rows.shape == (64, 9)
        o, d = np.ascontiguousarray(rows[:, 0:3]), np.ascontiguousarray(rows[:, 3:6])
        with capi.Renderer(0) as r:
            r.set_scene(prims)
            plain, _, _ = r.trace_rays(o, d, 3, capi.RT_PREC_F64, flags)
            r.set_transmission(trans)
            want, _, _ = r.trace_rays(o, d, 3, capi.RT_PREC_F64, flags)
        assert np.ascontiguousarray(rows[:, 6:]).tobytes() == want.tobytes()
        assert np.abs(want - plain).max() > 1e-3


def test_a_vector_of_the_wrong_size_throws(glass_main):
    assert subprocess.run([glass_main, "mismatch"], capture_output=True).returncode == 0


def test_rt_frames_glass_option(tmp_path):
    pics = {}
    for name, extra in (("plain", []),
                        ("glass", ["--glass", "0,.85", "--glass", "9,.6,1"]),
                        ("glass_sh", ["--glass", "0,.85,1.33", "--glass", "9,.6,1", "--shadows"]),
                        ("surface", ["--glass", "0,.85", "--glass", "9,.6,1", "--gpu-surface"])):
        ppm = tmp_path / f"{name}.ppm"
        out = subprocess.run([RT_FRAMES, "--frames", "2", "--width", "64", "--depth", "3", "--scene",
                              "synthetic:8,4", "--ppm", str(ppm)] + extra, capture_output=True,
                             text=True, check=True).stdout
        assert "Number of frames: 2" in out
        pics[name] = ppm.read_bytes()
    assert len(set(len(p) for p in pics.values())) == 1
    assert pics["plain"] != pics["glass"] != pics["glass_sh"] != pics["plain"]
    assert pics["surface"] != pics["plain"]
    for bad in (["--glass", "1"], ["--glass", "99,.5"], ["--glass", "-1,.5"]):
        res = subprocess.run([RT_FRAMES, "--frames", "1", "--scene", "synthetic:8,4"] + bad,
                             capture_output=True, text=True)
        assert res.returncode == 2, bad
