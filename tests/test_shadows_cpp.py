"""RT_FLAG_SHADOWS through the C++ mirror (include/rt/scene.h) and the headless frame loop:
rt_scene with RtSceneOptions::flags = RT_FLAG_SHADOWS gives the C-ABI's flagged frame,
rt_radiance honours the flag, and rt_frames --shadows renders a different picture."""
import os
import subprocess

import numpy as np
import pytest

import shadow_fixture as sfx
from conftest import REPO, has_gpu
from rtamd import capi, scenes

pytestmark = [pytest.mark.gpu,
              pytest.mark.skipif(not has_gpu(), reason="needs a HIP device")]

LIB = os.path.join(REPO, "ray-tracer-from-scratch_amd", "lib")
BIN = os.path.join(REPO, "tests", "cpp", "shadows_main")
RT_FRAMES = os.path.join(REPO, "ray-tracer-from-scratch_amd", "bin", "rt_frames")
SH = capi.RT_FLAG_SHADOWS


@pytest.fixture(scope="module")
def shadows_main():
    src = os.path.join(REPO, "tests", "cpp", "shadows_main.cpp")
    if not os.path.exists(BIN) or os.path.getmtime(BIN) < os.path.getmtime(src):
        subprocess.run(["g++", "-std=c++17", "-O2", "-I", os.path.join(REPO, "include"), src,
                        "-o", BIN, "-L", LIB, "-lrt_host", "-lrt_amd", f"-Wl,-rpath,{LIB}"],
                       check=True)
    return BIN


def shadow_scene():
    """shadows_main.cpp's scene."""
    M, S, W = scenes.Material, scenes.Sphere, scenes.Wall
    return scenes.to_prims([
        S(M((0, 1, 0), 0.5), (1.5, 0, 0), .5),
        W(M((0, 0, 1)), (3.0, 2, 0), (0, -1, 0), 1, 1),
        W(M((0, 1, 0)), (3.0, -3, 0), (0, 1, 0), 2, 2),
        S(M((1, 0, 0), 0.25), (2.0, -1.5, 0.5), .6),
    ])


def test_rt_scene_with_the_flag_equals_the_capi_frame(shadows_main):
    W, H = 44, 33
    raw = subprocess.run([shadows_main, "render", str(W), str(H), str(SH)], capture_output=True,
                         check=True).stdout
    v = np.frombuffer(raw, dtype=np.float64)
    assert v.size == 12 + H * W * 3
    cam = capi.rt_camera()
    for k in range(3):
        cam.position[k], cam.image_top_left[k] = v[k], v[3 + k]
        cam.pixel_delta_x[k], cam.pixel_delta_y[k] = v[6 + k], v[9 + k]
    cam.width, cam.height = W, H
    with capi.Renderer(0) as r:
        r.set_scene(shadow_scene())
        plain, _ = r.render(cam, 3, capi.RT_PREC_F64, 0, capi.RT_OUT_RGB_F64)
        want, _ = r.render(cam, 3, capi.RT_PREC_F64, SH, capi.RT_OUT_RGB_F64)
    assert v[12:].tobytes() == want.tobytes()
    assert want.tobytes() != plain.tobytes()


def test_rt_radiance_honours_the_flag(shadows_main, oracle):
    rows = {}
    for flags in (0, SH):
        out = subprocess.run([shadows_main, "radiance", str(flags)], capture_output=True, text=True,
                             check=True).stdout
        rows[flags] = np.array([[float.fromhex(x) for x in ln.split()]
                                for ln in out.strip().splitlines()])
        assert rows[flags].shape == (64, 9)
    o, d = rows[SH][:, 0:3], rows[SH][:, 3:6]
    assert rows[0][:, :6].tobytes() == rows[SH][:, :6].tobytes()
    prims = shadow_scene()
    on = sfx.trace(oracle, prims, o, d, 3, True)
    off = sfx.trace(oracle, prims, o, d, 3, False)
    ok = ~on.fragile
    assert on.shadow.any() and ok.sum() >= 60
    assert np.abs(rows[SH][:, 6:] - on.rgb)[ok].max() <= 1e-12
    assert np.abs(rows[0][:, 6:] - off.rgb).max() <= 1e-12
    assert np.abs(on.rgb - off.rgb).max() > 1e-3


def test_rt_frames_shadows_option(tmp_path):
    pics = {}
    for name, extra in (("plain", []), ("shadows", ["--shadows"])):
        ppm = tmp_path / f"{name}.ppm"
        out = subprocess.run([RT_FRAMES, "--frames", "2", "--width", "64", "--depth", "3", "--scene",
                              "synthetic:8,4", "--ppm", str(ppm)] + extra, capture_output=True,
                             text=True, check=True).stdout
        assert "Number of frames: 2" in out
        pics[name] = ppm.read_bytes()
    assert len(pics["plain"]) == len(pics["shadows"]) and pics["plain"] != pics["shadows"]
