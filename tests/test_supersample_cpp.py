"""RtSceneOptions::supersample of the C++ mirror (include/rt/scene.h): rt_scene with
supersample = 2 gives the C-ABI's S = 2 F64 frame; combined with several devices it throws
std::invalid_argument before any device work."""
import os
import subprocess

import numpy as np
import pytest

from conftest import REPO, has_gpu
from rtamd import capi, scenes

LIB = os.path.join(REPO, "ray-tracer-from-scratch_amd", "lib")
BIN = os.path.join(REPO, "tests", "cpp", "supersample_main")


@pytest.fixture(scope="module")
def ss_main():
    src = os.path.join(REPO, "tests", "cpp", "supersample_main.cpp")
    if not os.path.exists(BIN) or os.path.getmtime(BIN) < os.path.getmtime(src):
        subprocess.run(["g++", "-std=c++17", "-O2", "-I", os.path.join(REPO, "include"), src,
                        "-o", BIN, "-L", LIB, "-lrt_host", "-lrt_amd", f"-Wl,-rpath,{LIB}"],
                       check=True)
    return BIN


@pytest.mark.parametrize("s,n", [(2, 2), (4, 3), (3, 0)])
def test_supersample_with_several_devices_throws(ss_main, s, n):
    """No device needed: the options are refused before the renderer is made.  (3 is no valid
    factor, refused the same way on the one-GPU renderer.)"""
    out = subprocess.run([ss_main, "tiled", str(s), str(n)], capture_output=True, text=True,
                         check=True).stdout
    assert out.startswith("1 ") and "supersample" in out, out


@pytest.mark.gpu
@pytest.mark.skipif(not has_gpu(), reason="needs a HIP device")
def test_rt_scene_supersample_equals_the_capi_frame(ss_main):
    W, H, S = 44, 33, 2
    raw = subprocess.run([ss_main, "render", str(W), str(H), str(S)], capture_output=True,
                         check=True).stdout
    v = np.frombuffer(raw, dtype=np.float64)
    assert v.size == 12 + H * W * 3
    cam = capi.rt_camera()
    for k in range(3):
        cam.position[k], cam.image_top_left[k] = v[k], v[3 + k]
        cam.pixel_delta_x[k], cam.pixel_delta_y[k] = v[6 + k], v[9 + k]
    cam.width, cam.height = W, H
    with capi.Renderer(0) as r:
        r.set_scene(scenes.to_prims(scenes.default_scene()))
        plain, _ = r.render(cam, 10, capi.RT_PREC_F64, 0, capi.RT_OUT_RGB_F64)
        r.set_option(capi.RT_OPT_SUPERSAMPLE, S)
        want, _ = r.render(cam, 10, capi.RT_PREC_F64, 0, capi.RT_OUT_RGB_F64)
    assert v[12:].tobytes() == want.tobytes()
    assert want.tobytes() != plain.tobytes()
