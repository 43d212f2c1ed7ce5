"""The C++ mirror's ambient occlusion frames (include/rt/scene.h: rt_scene_ao) and
rt_frames --ao: host code links to the built libraries; on the GPU their bytes equal the
expectation of tests/ao_fixture.py."""
import os
import subprocess

import numpy as np
import pytest

import ao_fixture as aofx
import aov_fixture as afx
from conftest import REPO, has_gpu
from rtamd import capi, scenes

LIB = os.path.join(REPO, "ray-tracer-from-scratch_amd", "lib")
BIN = os.path.join(REPO, "tests", "cpp", "ao_main")
K = 16   # the default scene is sparse: only probes without a limit find a blocker


@pytest.fixture(scope="module")
def ao_main():
    src = os.path.join(REPO, "tests", "cpp", "ao_main.cpp")
    if not os.path.exists(BIN) or os.path.getmtime(BIN) < os.path.getmtime(src):
        subprocess.run(["g++", "-std=c++17", "-O2", "-I", os.path.join(REPO, "include"), src,
                        "-o", BIN, "-L", LIB, "-lrt_host", "-lrt_amd", f"-Wl,-rpath,{LIB}"],
                       check=True)
    return BIN


def test_header_declares_the_mirror():
    text = open(os.path.join(REPO, "include", "rt", "scene.h")).read()
    assert "RtAo rt_scene_ao(std::vector<vec3> u" in text and "struct RtAo {" in text


def covered(e, radius):
    """The frame exercises something: hits, misses and occluded probes."""
    c = e.count(radius)
    return e.hitmask.any() and (~e.hitmask).any() and c.any() and (c[e.hitmask] == 0).any()


@pytest.mark.gpu
@pytest.mark.skipif(not has_gpu(), reason="needs a HIP device")
def test_cpp_ao_matches_expectation(ao_main):
    for radius, arg in ((1.5, "1.5"), (np.inf, "inf")):
        out = subprocess.run([ao_main, "frame", str(K), arg], capture_output=True, text=True,
                             check=True).stdout
        lines = out.strip().splitlines()
        head = lines[0].split()
        assert len(head) == 14
        W, H = int(head[12]), int(head[13])
        assert (W, H) == (16, 12) and len(lines) == 1 + K + W * H
        c = [float.fromhex(x) for x in head[:12]]
        cam = capi.rt_camera((capi.C.c_double * 3)(*c[0:3]), (capi.C.c_double * 3)(*c[3:6]),
                             (capi.C.c_double * 3)(*c[6:9]), (capi.C.c_double * 3)(*c[9:12]), W, H)
        dirs = np.array([[float.fromhex(x) for x in ln.split()] for ln in lines[1:1 + K]])
        assert afx.same_bytes(dirs, capi.ao_directions(K))
        rows = [ln.split() for ln in lines[1 + K:]]
        count = np.array([int(r[0]) for r in rows], np.uint8).reshape(H, W)
        ao = np.array([float.fromhex(r[1]) for r in rows]).astype(np.float32).reshape(H, W)
        e = aofx.build(scenes.to_prims(scenes.default_scene()), cam, dirs)
        exp = e.layers(radius)
        assert afx.same_bytes(count, exp["count"]) and afx.same_bytes(ao, exp["ao"])
        assert covered(e, radius) == (radius == np.inf)


@pytest.mark.gpu
@pytest.mark.skipif(not has_gpu(), reason="needs a HIP device")
def test_cpp_ao_refuses_invalid_probes(ao_main):
    """No directions, 65 directions, a zero direction and radius 0 throw std::runtime_error with
    the C-ABI's status; a primitive without pack() throws std::invalid_argument; so does
    rt_ao_direction_set(65) (runtime_error)."""
    out = subprocess.run([ao_main, "refuse"], capture_output=True, text=True, check=True).stdout
    lines = out.strip().splitlines()
    assert len(lines) == 6, out
    assert all(ln.startswith("1 runtime_error") for ln in lines[:4] + lines[5:]), out
    assert lines[4].startswith("1 invalid_argument") and "unsupported primitive" in lines[4], out


@pytest.mark.gpu
@pytest.mark.skipif(not has_gpu(), reason="needs a HIP device")
def test_rt_frames_ao_option(tmp_path):
    """rt_frames --ao PREFIX --ao-dirs K --ao-radius R writes the first frame's two layers as raw
    files: main.cpp:146-153's camera (aspect 4 / 3 evaluated as the integer 1) at 24 x 24 on the
    default scene."""
    rt_frames = os.path.join(REPO, "ray-tracer-from-scratch_amd", "bin", "rt_frames")
    prefix = tmp_path / "occ"
    out = subprocess.run([rt_frames, "--frames", "1", "--width", "24", "--depth", "2", "--ao", str(prefix),
                          "--ao-dirs", str(K), "--ao-radius", "inf"],
                         capture_output=True, text=True, check=True).stdout
    assert "Number of frames: 1" in out
    cam = capi.camera_init(position=(0, 0, 0), lookat=(-1, 0, 0), vup=(0, 0, -1), vfov=90,
                           aspect_ratio=1.0, image_width=24.0)
    e = aofx.build(scenes.to_prims(scenes.default_scene()), cam, capi.ao_directions(K))
    exp = e.layers(np.inf)
    ao = np.fromfile(str(prefix) + ".ao.f32", np.float32).reshape(24, 24)
    count = np.fromfile(str(prefix) + ".count.u8", np.uint8).reshape(24, 24)
    assert afx.same_bytes(count, exp["count"]) and afx.same_bytes(ao, exp["ao"])
    assert covered(e, np.inf)
