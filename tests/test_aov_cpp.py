"""The C++ mirror's frame AOVs (include/rt/scene.h: rt_scene_aov): host code links to the built
libraries; on the GPU its bytes equal the expectation of tests/aov_fixture.py."""
import os
import subprocess

import numpy as np
import pytest

import aov_fixture as afx
from conftest import REPO, has_gpu
from rtamd import capi, scenes

LIB = os.path.join(REPO, "ray-tracer-from-scratch_amd", "lib")
BIN = os.path.join(REPO, "tests", "cpp", "aov_main")


@pytest.fixture(scope="module")
def aov_main():
    src = os.path.join(REPO, "tests", "cpp", "aov_main.cpp")
    if not os.path.exists(BIN) or os.path.getmtime(BIN) < os.path.getmtime(src):
        subprocess.run(["g++", "-std=c++17", "-O2", "-I", os.path.join(REPO, "include"), src,
                        "-o", BIN, "-L", LIB, "-lrt_host", "-lrt_amd", f"-Wl,-rpath,{LIB}"],
                       check=True)
    return BIN


def test_aov_rejects_a_primitive_without_gpu_record(aov_main):
    """A SceneGeometry subclass that has no pack() makes rt_scene_aov throw
    std::invalid_argument before any device work (CPU)."""
    out = subprocess.run([aov_main, "plugin"], capture_output=True, text=True, check=True).stdout
    lines = out.strip().splitlines()
    assert len(lines) == 1
    assert lines[0].startswith("1 ") and "unsupported primitive" in lines[0], out


@pytest.mark.gpu
@pytest.mark.skipif(not has_gpu(), reason="needs a HIP device")
def test_cpp_aov_matches_expectation(aov_main, oracle):
    out = subprocess.run([aov_main, "frame"], capture_output=True, text=True, check=True).stdout
    lines = out.strip().splitlines()
    head = lines[0].split()
    assert len(head) == 14
    W, H = int(head[12]), int(head[13])
    assert (W, H) == (16, 12) and len(lines) == 1 + W * H
    c = [float.fromhex(x) for x in head[:12]]
    cam = capi.rt_camera((capi.C.c_double * 3)(*c[0:3]), (capi.C.c_double * 3)(*c[3:6]),
                         (capi.C.c_double * 3)(*c[6:9]), (capi.C.c_double * 3)(*c[9:12]), W, H)
    rows = [ln.split() for ln in lines[1:]]
    assert all(len(r) == 12 for r in rows)
    v = np.array([[float.fromhex(x) for x in r[1:]] for r in rows])
    got = np.zeros(W * H, capi.HIT_DTYPE)
    got["index"] = [int(r[0]) for r in rows]
    got["distance"], got["normal"] = v[:, 0], v[:, 1:4]
    exp = afx.expected(oracle, scenes.to_prims(scenes.default_scene()), cam)
    assert afx.same_bytes(got.reshape(H, W), exp["hit"])
    assert afx.same_bytes(v[:, 4].astype(np.float32).reshape(H, W), exp["depth"])
    assert afx.same_bytes(v[:, 5:8].astype(np.float32).reshape(H, W, 3), exp["normal"])
    assert afx.same_bytes(v[:, 8:11].astype(np.float32).reshape(H, W, 3), exp["albedo"])
    miss, sph, wall = afx.counts(exp)
    assert miss > 0 and sph > 0 and wall > 0   # the three outcomes occur


@pytest.mark.gpu
@pytest.mark.skipif(not has_gpu(), reason="needs a HIP device")
def test_rt_frames_aov_option(tmp_path, oracle):
    """rt_frames --aov PREFIX writes the first frame's depth and index layers as raw files:
    main.cpp:146-153's camera (aspect 4 / 3 evaluated as the integer 1) at 24 x 24 on the
    default scene."""
    rt_frames = os.path.join(REPO, "ray-tracer-from-scratch_amd", "bin", "rt_frames")
    prefix = tmp_path / "gbuf"
    out = subprocess.run([rt_frames, "--frames", "1", "--width", "24", "--depth", "2", "--aov", str(prefix)],
                         capture_output=True, text=True, check=True).stdout
    assert "Number of frames: 1" in out
    cam = capi.camera_init(position=(0, 0, 0), lookat=(-1, 0, 0), vup=(0, 0, -1), vfov=90,
                           aspect_ratio=1.0, image_width=24.0)
    exp = afx.expected(oracle, scenes.to_prims(scenes.default_scene()), cam)
    depth = np.fromfile(str(prefix) + ".depth.f32", np.float32).reshape(24, 24)
    index = np.fromfile(str(prefix) + ".index.i32", np.int32).reshape(24, 24)
    assert afx.same_bytes(index, exp["index"]) and afx.same_bytes(depth, exp["depth"])
    miss, sph, wall = afx.counts(exp)
    assert miss > 0 and sph > 0 and wall > 0
