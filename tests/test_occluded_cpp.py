"""The C++ mirror's occlusion query (include/rt/scene.h: rt_occluded): host code links to the
built libraries; on the GPU its bytes equal the expectation of tests/occluded_fixture.py."""
import os
import subprocess

import numpy as np
import pytest

from conftest import REPO, has_gpu
from occluded_fixture import expected_occluded, expected_params
from rtamd import scenes

LIB = os.path.join(REPO, "ray-tracer-from-scratch_amd", "lib")
BIN = os.path.join(REPO, "tests", "cpp", "occluded_main")


@pytest.fixture(scope="module")
def occluded_main():
    src = os.path.join(REPO, "tests", "cpp", "occluded_main.cpp")
    if not os.path.exists(BIN) or os.path.getmtime(BIN) < os.path.getmtime(src):
        subprocess.run(["g++", "-std=c++17", "-O2", "-I", os.path.join(REPO, "include"), src,
                        "-o", BIN, "-L", LIB, "-lrt_host", "-lrt_amd", f"-Wl,-rpath,{LIB}"],
                       check=True)
    return BIN


def test_occluded_rejects_a_primitive_without_gpu_record(occluded_main):
    """A SceneGeometry subclass that has no pack() makes rt_occluded throw
    std::invalid_argument before any device work (CPU)."""
    out = subprocess.run([occluded_main, "plugin"], capture_output=True, text=True, check=True).stdout
    lines = out.strip().splitlines()
    assert len(lines) == 1
    assert lines[0].startswith("1 ") and "unsupported primitive" in lines[0], out


@pytest.mark.gpu
@pytest.mark.skipif(not has_gpu(), reason="needs a HIP device")
def test_cpp_occluded_matches_expectation(occluded_main, oracle):
    out = subprocess.run([occluded_main, "query"], capture_output=True, text=True, check=True).stdout
    rows = [ln.split() for ln in out.strip().splitlines()]
    assert len(rows) == 100 and all(len(r) == 8 for r in rows)
    v = np.array([[float.fromhex(x) for x in r[:7]] for r in rows])
    got = np.array([int(r[7]) for r in rows], np.uint8)
    prims = scenes.to_prims(scenes.default_scene())
    T = expected_params(oracle, prims, v[:, 0:3], v[:, 3:6])
    exp = expected_occluded(T, v[:, 6])
    assert np.array_equal(got, exp)
    assert 10 <= int(exp.sum()) <= 90   # both outcomes occur
