"""The C++ mirror's batch ray queries (include/rt/scene.h: rt_closest_hits, rt_radiance):
host code written against the reference's find_closest_hit / recursive_ray_tracing links to
the built libraries; on the GPU its hits equal the oracle's bitwise and its radiance within
the F64 bound."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from conftest import REPO, has_gpu
from rtamd import scenes

LIB = os.path.join(REPO, "ray-tracer-from-scratch_amd", "lib")
BIN = os.path.join(REPO, "tests", "cpp", "rays_main")


@pytest.fixture(scope="module")
def rays_main():
    src = os.path.join(REPO, "tests", "cpp", "rays_main.cpp")
    if not os.path.exists(BIN) or os.path.getmtime(BIN) < os.path.getmtime(src):
        subprocess.run(["g++", "-std=c++17", "-O2", "-I", os.path.join(REPO, "include"), src,
                        "-o", BIN, "-L", LIB, "-lrt_host", "-lrt_amd", f"-Wl,-rpath,{LIB}"],
                       check=True)
    return BIN


def test_ray_queries_reject_a_primitive_without_gpu_record(rays_main):
    """rays_main.cpp builds against librt_host; a SceneGeometry subclass that has no pack()
    makes both calls throw std::invalid_argument before any device work (CPU)."""
    out = subprocess.run([rays_main, "plugin"], capture_output=True, text=True, check=True).stdout
    lines = out.strip().splitlines()
    assert len(lines) == 2
    for ln in lines:
        assert ln.startswith("1 ") and "unsupported primitive" in ln, out


@pytest.mark.gpu
@pytest.mark.skipif(not has_gpu(), reason="needs a HIP device")
@pytest.mark.parametrize("depth", [10, 0])
def test_cpp_ray_queries_match_oracle(rays_main, oracle, depth):
    out = subprocess.run([rays_main, "trace", str(depth)], capture_output=True, text=True,
                         check=True).stdout
    rows = [ln.split() for ln in out.strip().splitlines()]
    assert len(rows) == 100 and all(len(r) == 15 for r in rows)
    prims = scenes.to_prims(scenes.default_scene())
    nhit = 0
    for r in rows:
        v = [float.fromhex(x) for x in r[:6] + r[8:]]
        o, d = v[0:3], v[3:6]
        idx, hit = int(r[6]), int(r[7])
        dist, nrm, rgb = v[6], v[7:10], v[10:13]
        ei, ed, en = oracle.find_closest_hit(prims, o, d)
        assert idx == ei and hit == (1 if ei >= 0 else 0)
        assert np.float64(dist).tobytes() == np.float64(ed).tobytes()
        assert np.asarray(nrm, np.float64).tobytes() == np.asarray(en, np.float64).tobytes()
        ergb, _ = oracle.trace(prims, o, d, depth)
        assert np.abs(np.asarray(rgb) - np.asarray(ergb)).max() <= 1e-12
        nhit += hit
    assert 20 <= nhit <= 95   # the fixed rays exercise hits and misses
