"""bench.py --dump-outputs: DIR/frame.npy is the float32 frame of the last timed step, or a
fixed seeded sample of a frame above bench.DUMP_MAX_BYTES; the same arguments give the same
file run after run.

CPU: dump_frame's contract on arrays.  GPU (one MI355X): two plain runs dump bitwise the
same frame, and it is the frame a separate render of the same scene, camera and precision
through the C-ABI gives (the same kernel, pixels independent: bitwise)."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from conftest import REPO, has_gpu

import bench


def test_dump_frame_writes_a_small_frame_whole(tmp_path):
    rng = np.random.default_rng(7)
    frame = rng.random((54, 96, 3), dtype=np.float32)
    bench.dump_frame(str(tmp_path / "new" / "dir"), frame)
    got = np.load(tmp_path / "new" / "dir" / "frame.npy")
    assert got.dtype == np.float32 and got.shape == (54, 96, 3)
    assert np.array_equal(got.view(np.uint32), frame.view(np.uint32))
    # a float64 or uint8 frame is stored as float32 too
    bench.dump_frame(str(tmp_path / "u8"), np.arange(24, dtype=np.uint8).reshape(2, 3, 4))
    got = np.load(tmp_path / "u8" / "frame.npy")
    assert got.dtype == np.float32 and np.array_equal(got.ravel(), np.arange(24))


def test_dump_frame_samples_a_config5_frame_the_same_way_every_time(tmp_path):
    h, w = 4320, 7680
    frame = np.empty((h, w, 3), dtype=np.float32)   # 398 MB: above the cap
    pix = np.arange(h * w, dtype=np.int64)
    # each pixel carries its own index (y in channel 0, x in channel 1: exact in float32)
    frame[..., 0] = (pix // w).reshape(h, w)
    frame[..., 1] = (pix % w).reshape(h, w)
    frame[..., 2] = 0.5
    bench.dump_frame(str(tmp_path / "a"), frame)
    bench.dump_frame(str(tmp_path / "b"), frame)
    a = np.load(tmp_path / "a" / "frame.npy")
    b = np.load(tmp_path / "b" / "frame.npy")
    n = bench.DUMP_MAX_BYTES // 12
    assert a.dtype == np.float32 and a.shape == (n, 3)
    assert a.nbytes <= bench.DUMP_MAX_BYTES <= 64 << 20
    assert np.array_equal(a, b)
    idx = a[:, 0].astype(np.int64) * w + a[:, 1].astype(np.int64)
    assert np.all(np.diff(idx) > 0)              # distinct pixels, ascending
    assert 0 <= idx[0] and idx[-1] < h * w
    assert np.all(a[:, 2] == 0.5)                # whole pixels, not scattered floats
    want = np.sort(np.random.default_rng(0).choice(h * w, size=n, replace=False))
    assert np.array_equal(idx, want)             # the documented seed-0 sample


def _plain_dump(dirname):
    env = dict(os.environ)
    for k in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "MASTER_ADDR", "MASTER_PORT"):
        env.pop(k, None)
    p = subprocess.run([sys.executable, os.path.join(REPO, "bench.py"), "--gpus", "1", "--steps", "3",
                        "--warmup", "1", "--deadline", "120", "--dump-outputs", str(dirname)],
                       env=env, capture_output=True, text=True, timeout=200, cwd=REPO)
    assert p.returncode == 0, p.stderr[-4000:]
    lines = [ln for ln in p.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, p.stdout[-2000:]
    return json.loads(lines[0]), np.load(os.path.join(dirname, "frame.npy"))


@pytest.mark.gpu
@pytest.mark.skipif(not has_gpu(), reason="needs a HIP device")
def test_plain_runs_dump_the_same_frame_and_it_is_the_rendered_frame(tmp_path):
    from rtamd import capi, scenes
    r1, a = _plain_dump(tmp_path / "a")
    r2, b = _plain_dump(tmp_path / "b")
    cfg = scenes.CONFIGS["c2"]
    assert r1["steps"] == 3 and r1["ms_per_step"] > 0 and r1["full"] is False
    assert r1["gather_check"] is None and r1["cpu_baseline"] is None and r1["kernel_ms"] is None
    assert os.listdir(tmp_path / "a") == ["frame.npy"]
    assert a.dtype == np.float32 and a.shape == (cfg.height, cfg.width, 3)
    assert np.array_equal(a.view(np.uint32), b.view(np.uint32))
    cam = capi.camera_init(**scenes.camera_args(cfg.width, cfg.height))
    with capi.Renderer(0) as r:
        r.set_scene(scenes.to_prims(cfg.scene()))
        img, _ = r.render(cam, cfg.depth, capi.PRECISIONS[r1["config"]["precision"]], 0,
                          capi.RT_OUT_RGB_F32)
    assert np.array_equal(a.view(np.uint32), np.ascontiguousarray(img).view(np.uint32))
