#!/usr/bin/env python3
"""CPU check of the pixels on which tools/bench_ao.py's two routes differ.

    python tools/ao_check_pixels.py profiles/ao.json [N]

For the first N (default: all) pixels of every step's `differing_sample` ([pixel, composed,
fused]) the expected count is formed on the CPU as tests/ao_fixture.py forms it — the oracle's
find_closest_hit for the pixel's ray, P, nf, sp and the flips in numpy fp64, the probes through
occluded_fixture — and compared with both routes' values.  Needs no GPU.
"""
import json
import os
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in ("ray-tracer-from-scratch_amd", "oracle", "tests"):
    sys.path.insert(0, os.path.join(REPO, p))

import numpy as np  # noqa: E402

import ao_fixture as aofx  # noqa: E402
import aov_fixture as afx  # noqa: E402
import occluded_fixture as ofx  # noqa: E402
import oracle as orc_mod  # noqa: E402
from rtamd import capi, scenes  # noqa: E402


def main():
    doc = json.load(open(sys.argv[1]))
    limit = int(sys.argv[2]) if len(sys.argv) > 2 else None
    orc = orc_mod.Oracle()
    for step in doc["steps"]:
        smp = np.array((step.get("differing_sample") or [])[:limit], np.int64).reshape(-1, 3)
        print(step["config"], "differing pixels", step["differing_pixels"], "checked", len(smp))
        if not len(smp):
            continue
        cfg = scenes.CONFIGS[step["config"]]
        prims = scenes.to_prims(cfg.scene())
        cam = capi.camera_init(**scenes.camera_args(cfg.width, cfg.height))
        k = step["ndirs"]
        dirs = np.random.default_rng(16).normal(size=(k, 3))   # bench_ao.py's
        dirs /= np.linalg.norm(dirs, axis=1)[:, None]
        i, j = smp[:, 0] // cfg.width, smp[:, 0] % cfg.width
        pos, tl = np.array(cam.position[:]), np.array(cam.image_top_left[:])
        dx, dy = np.array(cam.pixel_delta_x[:]), np.array(cam.pixel_delta_y[:])
        d = pos - ((tl + dx * j[:, None].astype(np.float64)) + dy * i[:, None].astype(np.float64))
        o = np.broadcast_to(pos, d.shape).copy()
        hits = afx.closest_hits(orc, prims, o, d)
        hm = hits["index"] >= 0
        cnt = np.zeros(len(smp), np.int64)
        P, n = aofx.surface(prims, hits[hm], o[hm], d[hm])
        sp, w, _, _ = aofx.probes(P, n, d[hm], dirs)
        T = ofx.expected_params(orc, prims, np.repeat(sp, k, axis=0), w.reshape(-1, 3))
        cnt[hm] = ofx.expected_occluded(T, step["radius"]).reshape(-1, k).sum(axis=1)
        print("  fixture == fused on", int((cnt == smp[:, 2]).sum()), " fixture == composed on",
              int((cnt == smp[:, 1]).sum()), "of", len(smp))
        print("  composed - fixture:", dict(zip(*map(lambda a: a.tolist(),
                                                     np.unique(smp[:, 1] - cnt, return_counts=True)))))
        print("  fused - fixture:", dict(zip(*map(lambda a: a.tolist(),
                                                  np.unique(smp[:, 2] - cnt, return_counts=True)))))


if __name__ == "__main__":
    main()
