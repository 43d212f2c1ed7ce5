#!/usr/bin/env python3
"""Ambient occlusion frames (rt_render_ao_device): the fused kernel against the route there was
before it, on one GPU.

    python tools/bench_ao.py [--configs c2,c5] [--reps 20] [--windows 5] [--out FILE]

Per config, at bench.py's frame size and scene (c2: 1920x1080, 8 spheres + 4 walls, the linear
scan; c5: 7680x4320, 256 spheres, the wave cull), K = 16 directions, radius 1.5:

  composed   (a) the earlier route: rt_render_aov_device(hit), then K rt_occluded_device calls
             over probe rays built beforehand and resident (origin sp per pixel, one direction
             buffer per k with the flips applied, one limit buffer), one mask buffer per k.
             Building the rays and reducing the K masks are not timed, which favours (a).
  ao_count   (b) rt_render_ao_device, `count` only
  ao_both    (c) rt_render_ao_device, `count` and `ao`

Before timing, the sum of (a)'s K masks is compared with (b)'s count (`counts_equal`; the
first 2000 differing pixels are listed as [pixel, composed, fused] in `differing_sample`); the
probe rays are built on the device with torch's fp64 elementwise operations in the header's
order (one rounding per operation).  The directions are seeded random unit vectors, not
rt_ao_directions': none of their components is exactly 0.  Reported: every variant's median ms
per launch with its minimum and maximum window, and the verdict "(b) no slower than (a) beyond
(a)'s own max - min window spread".

Method as tools/bench_aov.py: each config in a child process of its own under its own time
limit (a step that fails, faults or runs out of time ends the run: nothing more is started on the
GPU); launches alternate between two streams with buffers of their own, HIP events around
windows of >= --reps launches, the variants interleaved window by window.

The last line printed is one JSON object {"steps": [...]}; --out also writes it to a file.
"""
import argparse
import json
import os
import statistics
import subprocess
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "ray-tracer-from-scratch_amd"))

STEP_LIMIT_S = 400
K = 16
RADIUS = 1.5


def dot(a, b):
    return (a[:, 0] * b[:, 0] + a[:, 1] * b[:, 1]) + a[:, 2] * b[:, 2]


def probe_rays(torch, r, cam, prims, dirs, dev):
    """-> (sp [npx, 3], [K] direction buffers [npx, 3], hit mask [npx]) on the device, from
    rt_render_aov_device's records: rt_capi.h's P, nf, sp and flips."""
    from rtamd import capi
    npx = cam.width * cam.height
    rec = torch.zeros(npx * 5, dtype=torch.float64, device=dev)   # rt_hit = 5 x 8 bytes
    torch.cuda.synchronize()
    r.render_aov_device(cam, {"hit": rec.data_ptr()})
    torch.cuda.synchronize()
    rec = rec.view(npx, 5)
    index = rec[:, 4].contiguous().view(torch.int32)[::2].to(torch.int64)
    hit = index >= 0
    t = lambda v: torch.tensor(list(v), dtype=torch.float64, device=dev)  # noqa: E731
    pos, tl, dx, dy = t(cam.position), t(cam.image_top_left), t(cam.pixel_delta_x), t(cam.pixel_delta_y)
    x = torch.arange(cam.width, dtype=torch.float64, device=dev)[None, :, None]
    i = torch.arange(cam.height, dtype=torch.float64, device=dev)[:, None, None]
    d = (pos - ((tl + dx * x) + dy * i)).reshape(-1, 3)
    o = pos.expand_as(d)
    is_wall = torch.tensor([p.kind == capi.RT_PRIM_WALL for p in prims] + [True], device=dev)
    centre = torch.tensor([list(p.position) for p in prims] + [[0.0] * 3], dtype=torch.float64, device=dev)
    rad = torch.tensor([p.radius for p in prims] + [1.0], dtype=torch.float64, device=dev)
    j = torch.where(hit, index, torch.full_like(index, len(prims)))
    # a sphere's projection (scene.cpp:45-72; det > 0 at a hit, p2 <= p1)
    oc = o - centre[j]
    a = dot(d, d)
    b = 2 * dot(d, oc)
    c = dot(oc, oc) - rad[j] * rad[j]
    det = b * b - 4 * a * c
    proj = (-b - torch.sqrt(det.clamp_min(0))) / (2 * a)
    par = torch.where(is_wall[j], rec[:, 0], proj)
    P = o + d * par[:, None]
    n = rec[:, 1:4]
    f = dot(d, n)
    nf = torch.where((f > 0)[:, None], -n, n)
    sp = (P + nf * .0001).contiguous()
    sp[~hit] = torch.tensor([0.0, 0.0, 1.0], dtype=torch.float64, device=dev)
    ws = []
    for k in range(len(dirs)):
        w = t(dirs[k])[None, :].expand(npx, 3)
        s = dot(w, nf)
        ws.append(torch.where((s < 0)[:, None], -w, w).contiguous())
    return sp, ws, hit


def run_step(name, args):
    import numpy as np
    import torch
    from rtamd import capi, scenes
    dev = torch.device("cuda", 0)
    streams = [torch.cuda.Stream(dev) for _ in range(2)]
    cfg = scenes.CONFIGS[name]
    W, H = cfg.width, cfg.height
    npx = W * H
    prims = scenes.to_prims(cfg.scene())
    cam = capi.camera_init(**scenes.camera_args(W, H))
    rng = np.random.default_rng(16)
    dirs = rng.normal(size=(K, 3))
    dirs /= np.linalg.norm(dirs, axis=1)[:, None]
    r = capi.Renderer(0)
    r.set_scene(prims)
    sp, ws, hit = probe_rays(torch, r, cam, prims, dirs, dev)
    # a miss has no probes: its limit is 0 (never occluded)
    tmax = torch.where(hit, torch.full((npx,), RADIUS, dtype=torch.float64, device=dev),
                       torch.zeros(npx, dtype=torch.float64, device=dev))
    rec = [torch.zeros(npx * 40, dtype=torch.uint8, device=dev) for _ in streams]
    masks = [torch.zeros((K, npx), dtype=torch.uint8, device=dev) for _ in streams]
    count = [torch.zeros(npx, dtype=torch.uint8, device=dev) for _ in streams]
    ao = [torch.zeros(npx, dtype=torch.float32, device=dev) for _ in streams]
    torch.cuda.synchronize()

    def composed(q):
        s = streams[q].cuda_stream
        r.render_aov_device(cam, {"hit": rec[q].data_ptr()}, stream=s)
        for k in range(K):
            r.occluded_device(sp.data_ptr(), ws[k].data_ptr(), tmax.data_ptr(), npx,
                              masks[q][k].data_ptr(), stream=s)

    def fused(layers):
        def go(q):
            bufs = {"count": count[q].data_ptr()}
            if "ao" in layers:
                bufs["ao"] = ao[q].data_ptr()
            r.render_ao_device(cam, dirs, RADIUS, bufs, stream=streams[q].cuda_stream)
        return go

    variants = [("composed", composed), ("ao_count", fused(("count",))), ("ao_both", fused(("count", "ao")))]

    composed(0)
    fused(("count",))(0)
    torch.cuda.synchronize()
    total = masks[0].sum(dim=0, dtype=torch.int32)
    bad = torch.nonzero(total != count[0].to(torch.int32)).reshape(-1)
    differing = int(bad.numel())
    # the first differing pixels as [pixel, composed, fused], for a check against the CPU fixture
    sample = [[int(q), int(total[q]), int(count[0][q])] for q in bad[:2000].tolist()]
    hist = torch.bincount(count[0][hit].to(torch.int64), minlength=K + 1).tolist()

    def window(launch, nf):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(streams[0])
        streams[1].wait_stream(streams[0])
        for f in range(nf):
            launch(f & 1)
        streams[0].wait_stream(streams[1])
        e1.record(streams[0])
        torch.cuda.synchronize()
        return e0.elapsed_time(e1) / nf

    rows = []
    for what, launch in variants:
        window(launch, 2)
        per = window(launch, 4)
        rows.append({"what": what, "launch": launch, "ms": [],
                     "reps": int(min(1000, max(args.reps, 50.0 / max(per, 1e-6))))})
    for _ in range(args.windows):
        for row in rows:
            row["ms"].append(window(row["launch"], row["reps"]))
    res = {"step": name, "config": name, "output": [W, H], "spheres": cfg.n_spheres, "walls": cfg.n_walls,
           "ndirs": K, "radius": RADIUS, "launches_in_flight": 2, "windows": args.windows,
           "counts_equal": differing == 0, "differing_pixels": differing, "hit_pixels": int(hit.sum()),
           "count_histogram": hist, "differing_sample": sample, "results": []}
    for row in rows:
        res["results"].append({"what": row["what"], "launches_per_window": row["reps"],
                               "ms_median": round(statistics.median(row["ms"]), 5),
                               "ms_min": round(min(row["ms"]), 5), "ms_max": round(max(row["ms"]), 5)})
    by = {x["what"]: x for x in res["results"]}
    a, b = by["composed"], by["ao_count"]
    spread = a["ms_max"] - a["ms_min"]
    res["composed_spread_ms"] = round(spread, 5)
    res["ao_count_over_composed"] = round(b["ms_median"] / a["ms_median"], 4)
    res["ao_count_no_slower_than_composed_within_its_spread"] = b["ms_median"] <= a["ms_median"] + spread
    r.close()
    print(json.dumps(res), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--configs", default="c2,c5")
    ap.add_argument("--reps", type=int, default=20, help="launches per timed window, at least")
    ap.add_argument("--windows", type=int, default=5)
    ap.add_argument("--out", default="")
    ap.add_argument("--step", default="", help="(internal) run this one config in this process")
    args = ap.parse_args()
    if args.reps < 5:
        ap.error("--reps must be at least 5")
    if args.step:
        run_step(args.step, args)
        return 0
    steps = []
    for c in args.configs.split(","):
        if c not in ("c2", "c5"):
            ap.error("--configs takes c2 and c5")
        cmd = [sys.executable, os.path.abspath(__file__), "--step", c, "--reps", str(args.reps),
               "--windows", str(args.windows)]
        try:
            p = subprocess.run(cmd, capture_output=True, text=True, timeout=STEP_LIMIT_S)
        except subprocess.TimeoutExpired:
            print(json.dumps({"step": c, "error": f"time limit of {STEP_LIMIT_S} s"}), flush=True)
            return 1   # a hung step: nothing more on the GPU
        if p.returncode != 0:
            sys.stderr.write(p.stderr[-2000:])
            print(json.dumps({"step": c, "error": f"exit status {p.returncode}"}), flush=True)
            return 1
        steps.append(json.loads(p.stdout.strip().splitlines()[-1]))
    doc = json.dumps({"steps": steps})
    if args.out:
        with open(args.out, "w") as fh:
            fh.write(doc + "\n")
    print(doc, flush=True)
    return 0


if __name__ == "__main__":
    sys.exit(main())
