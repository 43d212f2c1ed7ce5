#!/usr/bin/env python3
"""Transmission records (rt_set_transmission): what k transmissive spheres and one pane cost,
against the same scene with every object opaque routed through the lights kernels, on one GPU.

    python tools/bench_glass.py [--reps 20] [--windows 5] [--out FILE]

Config c2 (8 spheres + 4 walls, depth 4, 1920x1080), PATH64, RT_OUT_RGB_F32.  Variants:

  plain        a ctx without lights or records (the plain kernels), for scale
  lights_1     the reference's light {(0,0,0), (1,1,1)} set through rt_set_lights and no records:
               the lights kernels, which the glass kernels extend — the route to compare against
               (tools/bench_lights.py's lights_1)
  glass_k      k = 1, 2, 4, 8: spheres 0..k-1 with (.85, 1.5) and wall nS + 1 with (.6, 1), no
               lights set: the glass kernels with the reference's light

Reported per variant: ms per frame (median, minimum and maximum window), segments per frame, ns
per segment, and the primary rays that hit a transmissive object (counted from rt_render_aov's
index layer).  Per glass variant also `extra_ns_per_primary_glass_hit`: (ms - segments x
lights_1's ns per segment) / primary transmissive hits — the cost of the passages beyond the
segments they lead to, charged to the primary transmissive hits alone, so an upper bound on the
cost per transmissive hit (deeper ones are not counted).

Method as tools/bench_lights.py: the work runs in a child process under a time limit (a step that
fails, faults or runs out of time ends the run: nothing more is started on the GPU).  Timing is
the warm frames-in-flight loop: consecutive frames alternate between two streams with buffers of
their own, HIP events around windows of >= --reps frames, the variants interleaved window by
window; the median window is reported.

The last line printed is one JSON object; --out also writes it to a file.
"""
import argparse
import json
import os
import statistics
import subprocess
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "ray-tracer-from-scratch_amd"))

STEP_LIMIT_S = 300
ONE = [((0, 0, 0), (1, 1, 1))]


def records(k, ns, nw):
    t = [(.85, 1.5) if j < k else 0 for j in range(ns)] + [0] * nw
    t[ns + 1] = (.6, 1)
    return t


def run_step(args):
    import numpy as np
    import torch
    from rtamd import capi, scenes
    dev = torch.device("cuda", 0)
    streams = [torch.cuda.Stream(dev) for _ in range(2)]
    cfg = scenes.CONFIGS["c2"]
    W, H, depth = cfg.width, cfg.height, cfg.depth
    ns, nw = cfg.n_spheres, cfg.n_walls
    prims = scenes.to_prims(cfg.scene())
    cam = capi.camera_init(**scenes.camera_args(W, H))
    prec, fmt = capi.RT_PREC_PATH64, capi.RT_OUT_RGB_F32
    r = capi.Renderer(0)
    r.set_scene(prims)
    index = r.render_aov(cam, layers=("index",))[0]["index"]
    img = [torch.zeros((H, W, 3), dtype=torch.float32, device=dev) for _ in streams]
    segs_t = torch.zeros(1, dtype=torch.int64, device=dev)

    def variant(lights, k):
        def setup():
            r.set_lights(lights)
            r.set_transmission(records(k, ns, nw) if k else None)

        def go(s, seg=0):
            r.render_device(cam, depth, img[s].data_ptr(), prec, 0, fmt, d_segments=seg,
                            stream=streams[s].cuda_stream)
        return setup, go

    variants = [("plain", 0, variant(None, 0)), ("lights_1", 0, variant(ONE, 0))]
    variants += [(f"glass_{k}", k, variant(None, k)) for k in (1, 2, 4, 8)]

    def window(v, nf):
        setup, launch = v
        torch.cuda.synchronize()   # a set replaces the ctx's table: between windows, nothing in flight
        setup()
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
    for what, k, v in variants:   # segments of one frame, and the warm-up
        segs_t.zero_()
        v[0]()
        v[1](0, seg=segs_t.data_ptr())
        torch.cuda.synchronize()
        hits = 0
        if k:
            glass = [j for j, t in enumerate(records(k, ns, nw)) if t != 0]
            hits = int(np.isin(index, glass).sum())
        row = {"what": what, "segments": int(segs_t.item()), "primary_glass_hits": hits, "ms": []}
        window(v, 4)
        per = window(v, args.reps)
        row["reps"] = int(min(2000, max(args.reps, 50.0 / max(per, 1e-6))))
        rows.append((row, v))
    for _ in range(args.windows):          # interleaved: drift of the box cancels out
        for row, v in rows:
            row["ms"].append(window(v, row["reps"]))
    res = {"config": "c2", "output": [W, H], "depth": depth, "precision": "path64",
           "out_format": "rgb_f32", "frames_in_flight": 2, "windows": args.windows, "results": []}
    for row, _ in rows:
        med = statistics.median(row["ms"])
        res["results"].append({"what": row["what"], "segments": row["segments"],
                               "primary_glass_hits": row["primary_glass_hits"],
                               "frames_per_window": row["reps"], "ms_median": round(med, 5),
                               "ms_min": round(min(row["ms"]), 5), "ms_max": round(max(row["ms"]), 5),
                               "ns_per_segment": round(1e6 * med / max(row["segments"], 1), 4)})
    by = {x["what"]: x for x in res["results"]}
    base = by["lights_1"]["ms_median"] / by["lights_1"]["segments"]   # ms per segment, all opaque
    for x in res["results"]:
        if x["what"].startswith("glass_"):
            x["ms_over_lights_1"] = round(x["ms_median"] / by["lights_1"]["ms_median"], 4)
            x["segments_over_lights_1"] = round(x["segments"] / by["lights_1"]["segments"], 4)
            extra = x["ms_median"] - x["segments"] * base
            x["extra_ns_per_primary_glass_hit"] = round(1e6 * extra / max(x["primary_glass_hits"], 1), 4)
    res["lights_1_over_plain"] = round(by["lights_1"]["ms_median"] / by["plain"]["ms_median"], 4)
    r.close()
    print(json.dumps(res), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20, help="frames per timed window, at least")
    ap.add_argument("--windows", type=int, default=5)
    ap.add_argument("--out", default="")
    ap.add_argument("--step", action="store_true", help="(internal) do the work in this process")
    args = ap.parse_args()
    if args.reps < 20:
        ap.error("--reps must be at least 20")
    if args.step:
        run_step(args)
        return 0
    cmd = [sys.executable, os.path.abspath(__file__), "--step", "--reps", str(args.reps),
           "--windows", str(args.windows)]
    try:
        p = subprocess.run(cmd, capture_output=True, text=True, timeout=STEP_LIMIT_S)
    except subprocess.TimeoutExpired:
        print(json.dumps({"error": f"time limit of {STEP_LIMIT_S} s"}), flush=True)
        return 1   # a hung step: nothing more on the GPU
    if p.returncode != 0:
        sys.stderr.write(p.stderr[-2000:])
        print(json.dumps({"error": f"exit status {p.returncode}"}), flush=True)
        return 1
    doc = p.stdout.strip().splitlines()[-1]
    json.loads(doc)
    if args.out:
        with open(args.out, "w") as fh:
            fh.write(doc + "\n")
    print(doc, flush=True)
    return 0


if __name__ == "__main__":
    sys.exit(main())
