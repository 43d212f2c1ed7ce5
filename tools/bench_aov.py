#!/usr/bin/env python3
"""Frame AOVs (rt_render_aov_device): what a G-buffer costs against the route there was before
it, on one GPU.

    python tools/bench_aov.py [--configs c2,c5] [--reps 20] [--windows 5] [--out FILE]

Per config, at bench.py's frame size and scene (c2: 1920x1080, 8 spheres + 4 walls, the linear
scan; c5: 7680x4320, 256 spheres, the wave cull), these variants are timed in one process:

  rays_hits    the earlier route: rt_trace_rays_device, hits only, on the frame's camera rays
               uploaded beforehand (48 B per pixel read, 40 B written) — the baseline
  aov_hit      rt_render_aov_device, `hit` only (40 B per pixel written, no ray buffer)
  aov_all      rt_render_aov_device, all five layers (72 B per pixel)
  aov_id_depth rt_render_aov_device, `index` + `depth` (8 B per pixel)
  frame_d0     a depth-0 PATH64 RT_OUT_RGB_F32 frame (rt_render_device), for scale

and reported: every variant's median ms per frame with its minimum and maximum window;
aov_hit over rays_hits with the verdict "no slower than rays_hits beyond rays_hits' own
spread" (aov_hit's median <= rays_hits' median + (rays_hits' max - min window)); aov_all and
aov_id_depth as a fraction of frame_d0.  Before timing, aov_hit's records are compared
bytewise with rays_hits' (`hits_equal`).

Method as tools/bench_lights.py: each config runs in a child process of its own under its own
time limit (a step that fails, faults or runs out of time ends the run: nothing more is started
on the GPU).  Timing is the warm frames-in-flight loop: consecutive launches alternate between
two streams with buffers of their own, HIP events around windows of >= --reps launches (more
when they take under ~50 ms), the variants interleaved window by window.  The shader clock
rocm-smi reports before and after is recorded as read (nothing is set).

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

STEP_LIMIT_S = 300
LAYER_BYTES = {"hit": 40, "index": 4, "depth": 4, "normal": 12, "albedo": 12}


def clocks():
    try:
        out = subprocess.run(["rocm-smi", "--showclocks", "-d", "0"], capture_output=True, text=True,
                             timeout=20).stdout
        return [ln.strip() for ln in out.splitlines() if "sclk" in ln or "mclk" in ln][:4]
    except Exception as e:  # the tool is optional
        return [f"unavailable: {e}"]


def camera_rays(torch, cam, dev):
    """The frame's pixel rays (main.cpp:132-134) in device memory: [H * W, 3] fp64 each."""
    t = lambda v: torch.tensor(list(v), dtype=torch.float64, device=dev)  # noqa: E731
    pos, tl, dx, dy = t(cam.position), t(cam.image_top_left), t(cam.pixel_delta_x), t(cam.pixel_delta_y)
    x = torch.arange(cam.width, dtype=torch.float64, device=dev)[None, :, None]
    i = torch.arange(cam.height, dtype=torch.float64, device=dev)[:, None, None]
    d = (pos - ((tl + dx * x) + dy * i)).reshape(-1, 3).contiguous()
    return pos.expand_as(d).contiguous(), d


def run_step(name, args):
    import torch
    from rtamd import capi, scenes
    dev = torch.device("cuda", 0)
    streams = [torch.cuda.Stream(dev) for _ in range(2)]
    cfg = scenes.CONFIGS[name]
    W, H = cfg.width, cfg.height
    npx = W * H
    prims = scenes.to_prims(cfg.scene())
    cam = capi.camera_init(**scenes.camera_args(W, H))
    clk0 = clocks()
    r = capi.Renderer(0)
    r.set_scene(prims)
    d_o, d_d = camera_rays(torch, cam, dev)
    bufs = [{k: torch.zeros(npx * b, dtype=torch.uint8, device=dev) for k, b in LAYER_BYTES.items()}
            for _ in streams]
    img = [torch.zeros((H, W, 3), dtype=torch.float32, device=dev) for _ in streams]
    torch.cuda.synchronize()

    def rays_hits(k):
        r.trace_rays_device(d_o.data_ptr(), d_d.data_ptr(), npx, 0, 0, bufs[k]["hit"].data_ptr(),
                            stream=streams[k].cuda_stream)

    def aov(layers):
        def go(k):
            r.render_aov_device(cam, {n: bufs[k][n].data_ptr() for n in layers},
                                stream=streams[k].cuda_stream)
        return go

    def frame_d0(k):
        r.render_device(cam, 0, img[k].data_ptr(), capi.RT_PREC_PATH64, 0, capi.RT_OUT_RGB_F32,
                        stream=streams[k].cuda_stream)

    variants = [("rays_hits", rays_hits, 88), ("aov_hit", aov(("hit",)), 40),
                ("aov_all", aov(tuple(LAYER_BYTES)), sum(LAYER_BYTES.values())),
                ("aov_id_depth", aov(("index", "depth")), 8), ("frame_d0", frame_d0, 12)]

    # the two routes give the same records
    rays_hits(0)
    torch.cuda.synchronize()
    ref = bufs[0]["hit"].clone()
    bufs[0]["hit"].zero_()
    torch.cuda.synchronize()   # (the clearing runs on torch's stream, the launch on streams[0])
    aov(("hit",))(0)
    torch.cuda.synchronize()
    hits_equal = bool(torch.equal(ref, bufs[0]["hit"]))
    del ref

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
    for what, launch, bpp in variants:   # the warm-up, and the window length
        window(launch, 4)
        per = window(launch, args.reps)
        rows.append({"what": what, "launch": launch, "bytes_per_pixel": bpp, "ms": [],
                     "reps": int(min(2000, max(args.reps, 50.0 / max(per, 1e-6))))})
    for _ in range(args.windows):          # interleaved: drift of the box cancels out
        for row in rows:
            row["ms"].append(window(row["launch"], row["reps"]))
    res = {"step": name, "config": name, "output": [W, H], "spheres": cfg.n_spheres, "walls": cfg.n_walls,
           "launches_in_flight": 2, "windows": args.windows, "hits_equal": hits_equal,
           "clocks_before": clk0, "clocks_after": clocks(), "results": []}
    for row in rows:
        med = statistics.median(row["ms"])
        res["results"].append({"what": row["what"], "bytes_per_pixel": row["bytes_per_pixel"],
                               "launches_per_window": row["reps"], "ms_median": round(med, 5),
                               "ms_min": round(min(row["ms"]), 5), "ms_max": round(max(row["ms"]), 5),
                               "gb_per_s": round(row["bytes_per_pixel"] * npx / med / 1e6, 1)})
    by = {x["what"]: x for x in res["results"]}
    a, b = by["rays_hits"], by["aov_hit"]
    spread = a["ms_max"] - a["ms_min"]
    res["rays_hits_spread_ms"] = round(spread, 5)
    res["aov_hit_over_rays_hits"] = round(b["ms_median"] / a["ms_median"], 4)
    res["aov_hit_no_slower_than_rays_hits_within_its_spread"] = b["ms_median"] <= a["ms_median"] + spread
    for k in ("aov_all", "aov_id_depth", "aov_hit"):
        res[f"{k}_over_frame_d0"] = round(by[k]["ms_median"] / by["frame_d0"]["ms_median"], 4)
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
    if args.reps < 20:
        ap.error("--reps must be at least 20")
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
