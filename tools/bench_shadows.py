#!/usr/bin/env python3
"""Hard shadows (RT_FLAG_SHADOWS): what the fused light ray costs, and the fused frame against
the two-pass way of getting the same shadow decisions, on one GPU.

    python tools/bench_shadows.py [--configs c2,c3] [--reps 20] [--windows 5] [--out FILE]

Per config (c2: 8 spheres + 4 walls, depth 4, 1920x1080; c3: 64 spheres + 6 walls, depth 6,
3840x2160), PATH64, RT_OUT_RGB_F32, these variants are timed:

  plain / shadows          rt_render_device without / with the flag at the config's depth
  plain_d0 / shadows_d0    the same at depth 0 (one segment per pixel)
  two_pass_d0              the unflagged depth-0 frame, then rt_trace_rays_device for the hit
                           records of the same pixel rays, then torch builds sp = pos +
                           normal * 1e-4 and -sp from the records, then rt_occluded_device with
                           limit 1 (0 for the rays that missed): what a caller had to do for
                           the decisions alone before the flag existed (and still could not
                           feed them into the recursion)

Each config runs in a child process of its own under its own time limit (a step that fails,
faults or runs out of time ends the run: nothing more is started on the GPU).  Timing is the
warm frames-in-flight loop: consecutive frames alternate between two streams with buffers of
their own, HIP events around windows of >= --reps frames (more when they take under ~50 ms),
the variants interleaved window by window; the median window is reported as ms per frame,
with the minimum and maximum window as the run-to-run spread.  The shader clock rocm-smi
reports before and after is recorded as read (nothing is set).

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


def clocks():
    try:
        out = subprocess.run(["rocm-smi", "--showclocks", "-d", "0"], capture_output=True, text=True,
                             timeout=20).stdout
        return [ln.strip() for ln in out.splitlines() if "sclk" in ln or "mclk" in ln][:4]
    except Exception as e:  # the tool is optional
        return [f"unavailable: {e}"]


def run_step(name, args):
    import numpy as np
    import torch
    from rtamd import capi, scenes
    dev = torch.device("cuda", 0)
    streams = [torch.cuda.Stream(dev) for _ in range(2)]
    cfg = scenes.CONFIGS[name]
    W, H, depth = cfg.width, cfg.height, cfg.depth
    prims = scenes.to_prims(cfg.scene())
    cam = capi.camera_init(**scenes.camera_args(W, H))
    prec, fmt, SH = capi.RT_PREC_PATH64, capi.RT_OUT_RGB_F32, capi.RT_FLAG_SHADOWS
    clk0 = clocks()
    r = capi.Renderer(0)
    r.set_scene(prims)
    n = W * H
    # the pixel rays of rt_scene (main.cpp:132-134): direction = position - pixel centre
    v = [np.array(a[:]) for a in (cam.position, cam.image_top_left, cam.pixel_delta_x, cam.pixel_delta_y)]
    pc = (v[1] + v[2] * np.arange(W, dtype=np.float64)[None, :, None]) + \
        v[3] * np.arange(H, dtype=np.float64)[:, None, None]
    drc = torch.from_numpy((v[0] - pc).reshape(-1, 3)).to(dev)
    org = torch.from_numpy(np.broadcast_to(v[0], (n, 3)).copy()).to(dev)
    img = [torch.zeros((H, W, 3), dtype=torch.float32, device=dev) for _ in streams]
    hits = [torch.zeros((n, 5), dtype=torch.float64, device=dev) for _ in streams]   # rt_hit records
    mask = [torch.zeros(n, dtype=torch.uint8, device=dev) for _ in streams]
    segs_t = torch.zeros(1, dtype=torch.int64, device=dev)

    def frame(flags, dep):
        def go(k, seg=0):
            r.render_device(cam, dep, img[k].data_ptr(), prec, flags, fmt, d_segments=seg,
                            stream=streams[k].cuda_stream)
        return go

    def two_pass(k, seg=0):
        s = streams[k].cuda_stream
        r.render_device(cam, 0, img[k].data_ptr(), prec, 0, fmt, d_segments=seg, stream=s)
        r.trace_rays_device(org.data_ptr(), drc.data_ptr(), n, 0, 0, hits[k].data_ptr(),
                            capi.RT_PREC_F64, 0, capi.RT_OUT_RGB_F64, stream=s)
        with torch.cuda.stream(streams[k]):
            hk = hits[k]
            hit = hk.view(torch.int32)[:, 8] >= 0
            pos = org + drc * hk[:, 0:1]
            sp = torch.where(hit[:, None], pos + hk[:, 1:4] * .0001, torch.ones_like(pos))
            sd = -sp
            tmax = hit.to(torch.float64)
            r.occluded_device(sp.data_ptr(), sd.data_ptr(), tmax.data_ptr(), n, mask[k].data_ptr(),
                              stream=s)
            two_pass.keep = (sp, sd, tmax)   # alive until the stream has used them

    variants = [("plain", frame(0, depth)), ("shadows", frame(SH, depth)),
                ("plain_d0", frame(0, 0)), ("shadows_d0", frame(SH, 0)), ("two_pass_d0", two_pass)]

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
    for what, launch in variants:   # segments of one frame, and the warm-up
        segs_t.zero_()
        launch(0, seg=segs_t.data_ptr())
        torch.cuda.synchronize()
        row = {"what": what, "segments": int(segs_t.item()), "ms": []}
        window(launch, 4)
        per = window(launch, args.reps)
        row["reps"] = int(min(2000, max(args.reps, 50.0 / max(per, 1e-6))))
        rows.append((row, launch))
    # the two ways decide alike: pixels the flag darkens at depth 0 are the occluded rays
    frame(0, 0)(0)
    frame(SH, 0)(1)
    torch.cuda.synchronize()
    darker = int(((img[0] - img[1]).abs().amax(dim=-1) > 0).sum().item())
    two_pass(0)
    torch.cuda.synchronize()
    occluded = int(mask[0].sum().item())
    for _ in range(args.windows):          # interleaved: drift of the box cancels out
        for row, launch in rows:
            row["ms"].append(window(launch, row["reps"]))
    res = {"step": name, "config": name, "output": [W, H], "depth": depth, "precision": "path64",
           "out_format": "rgb_f32", "frames_in_flight": 2, "windows": args.windows,
           "clocks_before": clk0, "clocks_after": clocks(),
           "pixels_darkened_at_depth_0": darker, "rays_occluded_two_pass": occluded, "results": []}
    for row, _ in rows:
        med = statistics.median(row["ms"])
        res["results"].append({"what": row["what"], "segments": row["segments"],
                               "frames_per_window": row["reps"], "ms_median": round(med, 5),
                               "ms_min": round(min(row["ms"]), 5), "ms_max": round(max(row["ms"]), 5)})
    by = {x["what"]: x["ms_median"] for x in res["results"]}
    res["shadows_over_plain"] = round(by["shadows"] / by["plain"], 4)
    res["shadows_d0_over_plain_d0"] = round(by["shadows_d0"] / by["plain_d0"], 4)
    res["shadows_d0_over_two_pass_d0"] = round(by["shadows_d0"] / by["two_pass_d0"], 4)
    r.close()
    print(json.dumps(res), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--configs", default="c2,c3")
    ap.add_argument("--reps", type=int, default=20, help="frames per timed window, at least")
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
        if c not in ("c2", "c3"):
            ap.error("--configs takes c2 and c3")
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
