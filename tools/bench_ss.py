#!/usr/bin/env python3
"""Supersampled frames (RT_OPT_SUPERSAMPLE): the fused in-kernel resolve against the two-pass
way of getting the same frame, on one GPU.

    python tools/bench_ss.py [--factors 2,4] [--reps 20] [--windows 5] [--out FILE]

Config c2's scene (8 spheres + 4 walls), depth 4, PATH64, RT_OUT_RGB_F32, a 1920x1080 output.
For each factor S these variants are timed:

  fused        rt_render_device with RT_OPT_SUPERSAMPLE = S: S*S rays per pixel traced and
               averaged in the kernel, 1920x1080 pixels written
  plain_large  rt_render_device of rt_supersample_camera(cam, S) into an (S*1080) x (S*1920)
               buffer: the same rays, every sample written (no resolve at all)
  plain_large_static_order
               plain_large with RT_OPT_ROW_FEEDBACK = 0: the centre-out tile-row order, which
               is what a supersampled frame gets (the measured order never samples one)
  two_pass     plain_large, then a torch mean over the S x S blocks on the same stream: what a
               caller had to do before the option existed

Each factor runs in a child process of its own under its own time limit (a step that fails,
faults or runs out of time ends the run: nothing more is started on the GPU).  Timing is the
warm frames-in-flight loop: consecutive frames alternate between two streams with a buffer
each, HIP events around windows of >= --reps frames (more when 20 frames take under ~50 ms),
the variants interleaved window by window; the median window is reported as ms per frame,
with the minimum and maximum window as the run-to-run spread.  bytes_written is what a frame
stores to HBM (two_pass also reads the large frame back once).

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

STEP_LIMIT_S = 240
W, H, DEPTH = 1920, 1080, 4


def run_step(s, args):
    import torch
    from rtamd import capi, scenes
    dev = torch.device("cuda", 0)
    streams = [torch.cuda.Stream(dev) for _ in range(2)]
    cfg = scenes.CONFIGS["c2"]
    prims = scenes.to_prims(cfg.scene())
    cam = capi.camera_init(**scenes.camera_args(W, H))
    vcam = capi.supersample_camera(cam, s)
    prec, fmt = capi.RT_PREC_PATH64, capi.RT_OUT_RGB_F32
    fused = capi.Renderer(0)
    fused.set_scene(prims)
    fused.set_option(capi.RT_OPT_SUPERSAMPLE, s)
    plain = capi.Renderer(0)
    plain.set_scene(prims)
    static = capi.Renderer(0)   # plain_large without the measured row order, which supersampled
    static.set_scene(prims)     # frames do not get either: like against like
    static.set_option(capi.RT_OPT_ROW_FEEDBACK, 0)
    small = [torch.zeros((H, W, 3), dtype=torch.float32, device=dev) for _ in streams]
    large = [torch.zeros((H * s, W * s, 3), dtype=torch.float32, device=dev) for _ in streams]
    segs_t = torch.zeros(1, dtype=torch.int64, device=dev)

    def f_fused(k, seg=0):
        fused.render_device(cam, DEPTH, small[k].data_ptr(), prec, 0, fmt, d_segments=seg,
                            stream=streams[k].cuda_stream)

    def f_plain(k, seg=0):
        plain.render_device(vcam, DEPTH, large[k].data_ptr(), prec, 0, fmt, d_segments=seg,
                            stream=streams[k].cuda_stream)

    def f_static(k, seg=0):
        static.render_device(vcam, DEPTH, large[k].data_ptr(), prec, 0, fmt, d_segments=seg,
                             stream=streams[k].cuda_stream)

    def f_two(k, seg=0):
        f_plain(k, seg)
        with torch.cuda.stream(streams[k]):
            torch.mean(large[k].view(H, s, W, s, 3), dim=(1, 3), out=small[k])

    px = W * H * 12
    variants = [("fused", f_fused, px), ("plain_large", f_plain, px * s * s),
                ("plain_large_static_order", f_static, px * s * s),
                ("two_pass", f_two, px * s * s + px)]

    def window(launch, n):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(streams[0])
        streams[1].wait_stream(streams[0])
        for f in range(n):
            launch(f & 1)
        streams[0].wait_stream(streams[1])
        e1.record(streams[0])
        torch.cuda.synchronize()
        return e0.elapsed_time(e1) / n

    rows = []
    for what, launch, nbytes in variants:   # segments of one frame, and the warm-up
        segs_t.zero_()
        launch(0, seg=segs_t.data_ptr())
        torch.cuda.synchronize()
        row = {"what": what, "segments": int(segs_t.item()), "bytes_written": nbytes, "ms": []}
        window(launch, 4)
        per = window(launch, args.reps)
        row["reps"] = int(min(2000, max(args.reps, 50.0 / max(per, 1e-6))))
        rows.append((row, launch))
    # the fused frame is the mean of the large one (fp32 mean of fp32 samples vs the kernel's
    # fp64 tree: equal to rounding)
    torch.cuda.synchronize()
    f_fused(0)
    f_two(1)
    torch.cuda.synchronize()
    max_diff = float((small[0] - small[1]).abs().max().item())
    for _ in range(args.windows):          # interleaved: drift of the box cancels out
        for row, launch in rows:
            row["ms"].append(window(launch, row["reps"]))
    res = {"step": f"S{s}", "factor": s, "config": "c2", "output": [W, H], "depth": DEPTH,
           "precision": "path64", "out_format": "rgb_f32", "frames_in_flight": 2,
           "windows": args.windows, "max_abs_diff_fused_vs_two_pass": max_diff, "results": []}
    for row, _ in rows:
        med = statistics.median(row["ms"])
        res["results"].append({
            "what": row["what"], "segments": row["segments"], "bytes_written": row["bytes_written"],
            "frames_per_window": row["reps"], "ms_median": round(med, 5),
            "ms_min": round(min(row["ms"]), 5), "ms_max": round(max(row["ms"]), 5),
            "gsegments_per_s": round(row["segments"] / (med * 1e-3) / 1e9, 3)})
    by = {r["what"]: r["ms_median"] for r in res["results"]}
    res["fused_over_plain_large"] = round(by["fused"] / by["plain_large"], 4)
    res["fused_over_plain_large_static_order"] = round(by["fused"] / by["plain_large_static_order"], 4)
    res["fused_over_two_pass"] = round(by["fused"] / by["two_pass"], 4)
    fused.close()
    plain.close()
    static.close()
    print(json.dumps(res), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--factors", default="2,4")
    ap.add_argument("--reps", type=int, default=20, help="frames per timed window, at least")
    ap.add_argument("--windows", type=int, default=5)
    ap.add_argument("--out", default="")
    ap.add_argument("--step", type=int, default=0, help="(internal) run this one factor in this process")
    args = ap.parse_args()
    if args.reps < 20:
        ap.error("--reps must be at least 20")
    if args.step:
        run_step(args.step, args)
        return 0
    steps = []
    for s in args.factors.split(","):
        if s not in ("2", "4", "8"):
            ap.error("--factors takes 2, 4 and 8")
        cmd = [sys.executable, os.path.abspath(__file__), "--step", s, "--reps", str(args.reps),
               "--windows", str(args.windows)]
        try:
            p = subprocess.run(cmd, capture_output=True, text=True, timeout=STEP_LIMIT_S)
        except subprocess.TimeoutExpired:
            print(json.dumps({"step": f"S{s}", "error": f"time limit of {STEP_LIMIT_S} s"}), flush=True)
            return 1   # a hung step: nothing more on the GPU
        if p.returncode != 0:
            sys.stderr.write(p.stderr[-2000:])
            print(json.dumps({"step": f"S{s}", "error": f"exit status {p.returncode}"}), flush=True)
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
