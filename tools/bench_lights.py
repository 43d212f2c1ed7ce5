#!/usr/bin/env python3
"""Scene lights (rt_set_lights): what n coloured lights cost, with and without RT_FLAG_SHADOWS,
against the same build's light-less and shadowed frames, on one GPU.

    python tools/bench_lights.py [--configs c2,c3] [--reps 20] [--windows 5] [--out FILE]

Per config (c2: 8 spheres + 4 walls, depth 4, 1920x1080; c3: 64 spheres + 6 walls, depth 6,
3840x2160), PATH64, RT_OUT_RGB_F32, these variants are timed:

  plain / shadows            rt_render_device on a ctx without lights, without / with the flag
                             (the plain and shadow kernels)
  lights_N / lights_N_sh     the same with N = 1, 2, 4, 8 lights set (the lights kernels); N = 1
                             is the reference's light {(0,0,0), (1,1,1)} through the general
                             path, N = 2, 4, 8 are tests/lights_fixture.py's K2, K4, K8

and these ratios reported: lights_N over plain, lights_N_sh over shadows, and the prediction
"an N-light shadowed frame costs less than N shadowed frames" (lights_N_sh over N x shadows,
below 1 = confirmed: the closest-hit scan, pos, N and sp are shared across the lights).

Method as tools/bench_shadows.py: each config runs in a child process of its own under its own
time limit (a step that fails, faults or runs out of time ends the run: nothing more is started
on the GPU).  Timing is the warm frames-in-flight loop: consecutive frames alternate between two
streams with buffers of their own, HIP events around windows of >= --reps frames (more when
they take under ~50 ms), the variants interleaved window by window; the median window is
reported as ms per frame, with the minimum and maximum window as the run-to-run spread.  The
shader clock rocm-smi reports before and after is recorded as read (nothing is set).

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

ONE = [((0, 0, 0), (1, 1, 1))]
K2 = [((1, -2, 2.5), (1, .8, .6)), ((6, 1.5, 3), (.3, .5, 1))]
K4 = K2 + [((0, 0, 0), (.5, .5, .5)), ((9, -3, .5), (.6, .2, .2))]
K8 = K4 + [((4, 0, 2.9), (.2, .2, .2)), ((1, 3.5, 1), (.1, .3, .1)), ((7, -2, 2.95), (.25, .1, .3)),
           ((-1, 1, -.5), (.3, .3, .1))]
SETS = {1: ONE, 2: K2, 4: K4, 8: K8}


def clocks():
    try:
        out = subprocess.run(["rocm-smi", "--showclocks", "-d", "0"], capture_output=True, text=True,
                             timeout=20).stdout
        return [ln.strip() for ln in out.splitlines() if "sclk" in ln or "mclk" in ln][:4]
    except Exception as e:  # the tool is optional
        return [f"unavailable: {e}"]


def run_step(name, args):
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
    img = [torch.zeros((H, W, 3), dtype=torch.float32, device=dev) for _ in streams]
    segs_t = torch.zeros(1, dtype=torch.int64, device=dev)

    def variant(nl, flags):
        # the records travel with each launch: rt_set_lights in front of a window costs no
        # synchronisation and does not touch frames already enqueued
        def setup():
            r.set_lights(SETS[nl] if nl else None)

        def go(k, seg=0):
            r.render_device(cam, depth, img[k].data_ptr(), prec, flags, fmt, d_segments=seg,
                            stream=streams[k].cuda_stream)
        return setup, go

    variants = [("plain", variant(0, 0)), ("shadows", variant(0, SH))]
    for nl in (1, 2, 4, 8):
        variants += [(f"lights_{nl}", variant(nl, 0)), (f"lights_{nl}_sh", variant(nl, SH))]

    def window(v, nf):
        setup, launch = v
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
    for what, v in variants:   # segments of one frame, and the warm-up
        segs_t.zero_()
        v[0]()
        v[1](0, seg=segs_t.data_ptr())
        torch.cuda.synchronize()
        row = {"what": what, "segments": int(segs_t.item()), "ms": []}
        window(v, 4)
        per = window(v, args.reps)
        row["reps"] = int(min(2000, max(args.reps, 50.0 / max(per, 1e-6))))
        rows.append((row, v))
    for _ in range(args.windows):          # interleaved: drift of the box cancels out
        for row, v in rows:
            row["ms"].append(window(v, row["reps"]))
    res = {"step": name, "config": name, "output": [W, H], "depth": depth, "precision": "path64",
           "out_format": "rgb_f32", "frames_in_flight": 2, "windows": args.windows,
           "clocks_before": clk0, "clocks_after": clocks(), "results": [], "ratios": {}}
    for row, _ in rows:
        med = statistics.median(row["ms"])
        res["results"].append({"what": row["what"], "segments": row["segments"],
                               "frames_per_window": row["reps"], "ms_median": round(med, 5),
                               "ms_min": round(min(row["ms"]), 5), "ms_max": round(max(row["ms"]), 5)})
    by = {x["what"]: x["ms_median"] for x in res["results"]}
    for nl in (1, 2, 4, 8):
        res["ratios"][f"lights_{nl}_over_plain"] = round(by[f"lights_{nl}"] / by["plain"], 4)
        res["ratios"][f"lights_{nl}_sh_over_shadows"] = round(by[f"lights_{nl}_sh"] / by["shadows"], 4)
        res["ratios"][f"lights_{nl}_sh_over_{nl}_shadowed_frames"] = round(
            by[f"lights_{nl}_sh"] / (nl * by["shadows"]), 4)
    res["prediction_n_lights_cheaper_than_n_shadowed_frames"] = all(
        res["ratios"][f"lights_{nl}_sh_over_{nl}_shadowed_frames"] < 1.0 for nl in (2, 4, 8))
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
