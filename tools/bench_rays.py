#!/usr/bin/env python3
"""Throughput of the ray-batch path (rt_trace_rays_device) on one GPU.

    python tools/bench_rays.py [--steps camera_c2,random_c2,random_c3,random_c5]
                               [--rays 2000000] [--reps 20] [--windows 5] [--out FILE]

Every GPU step runs in a child process of its own under its own time limit (a step that
fails, faults or runs out of time ends the run: nothing more is started on the GPU).  A step
times the device variant with events on a dedicated stream, warm, over windows of >= --reps
launches (more when 20 launches take under ~50 ms), the variants of a step interleaved
window by window; it reports the median window as ns per ray and segments per second, and
the shader clock (MHz) before and after the timed windows when tools/ubench/
libclock_probe.so has been built.

  camera_c2   the c2 camera's 1920x1080 pixel rays passed as a batch, PATH64 and F64, and in
              the same process the yardstick: the frame kernel at the same precision with
              RT_OPT_TILE_BINS, RT_OPT_EYE_TABLES and RT_OPT_MIRROR_BINS at 0 — the same
              algorithmic work without the frame-only shortcuts.  ratio = frame / rays time.
  random_cN   --rays uniformly random rays (the distribution of tests/golden/rays.npz,
              seeded) on config cN's scene at its depth, PATH64 and F64.
  occluded_cN (--occluded: c2, c3, c5) the occlusion query (rt_occluded_device) and the
              closest-hit-only query (rt_trace_rays_device without radiance) on the same
              --rays random rays and scene, tmax = inf; then on random point pairs (d = b - a)
              with tmax = 1 and inf.  ns per ray of each.

The last line printed is one JSON object {"steps": [...]}; --out also writes it to a file.
"""
import argparse
import ctypes as C
import json
import os
import statistics
import subprocess
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "ray-tracer-from-scratch_amd"))

STEP_LIMIT_S = 240
ALL_STEPS = "camera_c2,random_c2,random_c3,random_c5"
OCCLUDED_STEPS = "occluded_c2,occluded_c3,occluded_c5"


def camera_rays(cam):
    """Pixel rays row-major: pos - ((tl + dx*x) + dy*i), main.cpp:132-133."""
    import numpy as np
    pos, tl = np.array(cam.position[:]), np.array(cam.image_top_left[:])
    dx, dy = np.array(cam.pixel_delta_x[:]), np.array(cam.pixel_delta_y[:])
    i, x = np.meshgrid(np.arange(cam.height, dtype=np.float64),
                       np.arange(cam.width, dtype=np.float64), indexing="ij")
    d = (pos - ((tl + dx * x[..., None]) + dy * i[..., None])).reshape(-1, 3)
    return np.broadcast_to(pos, d.shape).copy(), d


def random_rays(n, seed=20261015):
    import numpy as np
    rng = np.random.default_rng(seed)
    o = rng.uniform([-2, -5, -2], [9, 5, 3], size=(n, 3))
    d = rng.normal(size=(n, 3)) * rng.choice([0.3, 1.0, 2.0], size=(n, 1))
    return o, d


def run_step(step, args):
    import numpy as np
    import torch
    from rtamd import capi, scenes
    dev = torch.device("cuda", 0)
    stream = torch.cuda.Stream(dev)
    kind, cname = step.split("_")
    cfg = scenes.CONFIGS[cname]
    prims = scenes.to_prims(cfg.scene())
    cam = capi.camera_init(**scenes.camera_args(cfg.width, cfg.height))
    o, d = camera_rays(cam) if kind == "camera" else random_rays(args.rays)
    n = len(o)
    t_o, t_d = torch.from_numpy(o).to(dev), torch.from_numpy(d).to(dev)
    out = torch.empty((n, 3), dtype=torch.float32, device=dev)
    segs_t = torch.zeros(1, dtype=torch.int64, device=dev)
    rend = capi.Renderer(0)       # the ray batches (and nothing else: options at their defaults)
    rend.set_scene(prims)
    frame = None
    if kind == "camera":
        frame = capi.Renderer(0)  # the yardstick: frame kernels without the frame-only shortcuts
        for opt in (capi.RT_OPT_TILE_BINS, capi.RT_OPT_EYE_TABLES, capi.RT_OPT_MIRROR_BINS):
            frame.set_option(opt, 0)
        frame.set_scene(prims)
    clk = None
    clk_path = os.path.join(REPO, "tools", "ubench", "libclock_probe.so")
    if os.path.exists(clk_path):
        clk = C.CDLL(clk_path)
        clk.clock_probe.argtypes = [C.c_void_p, C.c_void_p, C.c_ulonglong]
    cbuf = torch.zeros((2, 2), dtype=torch.int64, device=dev)
    sp = stream.cuda_stream

    variants = []
    for pname in ("path64", "f64"):
        prec = capi.PRECISIONS[pname]
        variants.append(("rays", pname, lambda prec=prec, seg=0: rend.trace_rays_device(
            t_o.data_ptr(), t_d.data_ptr(), n, cfg.depth, out.data_ptr(), 0, prec, 0,
            capi.RT_OUT_RGB_F32, d_segments=seg, stream=sp)))
        if frame is not None:
            variants.append(("frame_noshortcuts", pname, lambda prec=prec, seg=0: frame.render_device(
                cam, cfg.depth, out.data_ptr(), prec, 0, capi.RT_OUT_RGB_F32, d_segments=seg,
                stream=sp)))
    rows = []
    for what, pname, launch in variants:   # segments of one launch, and the warm-up
        segs_t.zero_()
        launch(seg=segs_t.data_ptr())
        torch.cuda.synchronize()
        row = {"what": what, "precision": pname, "segments": int(segs_t.item()), "ms": []}
        for _ in range(3):
            launch()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(stream)
        for _ in range(args.reps):
            launch()
        e1.record(stream)
        torch.cuda.synchronize()
        per = e0.elapsed_time(e1) / args.reps
        row["reps"] = int(min(2000, max(args.reps, 50.0 / max(per, 1e-6))))
        rows.append((row, launch))
    if clk is not None:
        clk.clock_probe(C.c_void_p(sp), C.c_void_p(cbuf[0].data_ptr()), 200)
    for _ in range(args.windows):          # interleaved: drift of the box cancels out
        for row, launch in rows:
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(stream)
            for _ in range(row["reps"]):
                launch()
            e1.record(stream)
            torch.cuda.synchronize()
            row["ms"].append(e0.elapsed_time(e1) / row["reps"])
    if clk is not None:
        clk.clock_probe(C.c_void_p(sp), C.c_void_p(cbuf[1].data_ptr()), 200)
    torch.cuda.synchronize()
    res = {"step": step, "config": cname, "rays": n, "depth": cfg.depth, "windows": args.windows,
           "results": []}
    for row, _ in rows:
        med = statistics.median(row["ms"])
        res["results"].append({
            "what": row["what"], "precision": row["precision"], "segments": row["segments"],
            "launches_per_window": row["reps"], "ms_median": round(med, 5),
            "ms_min": round(min(row["ms"]), 5), "ms_max": round(max(row["ms"]), 5),
            "ns_per_ray": round(med * 1e6 / n, 4),
            "gsegments_per_s": round(row["segments"] / (med * 1e-3) / 1e9, 3)})
    if frame is not None:
        by = {(r["what"], r["precision"]): r for r in res["results"]}
        res["ratio_frame_over_rays"] = {
            p: round(by[("frame_noshortcuts", p)]["ms_median"] / by[("rays", p)]["ms_median"], 4)
            for p in ("path64", "f64")}
        frame.close()
    if clk is not None:
        cb = cbuf.cpu().numpy()
        res["shader_mhz_before_after"] = [round(100.0 * float(c[0]) / max(1.0, float(c[1])), 1) for c in cb]
    rend.close()
    print(json.dumps(res), flush=True)


def run_occluded_step(step, args):
    """occluded_cN: the occlusion query against the closest-hit-only query (want_rgb=False:
    hit records, no shading) on the same rays and scene in one process.  Random rays with
    tmax = inf for both, then random point pairs in the same box (d = b - a) with tmax = 1 for
    the occlusion query — closest-hit has no limit to give."""
    import numpy as np
    import torch
    from rtamd import capi, scenes
    dev = torch.device("cuda", 0)
    stream = torch.cuda.Stream(dev)
    cname = step.split("_")[1]
    cfg = scenes.CONFIGS[cname]
    rend = capi.Renderer(0)
    rend.set_scene(scenes.to_prims(cfg.scene()))
    n = args.rays
    o, d = random_rays(n)
    rng = np.random.default_rng(20261020)
    b = rng.uniform([-2, -5, -2], [9, 5, 3], size=(n, 3))
    sp = stream.cuda_stream
    t_o = torch.from_numpy(o).to(dev)
    t_d = torch.from_numpy(d).to(dev)
    t_pd = torch.from_numpy(b - o).to(dev)
    t_one = torch.ones(n, dtype=torch.float64, device=dev)
    mask = torch.zeros(n, dtype=torch.uint8, device=dev)
    hits = torch.zeros(n * 40, dtype=torch.uint8, device=dev)
    cnt = torch.zeros(1, dtype=torch.int64, device=dev)

    def occ(dirs, tmax):
        return lambda c=0: rend.occluded_device(t_o.data_ptr(), dirs.data_ptr(), tmax, n,
                                                mask.data_ptr(), c, sp)

    def closest(dirs):
        return lambda c=0: rend.trace_rays_device(t_o.data_ptr(), dirs.data_ptr(), n, 0, 0,
                                                  hits.data_ptr(), stream=sp)

    variants = [("occluded", "random", "inf", occ(t_d, 0)),
                ("closest_hit", "random", "-", closest(t_d)),
                ("occluded", "point_pairs", "1", occ(t_pd, t_one.data_ptr())),
                ("occluded", "point_pairs", "inf", occ(t_pd, 0)),
                ("closest_hit", "point_pairs", "-", closest(t_pd))]
    rows = []
    for what, rays, tmax, launch in variants:
        cnt.zero_()
        torch.cuda.synchronize()
        launch(cnt.data_ptr())
        torch.cuda.synchronize()
        row = {"what": what, "rays": rays, "tmax": tmax, "ms": []}
        if what == "occluded":
            row["occluded_fraction"] = round(int(cnt.item()) / n, 4)
        for _ in range(3):
            launch()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(stream)
        for _ in range(args.reps):
            launch()
        e1.record(stream)
        torch.cuda.synchronize()
        per = e0.elapsed_time(e1) / args.reps
        row["reps"] = int(min(2000, max(args.reps, 50.0 / max(per, 1e-6))))
        rows.append((row, launch))
    for _ in range(args.windows):          # interleaved, as run_step
        for row, launch in rows:
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(stream)
            for _ in range(row["reps"]):
                launch()
            e1.record(stream)
            torch.cuda.synchronize()
            row["ms"].append(e0.elapsed_time(e1) / row["reps"])
    res = {"step": step, "config": cname, "rays": n, "windows": args.windows, "results": []}
    for row, _ in rows:
        med = statistics.median(row["ms"])
        r = {k: v for k, v in row.items() if k not in ("ms", "reps")}
        r.update({"launches_per_window": row["reps"], "ms_median": round(med, 5),
                  "ms_min": round(min(row["ms"]), 5), "ms_max": round(max(row["ms"]), 5),
                  "ns_per_ray": round(med * 1e6 / n, 4)})
        res["results"].append(r)
    rend.close()
    print(json.dumps(res), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", default="")
    ap.add_argument("--occluded", action="store_true",
                    help="the occlusion query against closest-hit (steps occluded_cN)")
    ap.add_argument("--rays", type=int, default=2_000_000)
    ap.add_argument("--reps", type=int, default=20, help="launches per timed window, at least")
    ap.add_argument("--windows", type=int, default=5)
    ap.add_argument("--out", default="")
    ap.add_argument("--step", default="", help="(internal) run this one step in this process")
    args = ap.parse_args()
    if args.reps < 20:
        ap.error("--reps must be at least 20")
    if args.step:
        if args.step.startswith("occluded_"):
            run_occluded_step(args.step, args)
        else:
            run_step(args.step, args)
        return 0
    steps = []
    for step in (args.steps or (OCCLUDED_STEPS if args.occluded else ALL_STEPS)).split(","):
        cmd = [sys.executable, os.path.abspath(__file__), "--step", step, "--rays", str(args.rays),
               "--reps", str(args.reps), "--windows", str(args.windows)]
        try:
            p = subprocess.run(cmd, capture_output=True, text=True, timeout=STEP_LIMIT_S)
        except subprocess.TimeoutExpired:
            print(json.dumps({"step": step, "error": f"time limit of {STEP_LIMIT_S} s"}), flush=True)
            return 1   # a hung step: nothing more on the GPU
        if p.returncode != 0:
            sys.stderr.write(p.stderr[-2000:])
            print(json.dumps({"step": step, "error": f"exit status {p.returncode}"}), flush=True)
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
