#!/usr/bin/env python3
"""Interleaved in-process A/B of an rt_set_option value on frames in flight: the benchmark's
loop (rt_render_device_frames over S streams and S buffers), static or moving camera.
tools/opt_ab.py times one stream; options that act on overlapping frames (RT_OPT_ROW_MIX)
need this one.

    python tools/frames_ab.py --option ROW_MIX --values 0,1,2 --configs c1,c2,c3,c5 \\
        --precisions path64,f32 --streams 2 [--move 0.01]

Per value: us/frame of every round (HIP events on stream 0, all streams joined), min, median
and max.  --streams 1 is the one-stream loop through the same call."""
import argparse
import json
import os
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "ray-tracer-from-scratch_amd"))
from rtamd import capi, scenes  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--option", default="ROW_MIX")
    ap.add_argument("--values", default="0,1")
    ap.add_argument("--configs", default="c2")
    ap.add_argument("--precisions", default="path64")
    ap.add_argument("--streams", type=int, default=2)
    ap.add_argument("--frames", type=int, default=200)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--move", type=float, default=0.0, help="camera step per frame along +x")
    args = ap.parse_args()
    import torch
    dev = torch.device("cuda", 0)
    streams = [torch.cuda.Stream(dev) for _ in range(max(1, args.streams))]
    sp = [s.cuda_stream for s in streams]
    rend = capi.Renderer(0)
    if args.move:
        rend.set_option(capi.RT_OPT_BOX_CACHE, 0)
    opt = getattr(capi, "RT_OPT_" + args.option)
    vals = [int(v) for v in args.values.split(",")]
    for cname in args.configs.split(","):
        cfg = scenes.CONFIGS[cname]
        rend.set_scene(scenes.to_prims(cfg.scene()))
        ca = scenes.camera_args(cfg.width, cfg.height)
        cams = []
        for f in range(args.frames if args.move else 1):
            a = dict(ca)
            a["position"] = (ca["position"][0] + args.move * f, ca["position"][1], ca["position"][2])
            a["lookat"] = (ca["lookat"][0] + args.move * f, ca["lookat"][1], ca["lookat"][2])
            cams.append(capi.camera_init(**a))
        outs = [torch.empty((cfg.height, cfg.width, 3), dtype=torch.float32, device=dev) for _ in streams]
        ptrs = [o.data_ptr() for o in outs]
        for pname in args.precisions.split(","):
            pc = capi.PRECISIONS[pname]
            t = {v: [] for v in vals}
            for rnd in range(args.rounds + 1):    # round 0 warms up (first snapshots) and is dropped
                for v in vals:
                    rend.set_option(opt, v)
                    rend.render_device_frames(cams[:1], cfg.depth, ptrs, pc, streams=sp, nframes=8)
                    torch.cuda.synchronize()
                    e0 = torch.cuda.Event(enable_timing=True)
                    e1 = torch.cuda.Event(enable_timing=True)
                    e0.record(streams[0])
                    for s in streams[1:]:
                        s.wait_stream(streams[0])
                    rend.render_device_frames(cams, cfg.depth, ptrs, pc, streams=sp, nframes=args.frames)
                    for s in streams[1:]:
                        streams[0].wait_stream(s)
                    e1.record(streams[0])
                    torch.cuda.synchronize()
                    if rnd:
                        t[v].append(round(e0.elapsed_time(e1) / args.frames * 1e3, 3))
            r = {"config": cname, "precision": pname, "option": args.option, "streams": len(streams),
                 "frames": args.frames, "move": args.move}
            for v in vals:
                s = sorted(t[v])
                r[f"us[{v}]"] = t[v]
                r[f"min_med_max[{v}]"] = [s[0], s[len(s) // 2], s[-1]]
            print(json.dumps(r), flush=True)
    rend.close()


if __name__ == "__main__":
    main()
