#!/usr/bin/env python3
"""Accumulated frames (kifs_render_accumulate_async) against the launch that marches the same rays without the resolve,
on one GPU and in one process: for each (count, samples) -- default (1, 16), (6, 8), (48, 4) of cfg2_julia_1080p -- the
motion-blur sub-frame cameras of `count` consecutive orbit frames (configs.shutter_cameras, shutter 0.5) are rendered as
    accumulate  kifs_render_accumulate_async: count frames, each the mean of its `samples` sub-frames
    animation   kifs_render_animation_async: the same count * samples views (the workload's options for every one) into
                count * samples frames -- the same whole rays, `samples` times as many stores
both in calls of at most 512 views on the same stream, timed with a pair of device events around each form's calls after
warm-up (mean and minimum over `--reps` repetitions).  Before anything is timed, a one-sample accumulate call is compared
byte for byte with the animated launch's frames.

    python tools/accumulate_bench.py --out profiles/r10/accumulate_bench.jsonl
"""
import argparse
import ctypes as C
import json
import sys
from pathlib import Path

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))
import torch  # noqa: E402

import kifs_raymarching_amd as K  # noqa: E402
from kifs_raymarching_amd.configs import WORKLOADS, shutter_cameras  # noqa: E402


def timed(stream, fn, warmup, reps):
    """(mean, min) ms of fn() on `stream` between two device events."""
    for _ in range(warmup):
        fn()
    stream.synchronize()
    ms = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record(stream)
        fn()
        b.record(stream)
        stream.synchronize()
        ms.append(a.elapsed_time(b))
    return sum(ms) / len(ms), min(ms)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--workload", default="cfg2_julia_1080p", choices=sorted(WORKLOADS))
    ap.add_argument("--shapes", default="1x16,6x8,48x4", help="count x samples, comma separated")
    ap.add_argument("--shutter", type=float, default=0.5)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--reps", type=int, default=40)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    w = WORKLOADS[args.workload]
    width, height = w.screen.width, w.screen.height
    with K.GraphicState(0, screen_data=w.screen, camera_data=w.camera, gui_data=w.gui) as gs:
        gs.set_iters(*w.iters)
        if w.extensions:
            gs.set_extensions(**w.extensions)
        stream = torch.cuda.Stream()
        for shape in args.shapes.split(","):
            count, samples = (int(v) for v in shape.split("x"))
            views = count * samples
            cams = K.camera_array([c for f in range(count) for c in shutter_cameras(w, f, samples, args.shutter)])
            options = K.options_array([w.gui] * views)
            per_call = max(1, K.MAX_BATCH // samples)  # frames per accumulate call: at most 512 views
            acc = torch.zeros((count, height, width, 4), dtype=torch.uint8, device="cuda:0")
            sub = torch.zeros((views, height, width, 4), dtype=torch.uint8, device="cuda:0")
            torch.cuda.synchronize()

            def part(array, first, n):
                return (type(array[0]) * n).from_address(C.addressof(array) + first * C.sizeof(array[0]))

            def accumulate():
                for f in range(0, count, per_call):
                    n = min(per_call, count - f)
                    gs.render_accumulate(part(cams, f * samples, n * samples), samples, outs=acc[f:f + n], stream=stream)

            def animation():
                for v in range(0, views, K.MAX_BATCH):
                    n = min(K.MAX_BATCH, views - v)
                    gs.render_animation(part(options, v, n), cameras=part(cams, v, n), outs=sub[v:v + n], stream=stream)

            # the two forms' inputs are identical: one sample per frame is the animated launch's frame
            one = min(views, 8)
            check = torch.zeros((one, height, width, 4), dtype=torch.uint8, device="cuda:0")
            gs.render_accumulate(part(cams, 0, one), 1, outs=check, stream=stream)
            animation()
            stream.synchronize()
            if not bool((check == sub[:one]).all()):
                raise SystemExit("accumulate_bench: one-sample accumulated frames differ from the animated launch's")
            accumulate()
            kernel = gs.debug_last_kernel()
            a_mean, a_min = timed(stream, accumulate, args.warmup, args.reps)
            m_mean, m_min = timed(stream, animation, args.warmup, args.reps)
            rec = dict(workload=args.workload, count=count, samples=samples, views=views, width=width, height=height,
                       shutter=args.shutter, warmup=args.warmup, reps=args.reps,
                       accumulate_ms=round(a_mean, 4), accumulate_min_ms=round(a_min, 4), accumulate_kernel=kernel,
                       animation_ms=round(m_mean, 4), animation_min_ms=round(m_min, 4),
                       accumulate_over_animation=round(a_mean / m_mean, 3), aim=1.25, aim_met=bool(a_mean <= 1.25 * m_mean),
                       one_sample_frames_equal=True)
            print(json.dumps(rec), flush=True)
            if args.out:
                Path(args.out).parent.mkdir(parents=True, exist_ok=True)
                with open(args.out, "a") as f:
                    f.write(json.dumps(rec) + "\n")
            del acc, sub, check


if __name__ == "__main__":
    main()
