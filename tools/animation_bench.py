#!/usr/bin/env python3
"""A morph in one launch (kifs_render_animation_async) against the only way to render it without that entry point, on one
GPU and in one process: `--frames` frames of a workload (default: 48 of cfg2_julia_1080p) whose constant moves linearly
to `--to`, camera fixed.  Forms, both enqueued on the same stream and timed with a pair of device events around the whole
sequence after warm-up (mean and minimum over `--reps` repetitions):
    animation   one kifs_render_animation_async call
    lone        frames x (kifs_set_options + kifs_render_async)
The two forms' frames are compared byte for byte before anything is timed.

    python tools/animation_bench.py --out profiles/r09/animation_bench.jsonl
"""
import argparse
import json
import sys
from pathlib import Path

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))
import torch  # noqa: E402

import kifs_raymarching_amd as K  # noqa: E402
from kifs_raymarching_amd.configs import WORKLOADS, morph_options  # noqa: E402


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
    ap.add_argument("--frames", type=int, default=48)
    ap.add_argument("--to", type=float, nargs=4, default=[0.3, 0.5, -0.2, 0.1], metavar=("R", "I", "J", "K"))
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    w = WORKLOADS[args.workload]
    n = args.frames
    guis = morph_options(w.gui, K.GuiData(**{**w.gui.__dict__, "constant": tuple(args.to)}), n)
    images = K.options_array(guis)
    with K.GraphicState(0, screen_data=w.screen, camera_data=w.camera, gui_data=w.gui) as gs:
        gs.set_iters(*w.iters)
        if w.extensions:
            gs.set_extensions(**w.extensions)
        frames = torch.zeros((n, w.screen.height, w.screen.width, 4), dtype=torch.uint8, device="cuda:0")
        lone = torch.zeros_like(frames)
        torch.cuda.synchronize()
        stream = torch.cuda.Stream()

        def animation():
            gs.render_animation(images, outs=frames, stream=stream)

        def lone_frames():
            for i in range(n):
                gs.update_options(images[i])
                gs.render_async(lone[i], stream=stream)

        animation()
        kernel = gs.debug_last_kernel()
        lone_frames()
        stream.synchronize()
        if not bool((frames == lone).all()):
            raise SystemExit("animation_bench: the animated launch's frames differ from the lone renders'")
        a_mean, a_min = timed(stream, animation, args.warmup, args.reps)
        l_mean, l_min = timed(stream, lone_frames, args.warmup, args.reps)
        lone_kernel = gs.debug_last_kernel()
    px = w.screen.width * w.screen.height * n
    rec = dict(workload=args.workload, frames=n, width=w.screen.width, height=w.screen.height, to=list(args.to),
               animation_ms=round(a_mean, 4), animation_min_ms=round(a_min, 4), animation_kernel=kernel,
               lone_ms=round(l_mean, 4), lone_min_ms=round(l_min, 4), lone_kernel=lone_kernel,
               lone_over_animation=round(l_mean / a_mean, 3),
               animation_gpixel_per_s=round(px / (a_mean * 1e-3) / 1e9, 2), lone_gpixel_per_s=round(px / (l_mean * 1e-3) / 1e9, 2),
               frames_equal=True)
    print(json.dumps(rec), flush=True)
    if args.out:
        Path(args.out).parent.mkdir(parents=True, exist_ok=True)
        with open(args.out, "a") as f:
            f.write(json.dumps(rec) + "\n")


if __name__ == "__main__":
    main()
