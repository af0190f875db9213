#!/usr/bin/env python3
"""The geometry output (kifs_render_geometry_async) against the plain launches it stands beside, on one GPU: for each
workload the lone frame and launches of 8 and 48 orbit frames, ms per launch from the library's device-event pairs
(kifs_set_profiling) after warm-up.  Forms:
    plain       kifs_render_async / kifs_render_batch_async: RGBA8 only
    geometry    kifs_render_geometry_async: RGBA8 plus 16 bytes per pixel
    background  the plain launch with the camera turned away from the scene: every tile leaves at the culls, so the
                launch is its stores and nothing else -- bytes / time is the write rate the plain path reaches
The forms that need no geometry entry point run on a tree from before it (--forms plain background), which is how the
parent commit's figures in profiles/r07/geometry_bench.jsonl were taken on the same box.

    python tools/geometry_bench.py --out profiles/r07/geometry_bench.jsonl
"""
import argparse
import json
import sys
from pathlib import Path

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))
import torch  # noqa: E402

import kifs_raymarching_amd as K  # noqa: E402
from kifs_raymarching_amd.configs import WORKLOADS, orbit_camera  # noqa: E402


def turned_away(cam):
    """The camera's uniform image looking the other way (the view direction is minus the first matrix column)."""
    u = cam.into_buffer_data()
    for r in range(3):
        u.matrix[0][r] = -u.matrix[0][r]
    return u


def measure(w, form, frames, warmup, reps):
    """Mean / min ms per launch of `frames` orbit frames (1 = a lone frame)."""
    screen = w.screen
    cams = [orbit_camera(w, i) for i in range(frames)]
    if form == "background":
        cams = [turned_away(c) for c in cams]
    with K.GraphicState(0, screen_data=screen, camera_data=orbit_camera(w, 0), gui_data=w.gui) as gs:
        gs.set_iters(*w.iters)
        if form == "background":
            gs.set_raw_uniforms(camera=cams[0])
        colour = torch.empty((frames, screen.height, screen.width, 4), dtype=torch.uint8, device="cuda:0")
        geometry = (torch.empty((frames, screen.height, screen.width, 4), dtype=torch.float32, device="cuda:0")
                    if form == "geometry" else None)
        outs = [colour[i] for i in range(frames)]
        torch.cuda.synchronize()
        stream = torch.cuda.Stream()

        def launch():
            if form == "geometry":
                gs.render_geometry_batch(cams if frames > 1 else None, stream=stream, colour=colour, geometry=geometry)
            elif frames == 1:
                gs.render_async(outs[0], stream=stream)
            else:
                gs.render_batch_async(outs, cams, stream=stream)

        for _ in range(warmup):
            launch()
        stream.synchronize()
        gs.set_profiling(1)
        for _ in range(reps):
            launch()
        stream.synchronize()
        n, mean_ms, min_ms, _ = gs.profile_read()
        gs.set_profiling(0)
        kernel = gs.debug_last_kernel()
    assert n == reps, (n, reps)
    return mean_ms, min_ms, kernel


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--workloads", nargs="*", default=["cfg2_julia_1080p", "cfg3_sierpinski_1080p"])
    ap.add_argument("--forms", nargs="*", default=["plain", "geometry", "background"],
                    choices=["plain", "geometry", "background"])
    ap.add_argument("--batches", type=int, nargs="*", default=[1, 8, 48])
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--reps", type=int, default=40)
    ap.add_argument("--tree", default="this", help="label of the tree the figures belong to (this / parent)")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    lines = []
    for name in args.workloads:
        w = WORKLOADS[name]
        px = w.screen.width * w.screen.height
        for b in args.batches:
            for form in args.forms:
                mean_ms, min_ms, kernel = measure(w, form, b, args.warmup, args.reps)
                bytes_written = px * b * (20 if form == "geometry" else 4)
                rec = dict(tree=args.tree, workload=name, form=form, frames_per_launch=b, width=w.screen.width,
                           height=w.screen.height, ms_per_launch=round(mean_ms, 4), min_ms=round(min_ms, 4), kernel=kernel,
                           gpixel_per_s=round(px * b / (mean_ms * 1e-3) / 1e9, 3),
                           written_gb_per_s=round(bytes_written / (mean_ms * 1e-3) / 1e9, 1))
                print(json.dumps(rec), flush=True)
                lines.append(rec)
    if args.out:
        Path(args.out).parent.mkdir(parents=True, exist_ok=True)
        with open(args.out, "a") as f:
            f.write("".join(json.dumps(r) + "\n" for r in lines))


if __name__ == "__main__":
    main()
