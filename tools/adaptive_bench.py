#!/usr/bin/env python3
"""Adaptive anti-aliasing (kifs_render_adaptive_async) against the launches it is made of and the one it replaces, on
one GPU: for each workload the lone frame and launches of 8 and 48 orbit frames, ms per launch between two device events
on the launch stream around every call (the library's own profiling pairs bracket one kernel, and this call is three),
mean of `--reps` launches after `--warmup`.  The launches are enqueued back to back, so an event pair also spans any
time the device waits for the host's next enqueue: `enqueue_ms` is the host's wall time per call in that loop, and a row
whose enqueue_ms is not well below its ms_per_launch is marked `host_bound` -- its figure is an upper bound.  The camera
array, the destination pointers' tensor and the counts tensor are prepared once, outside the loop.  Forms:
    plain        kifs_render_async / kifs_render_batch_async
    geometry     kifs_render_geometry_async: pass A of the adaptive call on its own
    ssaa2, ssaa3 kifs_set_supersampling(k): k^2 rays for every pixel
    adaptive2, adaptive3   the adaptive call at k with the default thresholds; edge_share = edge pixels / pixels

    python tools/adaptive_bench.py --out profiles/r08/adaptive_bench.jsonl
"""
import argparse
import json
import sys
import time
from pathlib import Path

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))
import torch  # noqa: E402

import kifs_raymarching_amd as K  # noqa: E402
from kifs_raymarching_amd.configs import WORKLOADS, orbit_camera  # noqa: E402

FORMS = ["plain", "geometry", "ssaa2", "ssaa3", "adaptive2", "adaptive3"]


def measure(w, form, frames, warmup, reps, normal_cos, depth_rel):
    """(mean ms, min ms, kernel name, edge share or None, host ms per enqueue) per launch of `frames` orbit frames (1 = a lone frame)."""
    screen = w.screen
    cams = K.camera_array([orbit_camera(w, i) for i in range(frames)])
    k = int(form[-1]) if form[-1].isdigit() else 1
    with K.GraphicState(0, screen_data=screen, camera_data=orbit_camera(w, 0), gui_data=w.gui) as gs:
        gs.set_iters(*w.iters)
        if form.startswith("ssaa"):
            gs.set_supersampling(k)
        colour = torch.empty((frames, screen.height, screen.width, 4), dtype=torch.uint8, device="cuda:0")
        geometry = (torch.empty((frames, screen.height, screen.width, 4), dtype=torch.float32, device="cuda:0")
                    if form == "geometry" else None)
        outs = [colour[i] for i in range(frames)]
        torch.cuda.synchronize()
        stream = torch.cuda.Stream()
        edges = torch.zeros((frames,), dtype=torch.int32, device="cuda:0") if form.startswith("adaptive") else None
        if form in ("plain", "ssaa2", "ssaa3") and frames > 1:
            outs = K.DevicePointers(outs)
        torch.cuda.synchronize()

        def launch():
            if form.startswith("adaptive"):
                gs.render_adaptive_batch(cams if frames > 1 else None, k=k, normal_cos=normal_cos, depth_rel=depth_rel,
                                         stream=stream, colour=colour, edge_counts=edges)
            elif form == "geometry":
                gs.render_geometry_batch(cams if frames > 1 else None, stream=stream, colour=colour, geometry=geometry)
            elif frames == 1:
                gs.render_async(outs[0], stream=stream)
            else:
                gs.render_batch_async(outs, cams, stream=stream)

        for _ in range(warmup):
            launch()
        stream.synchronize()
        pairs = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(reps)]
        t0 = time.perf_counter()
        for a, b in pairs:
            a.record(stream)
            launch()
            b.record(stream)
        enqueue_ms = (time.perf_counter() - t0) * 1e3 / reps
        stream.synchronize()
        times = [a.elapsed_time(b) for a, b in pairs]
        kernel = gs.debug_last_kernel()
        share = None
        if edges is not None:
            share = float(edges.sum().item()) / (frames * screen.width * screen.height)
    return sum(times) / len(times), min(times), kernel, share, enqueue_ms


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--workloads", nargs="*", default=["cfg2_julia_1080p", "cfg3_sierpinski_1080p"])
    ap.add_argument("--forms", nargs="*", default=FORMS, choices=FORMS)
    ap.add_argument("--batches", type=int, nargs="*", default=[1, 8, 48])
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--reps", type=int, default=40)
    ap.add_argument("--normal-cos", type=float, default=0.9)
    ap.add_argument("--depth-rel", type=float, default=0.05)
    ap.add_argument("--tree", default="this", help="label of the tree the figures belong to (this / parent)")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    lines = []
    for name in args.workloads:
        w = WORKLOADS[name]
        px = w.screen.width * w.screen.height
        for b in args.batches:
            for form in args.forms:
                mean_ms, min_ms, kernel, share, enqueue_ms = measure(w, form, b, args.warmup, args.reps, args.normal_cos, args.depth_rel)
                rec = dict(tree=args.tree, workload=name, form=form, frames_per_launch=b, width=w.screen.width,
                           height=w.screen.height, ms_per_launch=round(mean_ms, 4), min_ms=round(min_ms, 4), kernel=kernel,
                           gpixel_per_s=round(px * b / (mean_ms * 1e-3) / 1e9, 3), enqueue_ms=round(enqueue_ms, 4),
                           host_bound=bool(enqueue_ms > 0.8 * mean_ms))
                if share is not None:
                    rec["edge_share"] = round(share, 5)
                print(json.dumps(rec), flush=True)
                lines.append(rec)
    if args.out:
        Path(args.out).parent.mkdir(parents=True, exist_ok=True)
        with open(args.out, "a") as f:
            f.write("".join(json.dumps(r) + "\n" for r in lines))


if __name__ == "__main__":
    main()
