#!/usr/bin/env python3
"""Jittered accumulated frames (kifs_render_accumulate_jittered_async) on one GPU and in one process, two questions:

  cost   what the jitter itself costs: for each (count, samples) -- default (1, 16), (6, 8), (48, 4) of cfg2_julia_1080p
         -- the motion-blur sub-frame cameras of `count` consecutive orbit frames (configs.shutter_cameras, shutter 0.5)
         rendered by kifs_render_accumulate_async and by the jittered call at --grid 4 with configs.jitter_cells -- and by
         the jittered call at a grid of 3 with every cell (1, 1), the pixel centre: the jitter kernel marching the very
         rays of the unjittered call (the same bytes, compared first), which separates the kernel's own cost from that of
         other rays.
  grid   the whole grid against the supersampling kernel: `count` orbit frames at g x g -- default 1x2, 1x3, 48x2, 16x3
         (count * g^2 <= 512) -- rendered by the jittered call (samples = g^2, cells NULL, one camera per frame) and by
         kifs_set_supersampling(g) + kifs_render_batch_async.  The two write the same bytes: compared before any timing.

Each form is timed with a pair of device events around its calls on one stream after --warmup launches (mean and minimum
over --reps repetitions).  --tree DIR imports the package from another checkout (one without the jittered call records the
forms it has: the A/B against the parent commit); --label names the run in the records.

    python tools/jitter_bench.py --out profiles/r12/jitter_bench.jsonl
"""
import argparse
import json
import sys
from pathlib import Path

ap = argparse.ArgumentParser()
ap.add_argument("--tree", default=str(Path(__file__).resolve().parent.parent), help="the checkout whose package is measured")
ap.add_argument("--label", default="this")
ap.add_argument("--workload", default="cfg2_julia_1080p")
ap.add_argument("--cost", default="1x16,6x8,48x4", help="count x samples, comma separated ('' = none)")
ap.add_argument("--grid", type=int, default=4, help="the jittered call's grid in the cost rows")
ap.add_argument("--whole", default="1x2,1x3,48x2,16x3", help="count x g, comma separated ('' = none)")
ap.add_argument("--shutter", type=float, default=0.5)
ap.add_argument("--warmup", type=int, default=10)
ap.add_argument("--reps", type=int, default=40)
ap.add_argument("--out", default=None)
args = ap.parse_args()
sys.path.insert(0, args.tree)
import torch  # noqa: E402

import kifs_raymarching_amd as K  # noqa: E402
from kifs_raymarching_amd import configs  # noqa: E402
from kifs_raymarching_amd.configs import WORKLOADS, orbit_camera, shutter_cameras  # noqa: E402

HAS_JITTER = hasattr(configs, "jitter_cells")


def timed(stream, fn):
    """(mean, min) ms of fn() on `stream` between two device events."""
    for _ in range(args.warmup):
        fn()
    stream.synchronize()
    ms = []
    for _ in range(args.reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record(stream)
        fn()
        b.record(stream)
        stream.synchronize()
        ms.append(a.elapsed_time(b))
    return round(sum(ms) / len(ms), 4), round(min(ms), 4)


def emit(rec):
    rec = dict(label=args.label, jittered_call=HAS_JITTER, workload=args.workload, warmup=args.warmup, reps=args.reps, **rec)
    print(json.dumps(rec), flush=True)
    if args.out:
        Path(args.out).parent.mkdir(parents=True, exist_ok=True)
        with open(args.out, "a") as f:
            f.write(json.dumps(rec) + "\n")


def main():
    w = WORKLOADS[args.workload]
    width, height = w.screen.width, w.screen.height
    with K.GraphicState(0, screen_data=w.screen, camera_data=w.camera, gui_data=w.gui) as gs:
        gs.set_iters(*w.iters)
        if w.extensions:
            gs.set_extensions(**w.extensions)
        stream = torch.cuda.Stream()
        for shape in filter(None, args.cost.split(",")):
            count, samples = (int(v) for v in shape.split("x"))
            cams = K.camera_array([c for f in range(count) for c in shutter_cameras(w, f, samples, args.shutter)])
            plain = torch.zeros((count, height, width, 4), dtype=torch.uint8, device="cuda:0")
            torch.cuda.synchronize()
            rec = dict(form="cost", count=count, samples=samples, shutter=args.shutter)
            if HAS_JITTER:
                # before any timing: a grid of 1 is the unjittered call, byte for byte
                one = torch.zeros_like(plain)
                gs.render_accumulate(cams, samples, outs=plain, stream=stream)
                gs.render_accumulate(cams, samples, outs=one, stream=stream, jitter=(1, [(0, 0)] * (count * samples)))
                stream.synchronize()
                if not bool((one == plain).all()):
                    raise SystemExit("jitter_bench: a grid of 1 differs from the unjittered call")
                cells = K._lib.KifsSubpixel * (count * samples)
                cells = cells(*[K._lib.KifsSubpixel(i, j) for f in range(count) for i, j in configs.jitter_cells(args.grid, samples, f)])
                rec["grid"] = args.grid
                rec["jittered_ms"], rec["jittered_min_ms"] = timed(
                    stream, lambda: gs.render_accumulate(cams, samples, outs=one, stream=stream, jitter=(args.grid, cells)))
                centre = (K._lib.KifsSubpixel * (count * samples))(*[K._lib.KifsSubpixel(1, 1)] * (count * samples))
                gs.render_accumulate(cams, samples, outs=one, stream=stream, jitter=(3, centre))
                stream.synchronize()
                if not bool((one == plain).all()):
                    raise SystemExit("jitter_bench: the centre cell of a 3 x 3 grid differs from the unjittered call")
                rec["centre_cell_ms"], rec["centre_cell_min_ms"] = timed(
                    stream, lambda: gs.render_accumulate(cams, samples, outs=one, stream=stream, jitter=(3, centre)))
                del one
            rec["accumulate_ms"], rec["accumulate_min_ms"] = timed(stream, lambda: gs.render_accumulate(cams, samples, outs=plain, stream=stream))
            if HAS_JITTER:
                rec["jittered_over_accumulate"] = round(rec["jittered_ms"] / rec["accumulate_ms"], 3)
            emit(rec)
            del plain
        for shape in filter(None, args.whole.split(",")):
            count, g = (int(v) for v in shape.split("x"))
            frame_cams = [orbit_camera(w, f) for f in range(count)]
            ssaa = torch.zeros((count, height, width, 4), dtype=torch.uint8, device="cuda:0")
            torch.cuda.synchronize()
            outs = [ssaa[i] for i in range(count)]
            rec = dict(form="whole_grid", count=count, grid=g, samples=g * g)

            def supersampled():
                gs.render_batch_async(outs, frame_cams, stream=stream)

            gs.set_supersampling(g)
            supersampled()
            stream.synchronize()
            rec["supersampling_kernel"] = gs.debug_last_kernel()
            rec["supersampling_ms"], rec["supersampling_min_ms"] = timed(stream, supersampled)
            gs.set_supersampling(1)
            if HAS_JITTER:
                cams = K.camera_array([c for c in frame_cams for _ in range(g * g)])
                whole = torch.zeros_like(ssaa)
                gs.render_accumulate(cams, g * g, outs=whole, stream=stream, jitter=(g, None))
                stream.synchronize()
                if not bool((whole == ssaa).all()):
                    raise SystemExit("jitter_bench: the whole grid differs from the supersampled frames")
                rec["frames_equal"] = True
                rec["whole_grid_ms"], rec["whole_grid_min_ms"] = timed(
                    stream, lambda: gs.render_accumulate(cams, g * g, outs=whole, stream=stream, jitter=(g, None)))
                rec["whole_grid_over_supersampling"] = round(rec["whole_grid_ms"] / rec["supersampling_ms"], 3)
                del whole
            emit(rec)
            del ssaa, outs


if __name__ == "__main__":
    main()
