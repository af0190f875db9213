#!/usr/bin/env python3
"""Progressive accumulation (kifs_render_accumulate_resume_async) on one GPU and in one process: what carrying the plane
of sums costs a pass.

For each (count, samples) -- default (1, 16), (6, 8), (48, 4) of cfg2_julia_1080p -- the motion-blur sub-frame cameras of
`count` consecutive orbit frames (configs.shutter_cameras, shutter 0.5) through the cells of configs.jitter_cells at
--grid 4 are rendered by

  jittered   kifs_render_accumulate_jittered_async: the one-launch form, which a checkout without the new call has too
             (--tree DIR: the A/B against the parent commit);
  first      a pass with prior_samples = 0 and a picture: the plane is written, not read;
  resume     a pass with prior_samples = 16 and a picture: the plane is read and written -- 32 bytes per pixel and frame
             more than the jittered call moves;
  silent     the same pass without a picture (dev_outs NULL).

Before any timing the bytes are compared: a first pass against the jittered call (identity (a)), and the views of the
jittered call as two passes against the one call (identity (b)).  Each form is timed with a pair of device events around
its call on one stream after --warmup launches (mean and minimum over --reps repetitions).

    python tools/progressive_bench.py --out profiles/r13/progressive_bench.jsonl
"""
import argparse
import json
import sys
from pathlib import Path

ap = argparse.ArgumentParser()
ap.add_argument("--tree", default=str(Path(__file__).resolve().parent.parent), help="the checkout whose package is measured")
ap.add_argument("--label", default="this")
ap.add_argument("--workload", default="cfg2_julia_1080p")
ap.add_argument("--rows", default="1x16,6x8,48x4", help="count x samples, comma separated")
ap.add_argument("--grid", type=int, default=4)
ap.add_argument("--prior", type=int, default=16, help="prior_samples of the timed resume passes")
ap.add_argument("--shutter", type=float, default=0.5)
ap.add_argument("--warmup", type=int, default=10)
ap.add_argument("--reps", type=int, default=40)
ap.add_argument("--out", default=None)
args = ap.parse_args()
sys.path.insert(0, args.tree)
import torch  # noqa: E402

import kifs_raymarching_amd as K  # noqa: E402
from kifs_raymarching_amd import configs  # noqa: E402
from kifs_raymarching_amd.configs import WORKLOADS, shutter_cameras  # noqa: E402

HAS_RESUME = hasattr(K.GraphicState, "render_accumulate_resume")


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
    rec = dict(label=args.label, resume_call=HAS_RESUME, workload=args.workload, warmup=args.warmup, reps=args.reps, **rec)
    print(json.dumps(rec), flush=True)
    if args.out:
        Path(args.out).parent.mkdir(parents=True, exist_ok=True)
        with open(args.out, "a") as f:
            f.write(json.dumps(rec) + "\n")


def main():
    w = WORKLOADS[args.workload]
    width, height = w.screen.width, w.screen.height
    g = args.grid
    with K.GraphicState(0, screen_data=w.screen, camera_data=w.camera, gui_data=w.gui) as gs:
        gs.set_iters(*w.iters)
        if w.extensions:
            gs.set_extensions(**w.extensions)
        stream = torch.cuda.Stream()
        for shape in filter(None, args.rows.split(",")):
            count, samples = (int(v) for v in shape.split("x"))
            views = [c.into_buffer_data() for f in range(count) for c in shutter_cameras(w, f, samples, args.shutter)]
            cams = K.camera_array(views)
            pairs = [c for f in range(count) for c in configs.jitter_cells(g, samples, f)]
            cells = (K._lib.KifsSubpixel * len(pairs))(*[K._lib.KifsSubpixel(i, j) for i, j in pairs])
            one = torch.zeros((count, height, width, 4), dtype=torch.uint8, device="cuda:0")
            torch.cuda.synchronize()
            rec = dict(count=count, samples=samples, grid=g, shutter=args.shutter,
                       plane_bytes_read_and_written=32 * width * height * count)
            gs.render_accumulate(cams, samples, outs=one, stream=stream, jitter=(g, cells))
            stream.synchronize()
            if HAS_RESUME:
                sums = torch.full((count, height, width, 4), float("nan"), dtype=torch.float32, device="cuda:0")
                out = torch.zeros_like(one)
                torch.cuda.synchronize()
                # identity (a): a first pass over a plane of NaNs is the jittered call, byte for byte
                gs.render_accumulate_resume(sums, 0, cams, samples, outs=out, stream=stream, jitter=(g, cells))
                stream.synchronize()
                if not bool((out == one).all()) or bool(torch.isnan(sums).any()):
                    raise SystemExit("progressive_bench: a first pass differs from the jittered call")
                # identity (b): the same views as two passes
                if samples > 1:
                    a = samples // 2
                    halves = [[f * samples + s for f in range(count) for s in rng] for rng in (range(a), range(a, samples))]
                    out.zero_()
                    sums.fill_(float("nan"))
                    torch.cuda.synchronize()
                    gs.render_accumulate_resume(sums, 0, [views[v] for v in halves[0]], a, picture=False, stream=stream,
                                                jitter=(g, [pairs[v] for v in halves[0]]))
                    gs.render_accumulate_resume(sums, a, [views[v] for v in halves[1]], samples - a, outs=out, stream=stream,
                                                jitter=(g, [pairs[v] for v in halves[1]]))
                    stream.synchronize()
                    if not bool((out == one).all()) or not bool((sums[..., 3] == float(samples)).all()):
                        raise SystemExit("progressive_bench: two passes differ from the one call")
                rec["identities_hold"] = True
                rec["first_ms"], rec["first_min_ms"] = timed(
                    stream, lambda: gs.render_accumulate_resume(sums, 0, cams, samples, outs=out, stream=stream, jitter=(g, cells)))
                rec["prior"] = args.prior
                rec["resume_ms"], rec["resume_min_ms"] = timed(
                    stream, lambda: gs.render_accumulate_resume(sums, args.prior, cams, samples, outs=out, stream=stream, jitter=(g, cells)))
                rec["silent_ms"], rec["silent_min_ms"] = timed(
                    stream, lambda: gs.render_accumulate_resume(sums, args.prior, cams, samples, picture=False, stream=stream,
                                                                jitter=(g, cells)))
                del sums, out
            rec["jittered_ms"], rec["jittered_min_ms"] = timed(
                stream, lambda: gs.render_accumulate(cams, samples, outs=one, stream=stream, jitter=(g, cells)))
            if HAS_RESUME:
                rec["resume_over_jittered"] = round(rec["resume_ms"] / rec["jittered_ms"], 4)
            emit(rec)
            del one


if __name__ == "__main__":
    main()
