#!/usr/bin/env python3
"""Ray queries (kifs_trace_rays_async) against the frame-shaped call they generalise, on one GPU.  For each workload the
rays are the pixel rays of its lone frame (configs.pixel_rays), so the same 2 073 600 marches run through
    geometry        kifs_render_geometry_async of that frame: one origin in scalar registers, the hand-written Julia
                    loop, the wave culls -- the only form a tree from before the ray call can run (--tree parent)
    trace           kifs_trace_rays_async, both outputs, the rays in pixel order: what per-lane origins, the plain Julia
                    loop and the absent wave and tile culls cost
    trace_shuffled  the same rays in a seeded random order: the price of incoherent waves
    trace_geometry  the texels alone        trace_colour  the pixels alone
Before any timing the trace's words are compared with the frame's: texels with the geometry plane, pixels with the
frame's bytes, the shuffled call with the permuted unshuffled one.  Timing: a torch event pair around every launch on one
stream, after warm-up; mean and min of --reps launches; --runs runs per form.  --root PATH measures the package of
another checkout (the parent commit's tree, built there) with this script: only `geometry` exists in it.

    python tools/rays_bench.py --out profiles/r15/rays_bench.jsonl
    python tools/rays_bench.py --tree parent --root build_variants/parent --forms geometry --out profiles/r15/rays_bench.jsonl
"""
import argparse
import json
import sys
from pathlib import Path

FORMS = ["geometry", "trace", "trace_shuffled", "trace_geometry", "trace_colour"]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--workloads", nargs="*", default=["cfg2_julia_1080p", "cfg3_sierpinski_1080p"])
    ap.add_argument("--forms", nargs="*", default=FORMS, choices=FORMS)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--reps", type=int, default=40)
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--first-run", type=int, default=0, help="the number of the first run (trees alternate call by call)")
    ap.add_argument("--tree", default="this", help="label of the tree the figures belong to (this / parent)")
    ap.add_argument("--root", default=None, help="the checkout whose package is measured (default: this script's)")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    root = Path(args.root).resolve() if args.root else Path(__file__).resolve().parent.parent
    sys.path.insert(0, str(root))
    import numpy as np
    import torch

    import kifs_raymarching_amd as K
    from kifs_raymarching_amd.configs import WORKLOADS
    assert Path(K.__file__).resolve().parent.parent == root, K.__file__

    def timed(launch, stream):
        for _ in range(args.warmup):
            launch()
        stream.synchronize()
        pairs = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(args.reps)]
        for a, b in pairs:
            a.record(stream)
            launch()
            b.record(stream)
        stream.synchronize()
        ms = [a.elapsed_time(b) for a, b in pairs]
        return sum(ms) / len(ms), min(ms)

    lines = []
    for name in args.workloads:
        w = WORKLOADS[name]
        width, height = w.screen.width, w.screen.height
        n = width * height
        with K.GraphicState(0, screen_data=w.screen, camera_data=w.camera, gui_data=w.gui) as gs:
            gs.set_iters(*w.iters)
            stream = torch.cuda.Stream()
            colour = torch.empty((1, height, width, 4), dtype=torch.uint8, device="cuda:0")
            plane = torch.empty((1, height, width, 4), dtype=torch.float32, device="cuda:0")
            launches = {"geometry": lambda: gs.render_geometry_batch(None, stream=stream, colour=colour, geometry=plane)}
            if any(f != "geometry" for f in args.forms):
                from kifs_raymarching_amd.configs import pixel_rays
                host = pixel_rays(w.screen, w.camera)
                perm = np.random.default_rng(20261020).permutation(n)
                rays = torch.from_numpy(host).to("cuda:0")
                shuffled = torch.from_numpy(np.ascontiguousarray(host[perm])).to("cuda:0")
                # byte comparison before any timing
                frame = gs.render()
                gs.render_geometry_batch(None, colour=colour, geometry=plane)
                geom, rgba = gs.trace_rays(rays)
                sgeom, srgba = gs.trace_rays(shuffled)
                gs.synchronize()
                bits = lambda t: t.cpu().numpy().view(np.uint32)
                assert (bits(geom) == bits(plane).reshape(-1, 4)).all(), "texels differ from the geometry plane"
                assert (rgba.cpu().numpy() == frame.reshape(-1, 4)).all(), "pixels differ from the frame"
                assert (bits(sgeom) == bits(geom)[perm]).all() and (srgba.cpu().numpy() == rgba.cpu().numpy()[perm]).all(), "shuffled"
                hits = int(torch.isfinite(geom[:, 3]).sum())
                del geom, rgba, sgeom, srgba
                launches.update({
                    "trace": lambda: gs.trace_rays(rays, stream=stream),
                    "trace_shuffled": lambda: gs.trace_rays(shuffled, stream=stream),
                    "trace_geometry": lambda: gs.trace_rays(rays, colours=False, stream=stream),
                    "trace_colour": lambda: gs.trace_rays(rays, geometry=False, stream=stream),
                })
            else:
                hits = None
            torch.cuda.synchronize()
            for run in range(args.runs):
                for form in args.forms:
                    mean_ms, min_ms = timed(launches[form], stream)
                    rec = dict(tree=args.tree, workload=name, form=form, run=args.first_run + run, rays=n, rays_hit=hits, ms_per_launch=round(mean_ms, 4),
                               min_ms=round(min_ms, 4), grays_per_s=round(n / (mean_ms * 1e-3) / 1e9, 3), reps=args.reps)
                    print(json.dumps(rec), flush=True)
                    lines.append(rec)
    if args.out:
        Path(args.out).parent.mkdir(parents=True, exist_ok=True)
        with open(args.out, "a") as f:
            f.write("".join(json.dumps(r) + "\n" for r in lines))


if __name__ == "__main__":
    main()
