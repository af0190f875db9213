#!/usr/bin/env python3
"""Ambient occlusion (kifs_render_occlusion_async) against the unchanged launch of the same shape, on one GPU.

All frames are the headline workload's (1080p Julia) with the default term (5, 0.02, 0.75, 4.0):
    k = 1   occlusion, without and with the plane   against   kifs_render_geometry_async (the same whole-ray shape)
    k = 2   occlusion                                against   the supersampled kifs_render_async / _batch_async
each as a lone frame and as 48 orbit frames per launch (inline views).  Every form is warmed up; then the two or three
sides of a shape take turns in one process, `--windows` times each, a turn being a synchronised window of launches at
least `--window-s` long between two device events.  Reported per form: the median window's ms per launch and the spread
(max - min over its windows).  The aim, stated per shape: occlusion without the plane takes no longer than its baseline's
median plus the baseline's own spread in this run.

    python tools/occlusion_timing.py --out profiles/occlusion_timing.jsonl
"""
import argparse
import json
import statistics
import sys
from pathlib import Path

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))
import torch  # noqa: E402

import kifs_raymarching_amd as K  # noqa: E402
from kifs_raymarching_amd.configs import WORKLOADS, orbit_camera  # noqa: E402


def window(launch, stream, reps):
    """ms per launch over `reps` launches between two device events, synchronised at both ends."""
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    stream.synchronize()
    a.record(stream)
    for _ in range(reps):
        launch()
    b.record(stream)
    b.synchronize()
    return a.elapsed_time(b) / reps


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--workload", default="cfg2_julia_1080p")
    ap.add_argument("--frames", type=int, nargs="*", default=[1, 48], help="frames per launch (at most 64)")
    ap.add_argument("--factors", type=int, nargs="*", default=[1, 2], help="supersampling factors")
    ap.add_argument("--windows", type=int, default=5)
    ap.add_argument("--window-s", type=float, default=0.5)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--term", default="5,0.02,0.75,4.0", metavar="S,STEP,DECAY,STRENGTH",
                    help="the term (other probe counts say what a probe costs)")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    w = WORKLOADS[args.workload]
    screen, px = w.screen, w.screen.width * w.screen.height
    t = [float(v) for v in args.term.split(",")]
    ao = K.AmbientOcclusion(int(t[0]), t[1], t[2], t[3])
    lines = []
    with K.GraphicState(0, screen_data=screen, camera_data=orbit_camera(w, 0), gui_data=w.gui) as gs:
        gs.set_iters(*w.iters)
        if w.extensions:
            gs.set_extensions(**w.extensions)
        stream = torch.cuda.Stream()
        for k in args.factors:
            for n in args.frames:
                cams = [orbit_camera(w, i) for i in range(n)]
                arr = K.camera_array(cams)
                colour = torch.empty((n, screen.height, screen.width, 4), dtype=torch.uint8, device="cuda:0")
                outs = K.DevicePointers([colour[i] for i in range(n)])
                plane = torch.empty((n, screen.height, screen.width), dtype=torch.float32, device="cuda:0") if k == 1 else None
                geometry = torch.empty((n, screen.height, screen.width, 4), dtype=torch.float32, device="cuda:0") if k == 1 else None
                torch.cuda.synchronize()
                batch = arr if n > 1 else None
                forms = {}
                if k == 1:
                    forms["geometry (baseline)"] = lambda: gs.render_geometry_batch(batch, stream=stream, colour=colour, geometry=geometry)
                elif n == 1:
                    forms["supersampled (baseline)"] = lambda: gs.render_async(colour[0], stream=stream)
                else:
                    forms["supersampled (baseline)"] = lambda: gs.render_batch_async(outs, arr, stream=stream)
                forms["occlusion"] = lambda: gs.render_occlusion_batch(batch, ao=ao, stream=stream, colour=colour)
                if k == 1:
                    forms["occlusion + plane"] = lambda: gs.render_occlusion_batch(batch, ao=ao, stream=stream, colour=colour, plane=plane)
                gs.set_supersampling(k)
                reps = {}
                for name, launch in forms.items():  # warm up, then size the window
                    for _ in range(args.warmup):
                        launch()
                    ms = window(launch, stream, 5)
                    reps[name] = max(5, int(args.window_s * 1e3 / ms) + 1)
                seen = {name: [] for name in forms}
                for _ in range(args.windows):  # the sides take turns
                    for name, launch in forms.items():
                        seen[name].append(window(launch, stream, reps[name]))
                gs.set_supersampling(1)
                base_name = next(iter(forms))
                base = seen[base_name]
                bound = statistics.median(base) + (max(base) - min(base))
                for name, ms in seen.items():
                    med = statistics.median(ms)
                    rec = dict(workload=args.workload, term=args.term, width=screen.width, height=screen.height, k=k, frames_per_launch=n, form=name,
                               ms_per_launch=round(med, 4), spread_ms=round(max(ms) - min(ms), 4), windows=len(ms),
                               launches_per_window=reps[name], gpixel_per_s=round(px * n / (med * 1e-3) / 1e9, 3),
                               vs_baseline=round(med / statistics.median(base), 4))
                    if name == "occlusion":
                        rec["aim_bound_ms"] = round(bound, 4)
                        rec["aim_met"] = bool(med <= bound)
                    print(json.dumps(rec), flush=True)
                    lines.append(rec)
                del colour, plane, geometry
    if args.out:
        Path(args.out).parent.mkdir(parents=True, exist_ok=True)
        with open(args.out, "a") as f:
            f.write("".join(json.dumps(r) + "\n" for r in lines))


if __name__ == "__main__":
    main()
