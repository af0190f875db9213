#!/usr/bin/env python3
"""The configurable light (kifs_render_lit_async) against the calls it must equal, on one GPU.

All frames are the headline workload's (1080p Julia), the term the default one (5, 0.02, 0.75, 4.0), at k = 1 and 2, as a
lone frame and as 48 orbit frames per launch (inline views):
    (a) reference light with the term          against   kifs_render_occlusion_async with the same term
    (b) reference light, no term               against   kifs_render_geometry_async (k = 1) or the supersampled
                                                         kifs_render_async / _batch_async (k > 1)
    (c) light A with its highlight and the term against (a)'s own side, the reference light with the term and soft shadows
        against the occlusion call with soft shadows (the same bytes), and light A with highlight, term and soft shadows
        against that: what the highlight and the moved shadow cost
Every form is warmed up; then the forms of a shape take turns in one process, `--windows` times each, a turn being a
synchronised window of launches at least `--window-s` long between two device events.  Reported per form: the median
window's ms per launch and the spread (max - min over its windows).  The aim of row (a): no longer than the occlusion
call's median plus that call's own spread in this run.  (The occlusion kernel is instruction for instruction the parent
commit's, so this tree's occlusion call is the parent's side of row (a).)

    python tools/lighting_timing.py --out profiles/lighting_timing.jsonl
"""
import argparse
import json
import statistics
import sys
from pathlib import Path

import numpy as np

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))
import torch  # noqa: E402

import kifs_raymarching_amd as K  # noqa: E402
from kifs_raymarching_amd.configs import WORKLOADS, orbit_camera  # noqa: E402

SHADOWS = dict(soft_shadow=True, shadow_steps=64, shadow_k=8.0, shadow_t0=0.02, shadow_max_t=10.0)


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
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    w = WORKLOADS[args.workload]
    screen, px = w.screen, w.screen.width * w.screen.height
    ao = K.AmbientOcclusion()
    reference = K.Light()
    d = np.array([-0.55, 0.75, 0.36])
    light_a = K.Light(direction=tuple(float(v) for v in (d / np.linalg.norm(d)).astype(np.float32)), ambient=0.15, diffuse=0.85,
                      specular=(0.6, 0.6, 0.5), shininess_log2=3)
    lines = []
    with K.GraphicState(0, screen_data=screen, camera_data=orbit_camera(w, 0), gui_data=w.gui) as gs:
        gs.set_iters(*w.iters)
        stream = torch.cuda.Stream()

        def shadows(on):
            gs.set_extensions(**SHADOWS) if on else gs.set_extensions(soft_shadow=False)

        for k in args.factors:
            for n in args.frames:
                cams = [orbit_camera(w, i) for i in range(n)]
                arr = K.camera_array(cams)
                colour = torch.empty((n, screen.height, screen.width, 4), dtype=torch.uint8, device="cuda:0")
                outs = K.DevicePointers([colour[i] for i in range(n)])
                geometry = torch.empty((n, screen.height, screen.width, 4), dtype=torch.float32, device="cuda:0") if k == 1 else None
                torch.cuda.synchronize()
                batch = arr if n > 1 else None
                # name -> (row, the form it is held against, soft shadows, launch)
                forms = {}
                forms["occlusion"] = ("a", None, False, lambda: gs.render_occlusion_batch(batch, ao=ao, stream=stream, colour=colour))
                forms["lit: reference light + term"] = ("a", "occlusion", False,
                                                       lambda: gs.render_lit_batch(batch, reference, ao=ao, stream=stream, colour=colour))
                if k == 1:
                    forms["geometry"] = ("b", None, False, lambda: gs.render_geometry_batch(batch, stream=stream, colour=colour, geometry=geometry))
                    plain = "geometry"
                else:
                    forms["supersampled"] = ("b", None, False, (lambda: gs.render_async(colour[0], stream=stream)) if n == 1 else
                                             (lambda: gs.render_batch_async(outs, arr, stream=stream)))
                    plain = "supersampled"
                forms["lit: reference light"] = ("b", plain, False, lambda: gs.render_lit_batch(batch, reference, stream=stream, colour=colour))
                forms["lit: light A + highlight + term"] = ("c", "lit: reference light + term", False,
                                                           lambda: gs.render_lit_batch(batch, light_a, ao=ao, stream=stream, colour=colour))
                forms["occlusion, shadows"] = ("c", None, True, lambda: gs.render_occlusion_batch(batch, ao=ao, stream=stream, colour=colour))
                forms["lit: reference light + term, shadows"] = ("c", "occlusion, shadows", True,
                                                                lambda: gs.render_lit_batch(batch, reference, ao=ao, stream=stream, colour=colour))
                forms["lit: light A + highlight + term, shadows"] = ("c", "lit: reference light + term, shadows", True,
                                                                    lambda: gs.render_lit_batch(batch, light_a, ao=ao, stream=stream, colour=colour))
                gs.set_supersampling(k)
                reps = {}
                for name, (_, _, shadowed, launch) in forms.items():  # warm up, then size the window
                    shadows(shadowed)
                    for _ in range(args.warmup):
                        launch()
                    ms = window(launch, stream, 5)
                    reps[name] = max(5, int(args.window_s * 1e3 / ms) + 1)
                seen = {name: [] for name in forms}
                for _ in range(args.windows):  # the forms take turns
                    for name, (_, _, shadowed, launch) in forms.items():
                        shadows(shadowed)
                        seen[name].append(window(launch, stream, reps[name]))
                shadows(False)
                gs.set_supersampling(1)
                for name, ms in seen.items():
                    row, against, shadowed, _ = forms[name]
                    med = statistics.median(ms)
                    rec = dict(workload=args.workload, width=screen.width, height=screen.height, k=k, frames_per_launch=n, row=row,
                               form=name, soft_shadows=shadowed, ms_per_launch=round(med, 4), spread_ms=round(max(ms) - min(ms), 4),
                               windows=len(ms), launches_per_window=reps[name], gpixel_per_s=round(px * n / (med * 1e-3) / 1e9, 3))
                    if against:
                        base = seen[against]
                        rec["against"] = against
                        rec["vs_against"] = round(med / statistics.median(base), 4)
                        if row == "a":
                            bound = statistics.median(base) + (max(base) - min(base))
                            rec["aim_bound_ms"] = round(bound, 4)
                            rec["aim_met"] = bool(med <= bound)
                    print(json.dumps(rec), flush=True)
                    lines.append(rec)
                del colour, geometry
    if args.out:
        Path(args.out).parent.mkdir(parents=True, exist_ok=True)
        with open(args.out, "a") as f:
            f.write("".join(json.dumps(r) + "\n" for r in lines))


if __name__ == "__main__":
    main()
