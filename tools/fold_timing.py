#!/usr/bin/env python3
"""Kaleidoscopic IFS scenes (kifs_render_folded_async) against the lit call they extend, on one GPU.

All frames are 1080p with the Sierpinski workload's cameras (cfg3_sierpinski_1080p), light A with its highlight and the
default term, in four shapes: a lone frame and 48 orbit frames per launch (inline views), at k = 1 and 2.  Two rows per
shape, each a folded form held against a lit form:
    1. the cost of the door   folded, N = 0, on the Sierpinski pipeline          against   lit, the same context
       The fold loop is a scalar branch that is never entered; the folded launch runs with every cull off, which counts
       against this row (there is no tuning override that zeroes the lit call's culls, so the two are not separated).
       Aim: no longer than the lit call's median plus that call's own spread in the run.
    2. the fold itself        folded, TETRA, N = 10, s = 2, c = (1,1,1), sphere   against   lit, Sierpinski with fold_iters = 10
       Both make the same ten folds per estimate and the surfaces are 2^-10 apart; the lit side's loop is the
       hand-scheduled one (20 instructions per fold), the folded side's the compiler's.
       Aim: at most 27 / 20 of the lit call's median plus its spread.
The lit side stands for the parent commit's kifs_render_lit_async: light::render_kernel's listing (make asm) is the
parent's instruction for instruction, so the sides run in one process and take turns.  Every form is warmed up; then the
forms of a shape take turns, `--windows` times each, a turn being a synchronised window of launches at least `--window-s`
long between two device events.  Reported per form: the median window's ms per launch and the spread (max - min over its
windows).

    python tools/fold_timing.py --out profiles/fold_timing.jsonl
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

FOLDS = 10


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
    ap.add_argument("--workload", default="cfg3_sierpinski_1080p")
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
    d = np.array([-0.55, 0.75, 0.36])
    light_a = K.Light(direction=tuple(float(v) for v in (d / np.linalg.norm(d)).astype(np.float32)), ambient=0.15, diffuse=0.85,
                      specular=(0.6, 0.6, 0.5), shininess_log2=3)
    door = K.FoldSystem()  # N = 0
    tetra = K.FoldSystem(stages=("tetra",), iterations=FOLDS, scale=2.0, offset=(1.0, 1.0, 1.0))
    sphere = K.GuiData(**{**w.gui.__dict__, "primitive_shape": K.PrimitiveShape.Sphere})
    lines = []
    cam0 = orbit_camera(w, 0)
    with K.GraphicState(0, screen_data=screen, camera_data=cam0, gui_data=w.gui) as as_is, \
            K.GraphicState(0, screen_data=screen, camera_data=cam0, gui_data=w.gui) as ten, \
            K.GraphicState(0, screen_data=screen, camera_data=cam0, gui_data=sphere) as ball:
        as_is.set_iters(*w.iters)
        ten.set_iters(w.iters[0], w.iters[1], FOLDS)
        ball.set_iters(*w.iters)
        stream = torch.cuda.Stream()
        for k in args.factors:
            for n in args.frames:
                cams = [orbit_camera(w, i) for i in range(n)]
                arr = K.camera_array(cams)
                colour = torch.empty((n, screen.height, screen.width, 4), dtype=torch.uint8, device="cuda:0")
                torch.cuda.synchronize()
                batch = arr if n > 1 else None
                # name -> (the form it is held against, the factor on that form's median, launch)
                forms = {
                    "lit: Sierpinski as the workload has it": (
                        None, 1.0, lambda: as_is.render_lit_batch(batch, light_a, ao=ao, stream=stream, colour=colour)),
                    "folded: N = 0 on the Sierpinski pipeline (the door)": (
                        "lit: Sierpinski as the workload has it", 1.0,
                        lambda: as_is.render_folded_batch(batch, door, light=light_a, ao=ao, stream=stream, colour=colour)),
                    f"lit: Sierpinski with fold_iters = {FOLDS}": (
                        None, 1.0, lambda: ten.render_lit_batch(batch, light_a, ao=ao, stream=stream, colour=colour)),
                    f"folded: TETRA, N = {FOLDS}, s = 2, c = (1,1,1) on the sphere (the fold)": (
                        f"lit: Sierpinski with fold_iters = {FOLDS}", 27.0 / 20.0,
                        lambda: ball.render_folded_batch(batch, tetra, light=light_a, ao=ao, stream=stream, colour=colour)),
                }
                for g in (as_is, ten, ball):
                    g.set_supersampling(k)
                reps = {}
                for name, (_, _, launch) in forms.items():  # warm up, then size the window
                    for _ in range(args.warmup):
                        launch()
                    ms = window(launch, stream, 5)
                    reps[name] = max(5, int(args.window_s * 1e3 / ms) + 1)
                seen = {name: [] for name in forms}
                for _ in range(args.windows):  # the forms take turns
                    for name, (_, _, launch) in forms.items():
                        seen[name].append(window(launch, stream, reps[name]))
                for g in (as_is, ten, ball):
                    g.set_supersampling(1)
                for name, ms in seen.items():
                    against, factor, _ = forms[name]
                    med = statistics.median(ms)
                    rec = dict(workload=args.workload, width=screen.width, height=screen.height, k=k, frames_per_launch=n, form=name,
                               ms_per_launch=round(med, 4), spread_ms=round(max(ms) - min(ms), 4), windows=len(ms),
                               launches_per_window=reps[name], gpixel_per_s=round(px * n / (med * 1e-3) / 1e9, 3))
                    if against:
                        base = seen[against]
                        rec["against"] = against
                        rec["vs_against"] = round(med / statistics.median(base), 4)
                        bound = statistics.median(base) * factor + (max(base) - min(base))
                        rec["aim_factor"] = round(factor, 4)
                        rec["aim_bound_ms"] = round(bound, 4)
                        rec["aim_met"] = bool(med <= bound)
                        rec["over_aim_ms"] = round(max(med - bound, 0.0), 4)
                    print(json.dumps(rec), flush=True)
                    lines.append(rec)
                del colour
    if args.out:
        Path(args.out).parent.mkdir(parents=True, exist_ok=True)
        with open(args.out, "a") as f:
            f.write("".join(json.dumps(r) + "\n" for r in lines))


if __name__ == "__main__":
    main()
