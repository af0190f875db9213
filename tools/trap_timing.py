#!/usr/bin/env python3
"""Orbit-trap colouring (kifs_render_trapped_async) against the lit call it extends, on one GPU.

All frames are the headline workload's (1080p Julia) with the test trap J -- a point trap at the origin of orbit space,
K = 8 orbit points, the range 0.3 .. 0.9 -- under light A with its highlight and the default term, in four shapes: a lone
frame and 48 orbit frames per launch (inline views), at k = 1 and 2, each without and with soft shadows.  Per shape
    trapped: trap J, light A + highlight + term     against     lit: light A + highlight + term
The lit side stands for the parent commit's kifs_render_lit_async: light::render_kernel's listing (make asm) is the
parent's instruction for instruction, so the two sides run in one process and take turns.  Every form is warmed up; then
the forms of a shape take turns, `--windows` times each, a turn being a synchronised window of launches at least
`--window-s` long between two device events.  Reported per form: the median window's ms per launch and the spread
(max - min over its windows).  The aim of a trapped row: no longer than the lit call's median, plus that call's own spread
in this run, plus the trap's share of the scene's orbit trips -- hits x K / inner_iters of the CPU restatement's work
counters (kor_render_stats) for the first frame at `--share-scale` of the resolution (the share is a ratio of counts per
pixel), written into the row.

    python tools/trap_timing.py --out profiles/trap_timing.jsonl
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
from kifs_raymarching_amd.configs import WORKLOADS, orbit_camera, trap_range  # noqa: E402

SHADOWS = dict(soft_shadow=True, shadow_steps=64, shadow_k=8.0, shadow_t0=0.02, shadow_max_t=10.0)
TRAP_K = 8


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


def orbit_share(w, scale):
    """hits x K / inner_iters of the workload's first frame at `scale` of its resolution, from the CPU restatement's
    counters: what the trap's orbit adds to the scene's own orbit trips."""
    import oracle as O
    ub = K.uniform_bytes
    screen = K.ScreenData(max(1, int(w.screen.width * scale)), max(1, int(w.screen.height * scale)))
    s = O.from_bytes(O.Screen, ub(screen.into_buffer_data()))
    c = O.from_bytes(O.Camera, ub(orbit_camera(w, 0).into_buffer_data()))
    o = O.from_bytes(O.Options, ub(w.gui.into_buffer_data()))
    _, _, st = O.render_stats(s, c, o, O.iters(*w.iters))
    return int(st.hits), int(st.inner_iters), int(st.hits) * TRAP_K / max(int(st.inner_iters), 1)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--workload", default="cfg2_julia_1080p")
    ap.add_argument("--frames", type=int, nargs="*", default=[1, 48], help="frames per launch (at most 64)")
    ap.add_argument("--factors", type=int, nargs="*", default=[1, 2], help="supersampling factors")
    ap.add_argument("--windows", type=int, default=5)
    ap.add_argument("--window-s", type=float, default=0.5)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--share-scale", type=float, default=1.0)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    w = WORKLOADS[args.workload]
    screen, px = w.screen, w.screen.width * w.screen.height
    ao = K.AmbientOcclusion()
    d = np.array([-0.55, 0.75, 0.36])
    light_a = K.Light(direction=tuple(float(v) for v in (d / np.linalg.norm(d)).astype(np.float32)), ambient=0.15, diffuse=0.85,
                      specular=(0.6, 0.6, 0.5), shininess_log2=3)
    scale, bias = trap_range(0.3, 0.9)
    trap = K.OrbitTrap(centre=(0.0, 0.0, 0.0, 0.0), axes=15, iterations=TRAP_K, scale=float(scale), bias=float(bias))
    hits, inner, share = orbit_share(w, args.share_scale)
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
                torch.cuda.synchronize()
                batch = arr if n > 1 else None
                # name -> (the form it is held against, soft shadows, launch)
                forms = {}
                for shadowed in (False, True):
                    tail = ", shadows" if shadowed else ""
                    forms["lit: light A + highlight + term" + tail] = (
                        None, shadowed, lambda: gs.render_lit_batch(batch, light_a, ao=ao, stream=stream, colour=colour))
                    forms["trapped: trap J, light A + highlight + term" + tail] = (
                        "lit: light A + highlight + term" + tail, shadowed,
                        lambda: gs.render_trapped_batch(batch, trap, light=light_a, ao=ao, stream=stream, colour=colour))
                gs.set_supersampling(k)
                reps = {}
                for name, (_, shadowed, launch) in forms.items():  # warm up, then size the window
                    shadows(shadowed)
                    for _ in range(args.warmup):
                        launch()
                    ms = window(launch, stream, 5)
                    reps[name] = max(5, int(args.window_s * 1e3 / ms) + 1)
                seen = {name: [] for name in forms}
                for _ in range(args.windows):  # the forms take turns
                    for name, (_, shadowed, launch) in forms.items():
                        shadows(shadowed)
                        seen[name].append(window(launch, stream, reps[name]))
                shadows(False)
                gs.set_supersampling(1)
                for name, ms in seen.items():
                    against, shadowed, _ = forms[name]
                    med = statistics.median(ms)
                    rec = dict(workload=args.workload, width=screen.width, height=screen.height, k=k, frames_per_launch=n, form=name,
                               soft_shadows=shadowed, ms_per_launch=round(med, 4), spread_ms=round(max(ms) - min(ms), 4), windows=len(ms),
                               launches_per_window=reps[name], gpixel_per_s=round(px * n / (med * 1e-3) / 1e9, 3))
                    if against:
                        base = seen[against]
                        rec["against"] = against
                        rec["vs_against"] = round(med / statistics.median(base), 4)
                        rec.update(trap_iterations=TRAP_K, share_scale=args.share_scale, hits=hits, inner_iters=inner, orbit_share=round(share, 6))
                        bound = statistics.median(base) * (1.0 + share) + (max(base) - min(base))
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
