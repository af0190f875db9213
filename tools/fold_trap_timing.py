#!/usr/bin/env python3
"""Orbit-trap colouring of folded scenes (kifs_render_folded_trapped_async) against the folded call it extends, on one GPU.

All frames are 1080p with the Sierpinski workload's cameras (cfg3_sierpinski_1080p), light A with its highlight and the
default term.  Two systems -- the Menger preset (the box through ABS|SORT|MIRROR_Z, N = 4, s = 3) with a plane trap, and
TETRA, N = 10, s = 2, c = (1,1,1) on the sphere with a point trap, K = N each -- in four shapes: a lone frame and 48 orbit
frames per launch, at k = 1 and 2; each without and with soft shadows; and one row more with the plane of u (k = 1, a lone
frame, no shadows).  Every row holds the trapped form against kifs_render_folded_async with the same system, light and
term on the same context: fold::render_kernel's listing (make asm) is the parent commit's instruction for instruction, so
this tree's folded call stands for the parent's and the two sides run in one process and take turns.

Aim per row: the folded call's median x (1 + r), plus that call's own spread in the run.  r is the share of the launch's
fold rounds that the trap evaluations add, counted on the CPU model (`--count-share`, which needs no GPU): per pixel the
march's estimates from the heatmap counter, six for a hit's normal and the term's probes, N rounds each, against min(N, K)
rounds for a hit's orbit.  Soft-shadow steps are not counted, so the r of a row with shadows is an upper bound.  The
lone-frame rows also carry the record's 128-byte copy, which the folded call does not have.

Every form is warmed up; then the forms of a shape take turns, `--windows` times each, a turn being a synchronised window
of launches at least `--window-s` long between two device events.  Reported per form: the median window's ms per launch
and the spread (max - min over its windows).

    python tools/fold_trap_timing.py --count-share                     # r per system, on the CPU
    python tools/fold_trap_timing.py --out profiles/fold_trap_timing.jsonl
"""
import argparse
import json
import statistics
import sys
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))

import kifs_raymarching_amd as K  # noqa: E402
from kifs_raymarching_amd.configs import FOLD_PRESETS, WORKLOADS, orbit_camera  # noqa: E402

FOLDS = 10
# r per system as `--count-share` gave it at 240 x 135 (camera 0 of the orbit, one ray per pixel, the default term)
SHARE = {"menger": 0.002731, "tetra": 0.001365}
SHADOWS = dict(soft_shadow=True, shadow_steps=64, shadow_k=8.0, shadow_t0=0.02, shadow_max_t=10.0)


def systems(w):
    """name -> (options, fold system, trap): the two rows' scenes."""
    base, menger = FOLD_PRESETS["menger"]
    box = K.GuiData(**{**w.gui.__dict__, "primitive_shape": base})
    sphere = K.GuiData(**{**w.gui.__dict__, "primitive_shape": K.PrimitiveShape.Sphere})
    tetra = K.FoldSystem(stages=("tetra",), iterations=FOLDS, scale=2.0, offset=(1.0, 1.0, 1.0))
    return {"menger": (box, menger, K.OrbitTrap(centre=(0.0, 0.0, 0.0, 0.0), axes=4, iterations=menger.iterations, scale=1.0, bias=0.0)),
            "tetra": (sphere, tetra, K.OrbitTrap(centre=(0.0, 0.0, 0.0, 0.0), axes=15, iterations=FOLDS, scale=0.5, bias=0.0))}


def count_share(w, width, height):
    """r per system on the CPU model (tests/fold_trap_reference.c through its loader): the fold rounds of the trap
    evaluations over those of the launch's estimates."""
    sys.path.insert(0, str(ROOT / "tests"))
    sys.path.insert(0, str(ROOT))
    import fold_trap_reference as FT
    import oracle as O
    from helpers import oracle_uniforms
    screen = K.ScreenData(width, height)
    cam = orbit_camera(w, 0)
    term = K.AmbientOcclusion()
    out = {}
    for name, (gui, fold, trap) in systems(w).items():
        heat = K.GuiData(**{**gui.__dict__, "is_heatmap": True, "fractal_color": (255, 255, 255)})
        s, c, o = oracle_uniforms(O, K, (screen, cam, heat))
        f, t = fold.into_buffer_data(), trap.into_buffer_data()
        spec = dict(stages=f.stages, iterations=f.iterations, scale=f.scale, offset=tuple(f.offset), rotation=tuple(f.rotation))
        tr = dict(centre=tuple(t.centre), axes=t.axes, iterations=t.iterations, scale=t.scale, bias=t.bias, mid=tuple(t.mid), far=tuple(t.far))
        m = FT.march(O, s, c, o, O.iters(*w.iters), spec, tr)
        steps = np.rint(m.rgb[..., 0].astype(np.float64) * o.max_iterations)  # the counter: estimates that did not hit
        hits = int(m.hit.sum())
        estimates = float(steps.sum()) + hits * (1 + 6 + term.samples)  # the hit's own, its normal's six, the probes
        n, k = f.iterations, min(f.iterations, t.iterations)
        out[name] = dict(width=width, height=height, hits=hits, estimates=int(estimates), rounds_per_estimate=n, trap_rounds_per_hit=k,
                         share=round(hits * k / (estimates * n), 6))
    return out


def window(torch, launch, stream, reps):
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
    ap.add_argument("--window-s", type=float, default=0.25)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--count-share", action="store_true", help="count r per system on the CPU model and exit")
    ap.add_argument("--share-size", type=int, nargs=2, default=[240, 135])
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    w = WORKLOADS[args.workload]
    if args.count_share:
        for name, rec in count_share(w, *args.share_size).items():
            print(json.dumps(dict(system=name, **rec)))
        return
    import torch
    screen, px = w.screen, w.screen.width * w.screen.height
    ao = K.AmbientOcclusion()
    d = np.array([-0.55, 0.75, 0.36])
    light_a = K.Light(direction=tuple(float(v) for v in (d / np.linalg.norm(d)).astype(np.float32)), ambient=0.15, diffuse=0.85,
                      specular=(0.6, 0.6, 0.5), shininess_log2=3)
    lines = []
    cam0 = orbit_camera(w, 0)
    stream = torch.cuda.Stream()
    for name, (gui, fold, trap) in systems(w).items():
        with K.GraphicState(0, screen_data=screen, camera_data=cam0, gui_data=gui) as g:
            g.set_iters(*w.iters)
            for k in args.factors:
                for n in args.frames:
                    cams = [orbit_camera(w, i) for i in range(n)]
                    batch = K.camera_array(cams) if n > 1 else None
                    colour = torch.empty((n, screen.height, screen.width, 4), dtype=torch.uint8, device="cuda:0")
                    plane = torch.empty((n, screen.height, screen.width), dtype=torch.float32, device="cuda:0") if (k == 1 and n == 1) else None
                    torch.cuda.synchronize()
                    for shadows in (False, True):
                        g.set_extensions(**SHADOWS) if shadows else g.set_extensions(soft_shadow=False)
                        g.set_supersampling(k)
                        forms = {"folded": lambda: g.render_folded_batch(batch, fold, light=light_a, ao=ao, stream=stream, colour=colour),
                                 "folded trapped": lambda: g.render_folded_trapped_batch(batch, fold, trap, light=light_a, ao=ao, stream=stream,
                                                                                         colour=colour)}
                        if plane is not None and not shadows:
                            forms["folded trapped, with the plane"] = lambda: g.render_folded_trapped_batch(
                                batch, fold, trap, light=light_a, ao=ao, u_plane=plane, stream=stream, colour=colour)
                        reps = {}
                        for form, launch in forms.items():  # warm up, then size the window
                            for _ in range(args.warmup):
                                launch()
                            ms = window(torch, launch, stream, 5)
                            reps[form] = max(5, int(args.window_s * 1e3 / ms) + 1)
                        seen = {form: [] for form in forms}
                        for _ in range(args.windows):  # the forms take turns
                            for form, launch in forms.items():
                                seen[form].append(window(torch, launch, stream, reps[form]))
                        g.set_supersampling(1)
                        g.set_extensions(soft_shadow=False)
                        base = seen["folded"]
                        for form, ms in seen.items():
                            med = statistics.median(ms)
                            rec = dict(workload=args.workload, system=name, width=screen.width, height=screen.height, k=k, frames_per_launch=n,
                                       soft_shadows=shadows, form=form, ms_per_launch=round(med, 4), spread_ms=round(max(ms) - min(ms), 4),
                                       windows=len(ms), launches_per_window=reps[form], gpixel_per_s=round(px * n / (med * 1e-3) / 1e9, 3))
                            if form != "folded":
                                bound = statistics.median(base) * (1.0 + SHARE[name]) + (max(base) - min(base))
                                rec.update(against="folded", vs_against=round(med / statistics.median(base), 4), share=SHARE[name],
                                           share_is_upper_bound=shadows, aim_bound_ms=round(bound, 4), aim_met=bool(med <= bound),
                                           over_aim_ms=round(max(med - bound, 0.0), 4))
                            print(json.dumps(rec), flush=True)
                            lines.append(rec)
                    del colour, plane
    if args.out:
        Path(args.out).parent.mkdir(parents=True, exist_ok=True)
        with open(args.out, "a") as f:
            f.write("".join(json.dumps(r) + "\n" for r in lines))


if __name__ == "__main__":
    main()
