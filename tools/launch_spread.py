#!/usr/bin/env python3
"""GPU box: where does the launch-to-launch spread of a batched launch's kernel time come from?  The headline's call pattern
(bench.py: launch j renders poses 48 j .. 48 j + 47 of the 120-pose orbit, so five pose sets take turns), every launch timed
by the library's own event pair, one row per launch: kernel time, pose set (first pose % 120), place k in the tile order's
feedback period and the age of the order in launches.  Then the means by pose set and by k, and the spread that is left
within a pose set.  The period comes from the environment (KIFS_TUNING=1 KIFS_BATCH_PERIOD=n, KIFS_TILE_FEEDBACK=0);
--frozen pins the order the settle launches arrived at (no feedback afterwards).
    python tools/launch_spread.py [--workload W] [--frames B] [--launches N] [--settle N] [--period P] [--frozen] [--rows]
--period only labels the rows (k = launch % P, age): it must be the period the library runs with (default 3)."""
import argparse
import json
import os
import sys
from pathlib import Path

import numpy as np
import torch

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))
import kifs_raymarching_amd as K  # noqa: E402
from kifs_raymarching_amd.configs import HEADLINE, WORKLOADS, orbit_camera  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--workload", default=HEADLINE)
ap.add_argument("--frames", type=int, default=48)
ap.add_argument("--launches", type=int, default=120)
ap.add_argument("--settle", type=int, default=60)
ap.add_argument("--period", type=int, default=0, help="0: KIFS_BATCH_PERIOD under KIFS_TUNING=1, else 3")
ap.add_argument("--frozen", action="store_true")
ap.add_argument("--path", default="orbit", choices=["orbit", "spiral", "slow"],
                help="orbit: the benchmark's 120-pose loop; spiral: 3 degrees a frame like the orbit, with elevation and distance "
                     "drifting so that no view comes back; slow: 0.03 degrees a frame")
ap.add_argument("--scene-change", type=int, default=0, metavar="N",
                help="every N launches the Julia constant changes (two scenes in turn): update_options between launches")
ap.add_argument("--rows", action="store_true", help="print the row of every launch as well")
ap.add_argument("--label", default="")
args = ap.parse_args()

tuning = os.environ.get("KIFS_TUNING") == "1"
period = args.period or (int(os.environ.get("KIFS_BATCH_PERIOD", "3")) if tuning else 3)
feedback = not (tuning and os.environ.get("KIFS_TILE_FEEDBACK") == "0") and not args.frozen
w = WORKLOADS[args.workload]
W, H, B = w.screen.width, w.screen.height, args.frames
gs = K.GraphicState(0, screen_data=w.screen, camera_data=w.camera, gui_data=w.gui)
gs.set_iters(*w.iters)
if w.extensions:
    gs.set_extensions(**w.extensions)
bufs = [torch.zeros((B * H, W, 4), dtype=torch.uint8, device="cuda:0") for _ in range(2)]
torch.cuda.synchronize()
st = torch.cuda.Stream()
n_poses = max(w.frames, 120)
poses = [orbit_camera(w, i).into_buffer_data() for i in range(n_poses)]
arrays = {}
total = (args.settle + args.launches) * B


def pose(k):
    """Frame k of a path on which no view comes back."""
    base, u = w.camera, k / total
    if args.path == "slow":
        return K.CameraData(origin_distance=base.origin_distance, min_distance=base.min_distance, phi=2.0 * np.pi * k / 12000.0,
                            theta=base.theta).into_buffer_data()
    return K.CameraData(origin_distance=base.origin_distance * (0.8 + 0.5 * u), min_distance=base.min_distance,
                        phi=2.0 * np.pi * k / 120.0, theta=-0.9 + 1.8 * u).into_buffer_data()


other_gui = None
if args.scene_change:
    import dataclasses
    c = list(w.gui.constant)
    other_gui = dataclasses.replace(w.gui, constant=(c[0] + 0.15, c[1] - 0.1, c[2], c[3]))


def launch(j):
    if other_gui is not None and j % args.scene_change == 0:
        gs.update_options(other_gui if (j // args.scene_change) % 2 else w.gui)
    first = (j * B) % n_poses
    if args.path != "orbit":
        cams = K.camera_array([pose(j * B + i) for i in range(B)])
    else:
        if first not in arrays:
            arrays[first] = K.camera_array([poses[(first + i) % n_poses] for i in range(B)])
        cams = arrays[first]
    out = bufs[j % 2]
    gs.render_batch_async([out[i * H:(i + 1) * H] for i in range(B)], cams, stream=st)
    return first


for j in range(args.settle):
    launch(j)
    if j % 8 == 7:
        st.synchronize()
st.synchronize()
if args.frozen:
    gs.debug_set_tile_order(gs.debug_get_tile_order())
gs.set_profiling(1)
gs.profile_read()
rows = []
for j in range(args.settle, args.settle + args.launches):
    first = launch(j)
    st.synchronize()
    n, ms, _, _ = gs.profile_read()
    assert n == 1
    k = j % period  # (every launch since the context's first is a feedback launch of this table)
    rows.append((j, first, k if feedback else -1, ((k - 1) % period + 1) if feedback else -1, ms))

ms = np.array([r[4] for r in rows])
sets = sorted({r[1] for r in rows})
by_set = {s: ms[[r[1] == s for r in rows]] for s in sets}
by_k = {k: ms[[r[2] == k for r in rows]] for k in sorted({r[2] for r in rows})}
within = np.concatenate([v / v.mean() for v in by_set.values()])  # each launch over its pose set's mean
summary = {
    "label": args.label, "workload": args.workload, "frames": B, "kernel": gs.debug_last_kernel(), "launches": len(rows),
    "period": period if feedback else None, "feedback": "frozen after the settle" if args.frozen else ("on" if feedback else "off"),
    "ms": {"mean": round(float(ms.mean()), 4), "min": round(float(ms.min()), 4), "max": round(float(ms.max()), 4),
           "median": round(float(np.median(ms)), 4)},
    "by_pose_set": {str(s): {"n": len(v), "mean": round(float(v.mean()), 4), "min": round(float(v.min()), 4), "max": round(float(v.max()), 4)}
                    for s, v in by_set.items()},
    "by_k": {str(k): {"n": len(v), "mean": round(float(v.mean()), 4), "min": round(float(v.min()), 4), "max": round(float(v.max()), 4)}
             for k, v in by_k.items()},
    "by_k_over_pose_set_mean": {str(k): round(float(np.mean([r[4] / by_set[r[1]].mean() for r in rows if r[2] == k])), 4) for k in by_k},
    "pose_set_means_over_mean": [round(float(v.mean() / ms.mean()), 4) for v in by_set.values()],
    "within_pose_set": {"min": round(float(within.min()), 4), "max": round(float(within.max()), 4), "std": round(float(within.std()), 4)},
}
if args.rows:
    print("launch pose_set k age kernel_ms")
    for r in rows:
        print(f"{r[0]:6d} {r[1]:8d} {r[2]:1d} {r[3]:3d} {r[4]:.4f}")
print(json.dumps(summary))
