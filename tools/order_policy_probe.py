#!/usr/bin/env python3
"""GPU box: which tile order serves a batch whose views move?  The headline's call pattern (48 orbit poses per launch, five
pose sets in turn) under PINNED orders (debug_set_tile_order: no feedback), three alternating rounds of 30 launches each:
`centre` (the static centre-first order), `spread` (the feedback's order for ONE batch of 48 poses spread over the whole
orbit), `union` (every tile at its best rank in any of the five pose sets' own orders) and `own` (every launch under the
order measured on its own pose set: the ceiling of a shared order).  Prints one JSON line: mean kernel ms by order and pose set.
    python tools/order_policy_probe.py"""
import json
import sys
from pathlib import Path

import numpy as np
import torch

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))
import kifs_raymarching_amd as K  # noqa: E402
from kifs_raymarching_amd.configs import WORKLOADS, orbit_camera  # noqa: E402

w = WORKLOADS["cfg2_julia_1080p"]
W, H, B = w.screen.width, w.screen.height, 48
poses = [orbit_camera(w, i).into_buffer_data() for i in range(120)]
bufs = [torch.zeros((B * H, W, 4), dtype=torch.uint8, device="cuda:0") for _ in range(2)]
st = torch.cuda.Stream()


def ctx():
    g = K.GraphicState(0, screen_data=w.screen, camera_data=w.camera, gui_data=w.gui)
    g.set_iters(*w.iters)
    return g


def go(g, cams, j):
    out = bufs[j % 2]
    g.render_batch_async([out[i * H:(i + 1) * H] for i in range(B)], cams, stream=st)


def order_of(idx, launches=8):
    """The feedback's order for the pose list idx, rendered `launches` times by a fresh context."""
    g = ctx()
    cams = K.camera_array([poses[i % 120] for i in idx])
    for j in range(launches):
        go(g, cams, j)
    st.synchronize()
    o = g.debug_get_tile_order()
    g.close()
    return o


g0 = ctx()
go(g0, K.camera_array(poses[:B]), 0)
st.synchronize()
centre = g0.debug_get_tile_order()
g0.close()
spread = order_of([int(round(2.5 * i)) for i in range(B)])
own = {s: order_of(range(s, s + B)) for s in (0, 24, 48, 72, 96)}
# union: a position's rank = its best (smallest) rank in any pose set's own order
n = len(centre)
tx = (W + 31) // 32
best = np.full(n, n, dtype=np.int64)
for o in own.values():
    idx = (o & 0xffff).astype(np.int64) + (o >> 16).astype(np.int64) * tx
    best[idx] = np.minimum(best[idx], np.arange(n))
u = np.argsort(best, kind="stable")
union = ((u % tx) | ((u // tx) << 16)).astype(np.uint32)

g = ctx()
arrays = {s: K.camera_array([poses[(s + i) % 120] for i in range(B)]) for s in (0, 24, 48, 72, 96)}
for j in range(60):
    go(g, arrays[(j * B) % 120], j)
st.synchronize()
g.set_profiling(1)
g.profile_read()
res = {}
j = 60
for rnd in range(3):
    for name in ("centre", "spread", "union", "own"):
        if name != "own":
            g.debug_set_tile_order({"centre": centre, "spread": spread, "union": union}[name])
        for _ in range(30):
            s = (j * B) % 120
            if name == "own":
                g.debug_set_tile_order(own[s])
            go(g, arrays[s], j)
            st.synchronize()
            res.setdefault(name, {}).setdefault(s, []).append(g.profile_read()[1])
            j += 1
out = {name: {"mean": round(float(np.mean([x for v in d.values() for x in v])), 4),
              "by_pose_set": {str(s): round(float(np.mean(v)), 4) for s, v in sorted(d.items())},
              "min": round(float(min(x for v in d.values() for x in v)), 4), "max": round(float(max(x for v in d.values() for x in v)), 4)}
       for name, d in res.items()}
print(json.dumps(out))
