#!/usr/bin/env python3
"""k x k supersampling (kifs_set_supersampling) against the frames it replaces, on one GPU: for each workload and k, the
lone frame and launches of 8 and 48 orbit frames, ms per launch from the library's device-event pairs
(kifs_set_profiling) after warm-up, and the virtual samples per second; for comparison the plain path rendering the
2W x 2H frame (what a caller would downsample, with the resolve in the wrong space) with the same batch sizes.

    python tools/ssaa_bench.py --out profiles/r06/ssaa_bench.jsonl
"""
import argparse
import json
import sys
from pathlib import Path

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))
import torch  # noqa: E402

import kifs_raymarching_amd as K  # noqa: E402
from kifs_raymarching_amd.configs import WORKLOADS, orbit_camera  # noqa: E402


def measure(w, screen, k, frames, warmup, reps):
    """Mean / min ms per launch of `frames` orbit frames (1 = a lone frame) at supersampling k."""
    cams = [orbit_camera(w, i) for i in range(frames)]
    with K.GraphicState(0, screen_data=screen, camera_data=cams[0], gui_data=w.gui) as gs:
        gs.set_iters(*w.iters)
        gs.set_supersampling(k)
        outs = [torch.empty((screen.height, screen.width, 4), dtype=torch.uint8, device="cuda:0") for _ in cams]
        torch.cuda.synchronize()
        stream = torch.cuda.Stream()

        def launch():
            if frames == 1:
                gs.render_async(outs[0], stream=stream)
            else:
                gs.render_batch_async(outs, cams, stream=stream)

        for _ in range(warmup):
            launch()
        stream.synchronize()
        gs.set_profiling(1)
        for _ in range(reps):
            launch()
        stream.synchronize()
        n, mean_ms, min_ms, _ = gs.profile_read()
        gs.set_profiling(0)
        kernel = gs.debug_last_kernel()
    assert n == reps, (n, reps)
    return mean_ms, min_ms, kernel


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--workloads", nargs="*", default=["cfg2_julia_1080p", "cfg3_sierpinski_1080p"])
    ap.add_argument("--ks", type=int, nargs="*", default=[1, 2, 3])
    ap.add_argument("--batches", type=int, nargs="*", default=[1, 8, 48])
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    lines = []
    for name in args.workloads:
        w = WORKLOADS[name]
        for b in args.batches:
            rows = [("ssaa", k, w.screen) for k in args.ks]
            rows.append(("plain_2x_frame", 1, K.ScreenData(2 * w.screen.width, 2 * w.screen.height)))
            for form, k, screen in rows:
                mean_ms, min_ms, kernel = measure(w, screen, k, b, args.warmup, args.reps)
                samples = k * k * screen.width * screen.height * b
                rec = dict(workload=name, form=form, k=k, frames_per_launch=b, width=screen.width, height=screen.height,
                           ms_per_launch=round(mean_ms, 4), min_ms=round(min_ms, 4), kernel=kernel,
                           virtual_gsamples_per_s=round(samples / (mean_ms * 1e-3) / 1e9, 3),
                           output_gpixel_per_s=round(w.screen.width * w.screen.height * b / (mean_ms * 1e-3) / 1e9, 3))
                print(json.dumps(rec), flush=True)
                lines.append(rec)
    if args.out:
        Path(args.out).parent.mkdir(parents=True, exist_ok=True)
        Path(args.out).write_text("".join(json.dumps(r) + "\n" for r in lines))


if __name__ == "__main__":
    main()
