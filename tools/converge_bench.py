#!/usr/bin/env python3
"""Converging accumulation (kifs_render_accumulate_converge_async) on one GPU and in one process: what the rule costs a
pass in which nothing settles, and what it buys a frame in which most pixels do.

price    for each (count, samples) -- default (1, 16), (6, 8), (48, 4) of cfg2_julia_1080p, the motion-blur cameras and
         cells of tools/progressive_bench.py at --grid 4 -- a resume pass with prior 16 and a picture (which a checkout
         without the new call has too: --tree DIR is the A/B against the parent commit) and, where the tree has it, a
         converging pass over planes earlier passes left, with min_samples above every total: every pixel is marched, and
         the pass moves 8 bytes per pixel and frame more for the moments plane, plus the mask's reads; and the same pass
         without the counts, without a picture and as a restart (neither plane read), which say where a difference sits.
buys     a lens frame (configs.lens_cameras, aperture 0.05, focus 3.2) taken to 256 rays per pixel as 16 passes of 16
         with no rule (resume passes) and, where the tree has the call, with tolerances 1/64 and 1/256 (min_samples 16):
         the total ms, and per pass the ms, the active count after it and -- from the planes -- the share of the pixels
         it marched that sat in partly active 8 x 8 blocks, which lane masking cannot speed up.

Before any timing the bytes are compared: a restart pass against the jittered call (identity (a)), and two passes with
min_samples above the total against the same two resume passes, picture and sums plane (identity (b)).  Every figure is
timed with a pair of device events around the call on one stream after --warmup launches.

    python tools/converge_bench.py --out profiles/r14/converge_bench.jsonl
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
ap.add_argument("--prior", type=int, default=16, help="sub-frames in the planes of the timed passes")
ap.add_argument("--shutter", type=float, default=0.5)
ap.add_argument("--tolerances", default="0.015625,0.00390625", help="of the lens frame, comma separated")
ap.add_argument("--passes", type=int, default=16)
ap.add_argument("--per-pass", type=int, default=16)
ap.add_argument("--warmup", type=int, default=5)
ap.add_argument("--reps", type=int, default=20)
ap.add_argument("--only", default=None, choices=["price", "buys"], help="one of the two parts")
ap.add_argument("--out", default=None)
args = ap.parse_args()
sys.path.insert(0, args.tree)
import torch  # noqa: E402

import kifs_raymarching_amd as K  # noqa: E402
from kifs_raymarching_amd import configs  # noqa: E402
from kifs_raymarching_amd.configs import WORKLOADS, lens_cameras, shutter_cameras  # noqa: E402

HAS_CONVERGE = hasattr(K.GraphicState, "render_accumulate_converge")
NEVER = 1 << 24  # min_samples above every total: nothing settles


def timed(stream, fn, reps=None, warmup=None):
    """(mean, min) ms of fn() on `stream` between two device events."""
    for _ in range(args.warmup if warmup is None else warmup):
        fn()
    stream.synchronize()
    ms = []
    for _ in range(args.reps if reps is None else reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record(stream)
        fn()
        b.record(stream)
        stream.synchronize()
        ms.append(a.elapsed_time(b))
    return round(sum(ms) / len(ms), 4), round(min(ms), 4)


def emit(rec):
    rec = dict(label=args.label, converge_call=HAS_CONVERGE, workload=args.workload, warmup=args.warmup, reps=args.reps, **rec)
    print(json.dumps(rec), flush=True)
    if args.out:
        Path(args.out).parent.mkdir(parents=True, exist_ok=True)
        with open(args.out, "a") as f:
            f.write(json.dumps(rec) + "\n")


def price(gs, w, stream):
    width, height, g = w.screen.width, w.screen.height, args.grid
    for shape in filter(None, args.rows.split(",")):
        count, samples = (int(v) for v in shape.split("x"))
        views = [c.into_buffer_data() for f in range(count) for c in shutter_cameras(w, f, samples, args.shutter)]
        cams = K.camera_array(views)
        pairs = [c for f in range(count) for c in configs.jitter_cells(g, samples, f)]
        cells = (K._lib.KifsSubpixel * len(pairs))(*[K._lib.KifsSubpixel(i, j) for i, j in pairs])
        one = torch.zeros((count, height, width, 4), dtype=torch.uint8, device="cuda:0")
        out = torch.zeros_like(one)
        sums = torch.full((count, height, width, 4), float("nan"), dtype=torch.float32, device="cuda:0")
        torch.cuda.synchronize()
        rec = dict(kind="price", count=count, samples=samples, grid=g, prior=args.prior, extra_bytes=8 * width * height * count,
                   mask_read_bytes=3 * 20 * width * height * count)
        gs.render_accumulate(cams, samples, outs=one, stream=stream, jitter=(g, cells))
        gs.render_accumulate_resume(sums, 0, cams, samples, picture=False, stream=stream, jitter=(g, cells))
        stream.synchronize()
        if HAS_CONVERGE:
            csums = torch.full_like(sums, float("nan"))
            moments = torch.full((count, height, width), float("nan"), dtype=torch.float32, device="cuda:0")
            counts = torch.zeros((count,), dtype=torch.int32, device="cuda:0")
            torch.cuda.synchronize()
            # identity (a): a restart pass over planes of NaNs is the jittered call; its sums are the resume call's
            gs.render_accumulate_converge(csums, moments, cams, samples, (1.0 / 64, NEVER), restart=True, counts=counts, outs=out,
                                          stream=stream, jitter=(g, cells))
            stream.synchronize()
            if not bool((out == one).all()) or not bool((csums.view(torch.int32) == sums.view(torch.int32)).all()):
                raise SystemExit("converge_bench: a restart pass differs from the jittered call or the resume call's plane")
            if counts.cpu().tolist() != [width * height] * count:
                raise SystemExit("converge_bench: a pass below min_samples must leave every pixel active")
            # identity (b): a second pass of each kind over the same views
            gs.render_accumulate_resume(sums, samples, cams, samples, outs=one, stream=stream, jitter=(g, cells))
            gs.render_accumulate_converge(csums, moments, cams, samples, (1.0 / 64, NEVER), counts=counts, outs=out, stream=stream,
                                          jitter=(g, cells))
            stream.synchronize()
            if not bool((out == one).all()) or not bool((csums.view(torch.int32) == sums.view(torch.int32)).all()):
                raise SystemExit("converge_bench: a second pass differs from the resume call")
            rec["identities_hold"] = True
            # the timed pass: nothing settles, so every launch marches every pixel (n grows from launch to launch, which
            # changes nothing the pass does)
            rec["converge_ms"], rec["converge_min_ms"] = timed(
                stream, lambda: gs.render_accumulate_converge(csums, moments, cams, samples, (1.0 / 64, NEVER), counts=counts, outs=out,
                                                              stream=stream, jitter=(g, cells)))
            # what the other forms of the same pass say about it: without the counts (no atomic), without a picture, and
            # as a restart (neither plane is read: no mask loads, no texel loads)
            rec["converge_nocounts_ms"], rec["converge_nocounts_min_ms"] = timed(
                stream, lambda: gs.render_accumulate_converge(csums, moments, cams, samples, (1.0 / 64, NEVER), outs=out, stream=stream,
                                                              jitter=(g, cells)))
            rec["converge_silent_ms"], rec["converge_silent_min_ms"] = timed(
                stream, lambda: gs.render_accumulate_converge(csums, moments, cams, samples, (1.0 / 64, NEVER), counts=counts,
                                                              picture=False, stream=stream, jitter=(g, cells)))
            rec["converge_restart_ms"], rec["converge_restart_min_ms"] = timed(
                stream, lambda: gs.render_accumulate_converge(csums, moments, cams, samples, (1.0 / 64, NEVER), restart=True, counts=counts,
                                                              outs=out, stream=stream, jitter=(g, cells)))
            del csums, moments
        rec["resume_ms"], rec["resume_min_ms"] = timed(
            stream, lambda: gs.render_accumulate_resume(sums, args.prior, cams, samples, outs=one, stream=stream, jitter=(g, cells)))
        if HAS_CONVERGE:
            rec["converge_over_resume"] = round(rec["converge_ms"] / rec["resume_ms"], 4)
        emit(rec)
        del one, out, sums


def partly_active_share(mask):
    """Of a (H, W) bool mask on the device: the share of its set pixels that sit in 8 x 8 blocks that are not all set."""
    h, w = mask.shape
    pad = torch.zeros(((h + 7) // 8 * 8, (w + 7) // 8 * 8), dtype=torch.bool, device=mask.device)
    inside = torch.zeros_like(pad)
    pad[:h, :w] = mask
    inside[:h, :w] = True
    blocks = lambda t: t.view(pad.shape[0] // 8, 8, pad.shape[1] // 8, 8).sum(dim=(1, 3))
    on, size = blocks(pad), blocks(inside)
    total = int(on.sum())
    return round(float(on[on < size].sum()) / total, 4) if total else 0.0


def buys(gs, w, stream):
    width, height, g = w.screen.width, w.screen.height, args.grid
    n, per = args.passes, args.per_pass
    views = lens_cameras(w.camera, 0.05, 3.2, n * per)
    passes = []
    for p in range(n):
        pairs = configs.jitter_cells(g, per, p * per)
        passes.append((K.camera_array(views[p * per:(p + 1) * per]),
                       (K._lib.KifsSubpixel * per)(*[K._lib.KifsSubpixel(i, j) for i, j in pairs])))
    out = torch.zeros((1, height, width, 4), dtype=torch.uint8, device="cuda:0")
    sums = torch.zeros((1, height, width, 4), dtype=torch.float32, device="cuda:0")
    torch.cuda.synchronize()

    def resume_frame():
        for p, (cams, cells) in enumerate(passes):
            gs.render_accumulate_resume(sums, p * per, cams, per, outs=out, stream=stream, jitter=(g, cells))

    mean, least = timed(stream, resume_frame, reps=3, warmup=1)
    emit(dict(kind="buys", rule=None, passes=n, per_pass=per, grid=g, total_ms=mean, total_min_ms=least))
    if not HAS_CONVERGE:
        return
    moments = torch.zeros((1, height, width), dtype=torch.float32, device="cuda:0")
    counts = torch.zeros((1,), dtype=torch.int32, device="cuda:0")
    for tol in (float(t) for t in args.tolerances.split(",")):
        rule = (tol, per)

        def converge_frame():
            for p, (cams, cells) in enumerate(passes):
                gs.render_accumulate_converge(sums, moments, cams, per, rule, restart=p == 0, counts=counts, outs=out, stream=stream,
                                              jitter=(g, cells))

        mean, least = timed(stream, converge_frame, reps=3, warmup=1)
        rows = []
        for p, (cams, cells) in enumerate(passes):  # once more pass by pass: the ms, the count after, the marched pixels' blocks
            before = sums[0, ..., 3].clone() if p else None
            stream.synchronize()
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record(stream)
            gs.render_accumulate_converge(sums, moments, cams, per, rule, restart=p == 0, counts=counts, outs=out, stream=stream,
                                          jitter=(g, cells))
            b.record(stream)
            stream.synchronize()
            torch.cuda.synchronize()
            marched = torch.ones((height, width), dtype=torch.bool, device="cuda:0") if p == 0 else sums[0, ..., 3] != before
            rows.append(dict(ms=round(a.elapsed_time(b), 4), marched=int(marched.sum()), active_after=int(counts.cpu()[0]),
                             marched_in_partly_active_blocks=partly_active_share(marched)))
        emit(dict(kind="buys", rule=dict(tolerance=tol, min_samples=per), passes=n, per_pass=per, grid=g, total_ms=mean, total_min_ms=least,
                  mean_rays_per_pixel=round(float(sums[0, ..., 3].mean()), 3), per_pass_rows=rows))


def main():
    w = WORKLOADS[args.workload]
    with K.GraphicState(0, screen_data=w.screen, camera_data=w.camera, gui_data=w.gui) as gs:
        gs.set_iters(*w.iters)
        if w.extensions:
            gs.set_extensions(**w.extensions)
        stream = torch.cuda.Stream()
        if args.only != "buys":
            price(gs, w, stream)
        if args.only != "price":
            buys(gs, w, stream)


if __name__ == "__main__":
    main()
