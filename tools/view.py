#!/usr/bin/env python3
"""Live viewer over HTTP: renders a workload on the GPU and serves the frames to a browser, whose mouse
drives the camera as the reference's window does (drag = rotate, wheel = zoom).

    python tools/view.py [workload] [--port 8080] [--host 127.0.0.1] [--seconds S] [--png-dir DIR] [--refine G,S,P]
                         [--tolerance T]

--refine G,S,P: while nothing moves, every idle redraw adds a pass of S jittered rays per pixel (cells of a G x G grid) to
the frame's linear sums and presents the refined picture, up to P passes; any input starts over.
"""
import argparse
import sys
from pathlib import Path

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("workload", nargs="?", default="cfg2_julia_1080p")
    ap.add_argument("--host", default="127.0.0.1")
    ap.add_argument("--port", type=int, default=8080)
    ap.add_argument("--seconds", type=float, default=None, help="stop after this long (default: until Ctrl-C)")
    ap.add_argument("--png-dir", default=None, help="also keep every presented frame as a PNG here")
    ap.add_argument("--refine", default=None, metavar="G,S,P",
                    help="refine the still picture: grid, jittered samples per pass (<= G*G, <= 64), passes")
    ap.add_argument("--tolerance", type=float, default=None, metavar="T",
                    help="with --refine: a pass marches only the pixels whose mean luminance has not settled to a standard "
                         "error of T, and the refinement stops once none is left (or at P passes)")
    args = ap.parse_args()
    if args.tolerance is not None and (not args.refine or not args.tolerance >= 0.0):
        ap.error("--tolerance T >= 0 goes with --refine")
    refine = None
    if args.refine:
        try:
            refine = tuple(int(v) for v in args.refine.split(","))
            assert len(refine) == 3
        except (ValueError, AssertionError):
            ap.error("--refine takes three integers: G,S,P")
    import kifs_raymarching_amd as K
    from kifs_raymarching_amd.configs import WORKLOADS
    from kifs_raymarching_amd.viewer import HttpSink, PngSequenceSink, ViewerSession
    w = WORKLOADS[args.workload]
    with K.GraphicState(0, screen_data=w.screen, camera_data=w.camera, gui_data=w.gui) as gs:
        gs.set_iters(*w.iters)
        session = ViewerSession(gs, refine=refine, tolerance=args.tolerance)
        http = HttpSink(args.host, args.port, on_input=session.handle)
        session.sinks.append(http)
        if args.png_dir:
            session.sinks.append(PngSequenceSink(args.png_dir))
        print(f"viewer: {http.url}  ({args.workload}, {w.screen.width}x{w.screen.height})", flush=True)
        session.run(args.seconds)
        print(f"{session.frames_presented} frames presented; last frame {session.last_frame_ms:.2f} ms "
              "(render + copy to the host)")
        session.close()


if __name__ == "__main__":
    main()
