#!/usr/bin/env python3
"""Render a workload (or an orbit of it) with the HIP library and write PNG files.

    python tools/render.py cfg2_julia_1080p out.png
    python tools/render.py cfg2_julia_1080p out.png --aa 3          # 3 x 3 supersampled
    python tools/render.py cfg2_julia_1080p out.png --aa-adaptive 3 # 3 x 3 supersampling for the edge pixels only
    python tools/render.py cfg2_julia_1080p out.png --geometry out.npz --depth-png depth.png   # + normal and hit distance
    python tools/render.py cfg5_sierpinski_8k_orbit frames/orbit_%03d.png --frames 0 30 60 --scale 0.25
    python tools/render.py cfg2_julia_1080p out.png --morph-to 0.3,0.5,-0.2,0.1 --frames 48   # out_000.png .. out_047.png
    python tools/render.py cfg2_julia_1080p orbit_%03d.png --frames 0 1 2 --motion-blur 16 --shutter 0.5   # motion blur
    python tools/render.py cfg2_julia_1080p out.png --dof 0.05,3.2 --samples 32                # depth of field
    python tools/render.py cfg2_julia_1080p out.png --morph-to 0.3,0.5,-0.2,0.1 --frames 48 --motion-blur 8   # a blurred morph
    python tools/render.py cfg2_julia_1080p orbit_%03d.png --frames 0 1 2 --motion-blur 16 --jitter 4   # blur that anti-aliases
    python tools/render.py cfg2_julia_1080p out.png --morph-to 0.3,0.5,-0.2,0.1 --frames 48 --aa 2           # an anti-aliased morph
    python tools/render.py cfg2_julia_1080p out.png --dof 0.05,3.2 --spp 400 --jitter 8        # a lens at print quality: 7 passes
    python tools/render.py cfg2_julia_1080p orbit_%03d.png --frames 0 1 2 --motion-blur 16 --spp 150   # 64 + 64 + 22 sub-frames
    python tools/render.py cfg2_julia_1080p pano.png --panorama 0,0,2.5                        # 360 degrees from a point
    python tools/render.py cfg2_julia_1080p out.png --dof 0.05 --focus-at 960,540 --samples 32 # focus on what that pixel hits
    python tools/render.py cfg2_julia_1080p out.png --ao --ao-png ao.png                       # ambient occlusion + its factors
    python tools/render.py cfg5_sierpinski_8k_orbit orbit_%03d.png --frames 0 30 60 --scale 0.25 --ao 8,0.01,0.8,3 --aa 2
    python tools/render.py cfg2_julia_1080p out.png --light -0.55,0.75,0.36,0.15,0.85 --specular 0.6,0.6,0.5,3 --ao  # a moved light
    python tools/render.py cfg2_julia_1080p out.png --trap 0,0,0,0 --trap-colours 255,140,0:20,60,200 --trap-range auto --ao  # orbit-trap colours
    python tools/render.py cfg5_sierpinski_8k_orbit out.png --scale 0.25 --fold menger --ao    # a Menger sponge (kaleidoscopic IFS)
    python tools/render.py cfg5_sierpinski_8k_orbit out.png --scale 0.25 --fold menger --trap 0,0,0,0,4 --trap-colours 255,140,0:20,60,200 --trap-range auto --ao  # ... coloured by its fold orbit
    python tools/render.py cfg5_sierpinski_8k_orbit out.png --scale 0.25 --fold abs+sort,6,2,1,0,0 --fold-rotate z,14,y,9 --light -0.55,0.75,0.36
"""
import argparse
import sys
from pathlib import Path

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))
import kifs_raymarching_amd as K  # noqa: E402
from kifs_raymarching_amd.configs import (WORKLOADS, jitter_cells, lens_cameras, morph_options, orbit_camera, panorama_rays,  # noqa: E402
                                          pass_splits, pixel_rays, shutter_cameras, trap_range, FOLD_PRESETS, fold_rotation)
from kifs_raymarching_amd.image import write_png  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("workload", choices=sorted(WORKLOADS))
ap.add_argument("out")
ap.add_argument("--frames", type=int, nargs="*", default=None,
                help="orbit frame indices (out needs %%d); with --morph-to: one number, the frames of the morph")
ap.add_argument("--morph-to", metavar="R,I,J,K", default=None,
                help="a morph of the constant from the workload's to this quaternion, --frames N frames in launches of up to "
                     "512 (kifs_render_animation_async), written to OUT_000.png ..; with --aa K every frame is the K x K cells of "
                     "kifs_render_accumulate_jittered_async; not with --aa-adaptive or --geometry")
ap.add_argument("--scale", type=float, default=1.0, help="resolution scale")
ap.add_argument("--heatmap", action="store_true")
ap.add_argument("--aa", type=int, default=1, metavar="K", help="K x K supersampled anti-aliasing (1..4; 1 = off)")
ap.add_argument("--aa-adaptive", type=int, default=0, metavar="K",
                help="adaptive anti-aliasing (kifs_render_adaptive_async): K x K samples (2..4) for the pixels whose geometry "
                     "differs from a neighbour's, the plain pixel elsewhere; prints the share supersampled; not with --aa, "
                     "--geometry or --frames")
ap.add_argument("--aa-normal-cos", type=float, default=0.9, metavar="X",
                help="with --aa-adaptive: neighbouring hits whose normals' dot product is below X are an edge")
ap.add_argument("--aa-depth-rel", type=float, default=0.05, metavar="Y",
                help="with --aa-adaptive: neighbouring hits whose distances differ by more than Y of the nearer one are an edge")
ap.add_argument("--geometry", metavar="OUT.npz", default=None,
                help="also write the frame's geometry plane (kifs_render_geometry_async): arrays rgba (H, W, 4) uint8, "
                     "normal (H, W, 3) float32 and t (H, W) float32, +inf where the ray missed; not with --aa or --frames")
ap.add_argument("--depth-png", metavar="OUT.png", default=None,
                help="with --geometry: t as a grey image for a quick look (nearest hit white, misses black)")
ap.add_argument("--motion-blur", type=int, default=0, metavar="S",
                help="accumulated frames (kifs_render_accumulate_async): every orbit frame of --frames is the linear-colour mean "
                     "of S sub-frames (1..64) spread over the shutter interval; with --morph-to: every frame of the morph the "
                     "mean of S steps of it (per-sub-frame options); not with --aa, --aa-adaptive or --geometry")
ap.add_argument("--shutter", type=float, default=0.5, metavar="F",
                help="with --motion-blur on orbit frames: the shutter is open for F x the angle between two frames")
ap.add_argument("--dof", metavar="APERTURE,FOCUS", default=None,
                help="depth of field: the mean of --samples S sub-frames whose cameras sit on a lens of radius APERTURE and "
                     "share the plane at distance FOCUS; one frame, or the orbit frames of --frames; not with --motion-blur, "
                     "--morph-to, --aa, --aa-adaptive or --geometry")
ap.add_argument("--samples", type=int, default=16, metavar="S", help="with --dof: sub-frames per frame (1..64)")
ap.add_argument("--jitter", type=int, default=0, metavar="G",
                help="with --motion-blur S or --dof .. --samples S (S <= G x G): sub-frame s goes through its own cell of a "
                     f"G x G grid inside the pixel (1..{K.MAX_JITTER_GRID}; kifs_render_accumulate_jittered_async, cells from "
                     "configs.jitter_cells), so the blur's rays anti-alias as well")
ap.add_argument("--spp", type=int, default=None, metavar="N",
                help="with --dof, --motion-blur (also with --morph-to) and --jitter: N sub-frames per output frame in all, "
                     "instead of --samples S / --motion-blur S -- progressive accumulation "
                     "(kifs_render_accumulate_resume_async): passes of at most 64 (with --jitter G: at most G x G) carry the "
                     "frame's linear sums, only the last one encodes; N may be far above 64")
ap.add_argument("--tolerance", type=float, default=None, metavar="T",
                help="with --spp N: stop sampling the pixels whose mean luminance has settled to a standard error of T "
                     "(kifs_render_accumulate_converge_async) and stop the passes once none is left; N stays the cap")
ap.add_argument("--min-samples", type=int, default=16, metavar="M",
                help="with --tolerance: a pixel holding fewer than M sub-frames never stops (at least 2)")
ap.add_argument("--panorama", metavar="X,Y,Z", default=None,
                help="the equirectangular picture of the scene from the point X,Y,Z (kifs_trace_rays_async over "
                     "configs.panorama_rays): as wide as the workload's frame and half as high; on its own")
ap.add_argument("--focus-at", metavar="X,Y", default=None,
                help="with --dof APERTURE (no FOCUS): focus on what pixel X,Y of the frame shows -- its ray is traced "
                     "(kifs_trace_rays_async) and the focus distance is t * dot(dir, -m0), which is printed; a pixel that "
                     "shows the background ends the run with status 1; one frame, not with --frames")
ap.add_argument("--ao", metavar="S,STEP,DECAY,STRENGTH", nargs="?", const="5,0.02,0.75,4.0", default=None,
                help="ambient occlusion: S probes along the normal STEP apart, each weighted DECAY times the one before, "
                     "times STRENGTH (default 5,0.02,0.75,4.0); goes with --aa, --frames and the shadow workloads")
ap.add_argument("--ao-png", metavar="OUT.png", default=None,
                help="with --ao (one frame, no --aa): also write the factors as a grey picture, white = open")
ap.add_argument("--light", metavar="X,Y,Z[,AMBIENT,DIFFUSE]", default=None,
                help="light the hits from direction X,Y,Z (towards the light, used as given in the direct term) with the "
                     "weights AMBIENT,DIFFUSE (default 0.1,0.9); goes with --ao, --aa, --frames and the shadow workloads")
ap.add_argument("--specular", metavar="R,G,B[,E]", default=None,
                help="a Blinn-Phong highlight of linear weight R,G,B and exponent 2^E (E 0..10, default 5) under --light "
                     "(without --light: under the reference's light 1,1,1)")
ap.add_argument("--trap", metavar="CX,CY,CZ,CW[,AXES[,K]]", default=None,
                help="colour the hits by an orbit trap (kifs_render_trapped_async): the least distance of the hit point's orbit to "
                     "the point CX,CY,CZ,CW of orbit space over the components of the mask AXES (x = 1, y = 2, z = 4, w = 8; "
                     "default 15, a point trap) within K orbit points (0..32, default 8), through a gradient from the workload's "
                     "colour; goes with --light, --specular, --ao, --aa, --frames and the shadow workloads, and with --fold "
                     "(kifs_render_folded_trapped_async: the orbit is then the fold's own, continued by the base primitive's)")
ap.add_argument("--trap-colours", metavar="R,G,B:R,G,B", default="255,140,0:20,60,200",
                help="with --trap: the gradient's middle and far stops as sRGB bytes")
ap.add_argument("--trap-range", metavar="LO,HI|auto", default="auto",
                help="with --trap: the distances that take the gradient's first and last stop; auto: the 5th and 95th "
                     "percentile of the distances at the first frame's hits (kifs_render_geometry_async and kifs_eval_trap; with "
                     "--fold the plane of u of kifs_render_folded_trapped_async)")
ap.add_argument("--fold", metavar="PRESET|STAGES,N,SCALE,CX,CY,CZ", default=None,
                help="a kaleidoscopic IFS scene (kifs_render_folded_async): the base primitive seen through N rounds of the "
                     "stages STAGES (a mask 0..31, or names joined by +: abs+sort+tetra+rotate+mirror_z), scaled by SCALE about "
                     f"CX,CY,CZ -- or a preset ({', '.join(sorted(FOLD_PRESETS))}), which also picks the base primitive; a KIFS "
                     "workload; goes with --light, --specular, --ao, --aa, --frames and the shadow workloads")
ap.add_argument("--fold-rotate", metavar="AXIS,DEG[,AXIS,DEG..]", default=None,
                help="with --fold STAGES,..: the rotation of the rotate stage as a chain of axis rotations in degrees "
                     "(configs.fold_rotation), which also switches that stage on")
args = ap.parse_args()
def _numbers(text, count):
    try:
        v = tuple(float(x) for x in text.split(","))
    except ValueError:
        v = ()
    return v if len(v) == count else None
panorama = None
if args.panorama is not None:
    panorama = _numbers(args.panorama, 3)
    others = (args.frames, args.morph_to, args.geometry, args.depth_png, args.dof, args.spp, args.tolerance, args.focus_at, args.ao, args.ao_png,
              args.light, args.specular, args.trap, args.fold)
    if panorama is None or args.aa != 1 or args.aa_adaptive or args.motion_blur or args.jitter or any(o is not None for o in others):
        ap.error("--panorama takes three numbers X,Y,Z and renders on its own (--scale and --heatmap apply; no --ao, --light or "
                 "--specular: ray queries compute neither the term nor a light of the caller's)")
focus_at = None
if args.focus_at is not None:
    focus_at = _numbers(args.focus_at, 2)
    if focus_at is None or args.dof is None or args.frames is not None or any(v < 0 or v != int(v) for v in focus_at):
        ap.error("--focus-at takes a pixel X,Y and goes with --dof APERTURE, without --frames")
    args.dof = args.dof + ",1"  # (the focus distance is traced below)
if args.tolerance is not None and (args.spp is None or not args.tolerance >= 0.0 or not 2 <= args.min_samples <= 1 << 24):
    ap.error("--tolerance T >= 0 goes with --spp, --min-samples M within 2..16777216")
dof = None
if args.dof is not None:
    try:
        dof = tuple(float(x) for x in args.dof.split(","))
    except ValueError:
        dof = ()
    if len(dof) != 2 or not dof[1] > 0.0:
        ap.error("--dof takes two numbers APERTURE,FOCUS with a positive focus distance")
    if args.motion_blur or args.morph_to is not None:
        ap.error("--dof goes without --motion-blur and --morph-to")
accumulate = args.motion_blur or (args.samples if dof else 0)
if args.spp is not None:
    if not accumulate:
        ap.error("--spp goes with --dof or --motion-blur")
    if not 1 <= args.spp <= 1 << 24:
        ap.error("--spp N: 1..16777216 sub-frames per frame")
    accumulate = args.spp
elif (args.motion_blur or dof) and not 1 <= accumulate <= K.MAX_ACCUMULATE:
    ap.error(f"1..{K.MAX_ACCUMULATE} sub-frames per frame (more with --spp)")
if accumulate and (args.aa != 1 or args.aa_adaptive or args.geometry):
    ap.error("--motion-blur and --dof render without --aa, --aa-adaptive or --geometry")
if args.jitter:
    if not accumulate:
        ap.error("--jitter goes with --motion-blur or --dof")
    if not 1 <= args.jitter <= K.MAX_JITTER_GRID or (accumulate > args.jitter ** 2 and args.spp is None):
        ap.error(f"--jitter G: 1..{K.MAX_JITTER_GRID}, with at most G x G sub-frames per frame")
# --aa K for a morph or several orbit frames: one launch, every frame the K x K cells of a pixel in supersampling order
aa_grid = args.aa > 1 and not accumulate and (args.morph_to is not None or (args.frames is not None and len(args.frames) > 1))
if args.motion_blur and args.morph_to is None and not args.frames:
    ap.error("--motion-blur needs the orbit frames of --frames (or --morph-to)")
if args.geometry and (args.aa != 1 or args.frames is not None):
    ap.error("--geometry renders one frame without supersampling")
if args.aa_adaptive and (args.aa != 1 or args.geometry or args.frames is not None):
    ap.error("--aa-adaptive renders one frame, without --aa or --geometry")
if args.depth_png and not args.geometry:
    ap.error("--depth-png goes with --geometry")
ao = None
if args.ao is not None:
    numbers = _numbers(args.ao, 4)
    if numbers is None or numbers[0] != int(numbers[0]):
        ap.error("--ao takes four numbers S,STEP,DECAY,STRENGTH (S a whole number)")
    ao = K.AmbientOcclusion(int(numbers[0]), numbers[1], numbers[2], numbers[3])
    # the term exists in kifs_render_occlusion_async alone
    if accumulate or args.jitter or args.aa_adaptive or args.geometry or args.morph_to is not None:
        ap.error("--ao renders without --motion-blur, --dof, --spp, --jitter, --aa-adaptive, --geometry and --morph-to: "
                 "the accumulate, adaptive, geometry and animation entry points do not compute the term")
    aa_grid = False  # several supersampled frames go through the occlusion batch, not through the accumulate family
if args.ao_png and (ao is None or args.aa != 1 or args.frames is not None):
    ap.error("--ao-png goes with --ao, one frame, without --aa: a resolved pixel has no single factor")
light = None
if args.light is not None or args.specular is not None:
    # the light exists in kifs_render_lit_async alone
    if accumulate or args.jitter or args.aa_adaptive or args.geometry or args.morph_to is not None:
        ap.error("--light and --specular render without --motion-blur, --dof, --spp, --jitter, --aa-adaptive, --geometry and "
                 "--morph-to: the accumulate, adaptive, geometry and animation entry points shade with the reference's light")
    if args.ao_png:
        ap.error("--ao-png goes without --light and --specular: the lit call writes no plane of factors")
    lit = (1.0, 1.0, 1.0, 0.1, 0.9)
    if args.light is not None:
        lit = _numbers(args.light, 5) or ((_numbers(args.light, 3) or ()) + (0.1, 0.9))
        if len(lit) != 5:
            ap.error("--light takes three numbers X,Y,Z or five X,Y,Z,AMBIENT,DIFFUSE")
    shine = (0.0, 0.0, 0.0, 5.0)
    if args.specular is not None:
        shine = _numbers(args.specular, 4) or ((_numbers(args.specular, 3) or ()) + (5.0,))
        if len(shine) != 4 or shine[3] != int(shine[3]):
            ap.error("--specular takes three numbers R,G,B or four R,G,B,E (E a whole number)")
    light = K.Light(direction=lit[:3], ambient=lit[3], diffuse=lit[4], specular=shine[:3], shininess_log2=int(shine[3]))
    aa_grid = False  # several supersampled frames go through the lit batch, not through the accumulate family
trap = None
if args.trap is not None:
    # the trap exists in kifs_render_trapped_async alone
    if accumulate or args.jitter or args.aa_adaptive or args.geometry or args.morph_to is not None:
        ap.error("--trap renders without --motion-blur, --dof, --spp, --jitter, --aa-adaptive, --geometry and --morph-to: the "
                 "accumulate, adaptive, geometry and animation entry points colour with the one fractal colour")
    if args.ao_png:
        ap.error("--ao-png goes without --trap: the trapped call writes no plane of factors")
    given = args.trap.count(",") + 1
    numbers = (_numbers(args.trap, given) or ()) + (15.0, 8.0)[max(given - 4, 0):]  # (the defaults of what was left out)
    if not 4 <= given <= 6 or len(numbers) != 6 or numbers[4] != int(numbers[4]) or numbers[5] != int(numbers[5]):
        ap.error("--trap takes four numbers CX,CY,CZ,CW, then optionally the mask AXES and the count K (whole numbers)")
    stops = [_numbers(part, 3) for part in args.trap_colours.split(":")]
    if len(stops) != 2 or None in stops or any(v != int(v) or not 0 <= v <= 255 for stop in stops for v in stop):
        ap.error("--trap-colours takes two sRGB colours R,G,B:R,G,B of bytes")
    span = None if args.trap_range == "auto" else _numbers(args.trap_range, 2)
    if args.trap_range != "auto" and (span is None or span[0] == span[1]):
        ap.error("--trap-range takes two different distances LO,HI, or auto")
    trap = K.OrbitTrap(centre=numbers[:4], axes=int(numbers[4]), iterations=int(numbers[5]), mid=tuple(int(v) for v in stops[0]),
                       far=tuple(int(v) for v in stops[1]))
    try:
        trap.into_buffer_data()
    except ValueError as e:
        ap.error(f"--trap: {e}")
    if span is not None:
        trap.scale, trap.bias = (float(v) for v in trap_range(*span))
    aa_grid = False  # several supersampled frames go through the trapped batch, not through the accumulate family
fold, fold_base = None, None
if args.fold is not None:
    # the folded estimate exists in kifs_render_folded_async and, with --trap, in kifs_render_folded_trapped_async
    if accumulate or args.jitter or args.aa_adaptive or args.geometry or args.morph_to is not None:
        ap.error("--fold renders without --motion-blur, --dof, --spp, --jitter, --aa-adaptive, --geometry and --morph-to: "
                 "the accumulate, adaptive, geometry and animation entry points march the unfolded scene")
    if args.ao_png:
        ap.error("--ao-png goes without --fold: the folded calls write no plane of factors")
    if args.fold in FOLD_PRESETS:
        if args.fold_rotate is not None:
            ap.error("--fold-rotate goes with --fold STAGES,..: a preset brings its own rotation")
        fold_base, fold = FOLD_PRESETS[args.fold]
    else:
        parts = args.fold.split(",")
        numbers = _numbers(",".join(parts[1:]), 5) if len(parts) == 6 else None
        if numbers is None or numbers[0] != int(numbers[0]):
            ap.error(f"--fold takes a preset ({', '.join(sorted(FOLD_PRESETS))}) or STAGES,N,SCALE,CX,CY,CZ (N a whole number)")
        stages = int(parts[0]) if parts[0].strip().isdigit() else parts[0].replace("+", ",")
        fold = K.FoldSystem(stages=stages, iterations=int(numbers[0]), scale=numbers[1], offset=numbers[2:5])
        if args.fold_rotate is not None:
            turns = args.fold_rotate.split(",")
            try:
                import math
                pairs = [(turns[i].strip(), math.radians(float(turns[i + 1]))) for i in range(0, len(turns) - 1, 2)]
                if len(turns) % 2 or not pairs:
                    raise ValueError("pairs of AXIS,DEG")
                fold.rotation = fold_rotation(*pairs)
                fold.stages = fold.stage_bits() | 8
            except (ValueError, TypeError) as e:
                ap.error(f"--fold-rotate takes AXIS,DEG[,AXIS,DEG..] with the axes x, y, z: {e}")
    try:
        fold.into_buffer_data()
    except ValueError as e:
        ap.error(f"--fold: {e}")
    aa_grid = False  # several supersampled frames go through the folded batch, not through the accumulate family
elif args.fold_rotate is not None:
    ap.error("--fold-rotate goes with --fold")
morph_to = None
if args.morph_to is not None:
    try:
        morph_to = tuple(float(x) for x in args.morph_to.split(","))
    except ValueError:
        morph_to = ()
    if len(morph_to) != 4:
        ap.error("--morph-to takes four numbers R,I,J,K")
    if args.aa_adaptive or args.geometry:
        ap.error("--morph-to renders without --aa-adaptive or --geometry")
    if args.frames is None or len(args.frames) != 1 or args.frames[0] < 1:
        ap.error("--morph-to needs --frames N, the number of frames (at least 1)")
w = WORKLOADS[args.workload]
screen = K.ScreenData(max(1, int(w.screen.width * args.scale)), max(1, int(w.screen.height * args.scale)))
gui = w.gui
if fold is not None:
    if gui.fractal_group != K.FractalGroup.KaleidoscopicIFS:
        ap.error("--fold takes a KIFS workload: the two Julia pipelines have no folded form")
    if fold_base is not None:
        gui = K.GuiData(**{**gui.__dict__, "primitive_shape": fold_base})
if args.heatmap:
    gui = K.GuiData(**{**gui.__dict__, "is_heatmap": True, "fractal_color": (255, 255, 255)})
with K.GraphicState(0, screen_data=screen, camera_data=w.camera, gui_data=gui) as gs:
    gs.set_iters(*w.iters)
    if w.extensions:
        gs.set_extensions(**w.extensions)
    gs.set_supersampling(1 if aa_grid else args.aa)
    if focus_at is not None:
        import numpy as np
        x, y = int(focus_at[0]), int(focus_at[1])
        if x >= screen.width or y >= screen.height:
            sys.exit(f"--focus-at {x},{y}: outside the {screen.width}x{screen.height} frame")
        ray = pixel_rays(screen, w.camera)[y * screen.width + x]
        geometry, _ = gs.trace_rays((ray[None, 0:3], ray[None, 4:7]), colours=False)
        gs.synchronize()
        t = geometry.cpu().numpy()[0, 3]
        if not np.isfinite(t):
            print(f"--focus-at {x},{y}: the pixel's ray misses the scene, nothing to focus on")
            sys.exit(1)
        m0 = np.array(w.camera.into_buffer_data().matrix[0][:3], dtype=np.float32)
        d = ray[4:7]
        focus = t * ((d[0] * -m0[0] + d[1] * -m0[1]) + d[2] * -m0[2])  # f32: the hit's distance along the view axis
        print(f"--focus-at {x},{y}: hit at t = {float(t):.6g}, focus distance {float(focus):.6g}")
        if not focus > 0.0:
            sys.exit(1)
        dof = (dof[0], float(focus))
    jitter_of = lambda frames, S: None if not args.jitter else (args.jitter, [c for k in frames for c in jitter_cells(args.jitter, S, k or 0)])
    if panorama is not None:
        pw, ph = screen.width, max(1, screen.width // 2)
        import torch
        rays = torch.from_numpy(panorama_rays(panorama, pw, ph)).to(f"cuda:{gs.device}")
        geometry, rgba = gs.trace_rays(rays)
        gs.synchronize()
        write_png(args.out, rgba.cpu().numpy().reshape(ph, pw, 4))
        hit = torch.isfinite(geometry[:, 3])
        print(f"{args.out}: {pw}x{ph} equirectangular from {panorama}, {int(hit.sum())} rays hit")
    elif args.geometry:
        import numpy as np
        colour, geometry = gs.render_geometry()
        rgba, geometry = colour.cpu().numpy(), geometry.cpu().numpy()
        write_png(args.out, rgba)
        np.savez_compressed(args.geometry, rgba=rgba, normal=geometry[..., :3], t=geometry[..., 3])
        hit = np.isfinite(geometry[..., 3])
        print(f"{args.out}, {args.geometry}: {screen.width}x{screen.height}, {int(hit.sum())} pixels hit")
        if args.depth_png:
            t = geometry[..., 3]
            grey = np.zeros(t.shape, dtype=np.uint8)
            if hit.any():
                lo, hi = float(t[hit].min()), float(t[hit].max())
                grey[hit] = (255.0 - 215.0 * (t[hit] - lo) / max(hi - lo, 1e-30)).astype(np.uint8)
            write_png(args.depth_png, np.dstack([grey, grey, grey, np.full_like(grey, 255)]))
    elif args.aa_adaptive:
        colour, edges = gs.render_adaptive(k=args.aa_adaptive, normal_cos=args.aa_normal_cos, depth_rel=args.aa_depth_rel)
        write_png(args.out, colour.cpu().numpy())
        pixels = screen.width * screen.height
        print(f"{args.out}: {screen.width}x{screen.height}, {edges} of {pixels} pixels supersampled "
              f"{args.aa_adaptive}x{args.aa_adaptive} ({100.0 * edges / pixels:.2f} %)")
    elif args.spp is not None:
        # progressive accumulation: N sub-frames per frame as passes that carry the frames' linear sums (K.Accumulator);
        # the views are those of the one-launch forms below for S = N, handed out pass by pass
        N, G = args.spp, args.jitter
        splits = pass_splits(N, min(K.MAX_ACCUMULATE, G * G) if G else K.MAX_ACCUMULATE)
        morph = morph_to is not None
        if morph:
            n = args.frames[0]
            guis = morph_options(gui, K.GuiData(**{**gui.__dict__, "constant": morph_to}), n * N)
            indices, out = list(range(n)), Path(args.out)
        else:
            indices = args.frames if args.frames is not None else [None]
        per_call = max(1, K.MAX_BATCH // max(splits))
        for first in range(0, len(indices), per_call):
            part = indices[first:first + per_call]
            cams, opts = [], None
            for k in part:
                if morph:
                    cams.append([w.camera.into_buffer_data()] * N)
                elif dof:
                    cams.append(lens_cameras(w.camera if k is None else orbit_camera(w, k), dof[0], dof[1], N))
                else:
                    cams.append([c.into_buffer_data() for c in shutter_cameras(w, k, N, args.shutter)])
            if morph:
                opts = [guis[k * N:(k + 1) * N] for k in part]
            converging = args.tolerance is not None
            acc = (K.ConvergingAccumulator(gs, count=len(part), tolerance=args.tolerance, min_samples=args.min_samples) if converging
                   else K.Accumulator(gs, count=len(part)))
            done, frames, passes_run = 0, None, 0
            for p, S in enumerate(splits):
                jitter = None if not G else (G, [c for k in part for c in jitter_cells(G, S, (k or 0) + done)])
                # (a converging run does not know its last pass beforehand: every pass encodes, into the same frames)
                frames = acc.add([cams[f][done + s] for f in range(len(part)) for s in range(S)], S,
                                 options=None if opts is None else [opts[f][done + s] for f in range(len(part)) for s in range(S)],
                                 picture=converging or p == len(splits) - 1, jitter=jitter, outs=frames)
                done += S
                passes_run += 1
                if converging and not any(acc.active()):
                    break
            gs.synchronize()
            if converging:
                rays = acc.samples_per_pixel().mean(dim=(1, 2)).cpu().tolist()
            for k, frame in zip(part, frames.cpu().numpy()):
                path = str(out.with_name(f"{out.stem}_{k:03d}{out.suffix}")) if morph else args.out if k is None else args.out % k
                write_png(path, frame)
                if converging:
                    print(f"{path}: {screen.width}x{screen.height}, tolerance {args.tolerance:g}: {passes_run} of {len(splits)} passes run"
                          f"{' (stopped early)' if passes_run < len(splits) else ''}, {rays[part.index(k)]:.2f} rays per pixel on average "
                          f"of at most {N}" + (f", jittered over a {G}x{G} grid" if G else ""))
                    continue
                print(f"{path}: {screen.width}x{screen.height}, the mean of {N} sub-frames in {len(splits)} passes"
                      + (f", jittered over a {G}x{G} grid" if G else ""))
    elif morph_to is not None and args.motion_blur:
        # frame i of the morph is the mean of steps i S .. i S + S - 1 of a morph of n S steps
        n, S = args.frames[0], args.motion_blur
        guis = morph_options(gui, K.GuiData(**{**gui.__dict__, "constant": morph_to}), n * S)
        out = Path(args.out)
        per_call = max(1, K.MAX_BATCH // S)
        for first in range(0, n, per_call):
            sub = guis[first * S:(first + per_call) * S]
            frames = gs.render_accumulate([w.camera] * len(sub), S, options=sub, jitter=jitter_of(range(first, first + len(sub) // S), S))
            gs.synchronize()
            for i, frame in enumerate(frames.cpu().numpy(), start=first):
                write_png(str(out.with_name(f"{out.stem}_{i:03d}{out.suffix}")), frame)
        print(f"{out.with_name(out.stem + '_000' + out.suffix)} .. : {n} frames of {screen.width}x{screen.height}, each the mean "
              f"of {S} steps, constant {tuple(gui.constant)} -> {morph_to}")
    elif accumulate:
        # motion blur over the orbit's frames, or depth of field for one frame / the orbit's frames
        S = accumulate
        indices = args.frames if args.frames is not None else [None]
        per_call = max(1, K.MAX_BATCH // S)
        for first in range(0, len(indices), per_call):
            part = indices[first:first + per_call]
            cams = []
            for k in part:
                if dof:
                    cams.extend(lens_cameras(w.camera if k is None else orbit_camera(w, k), dof[0], dof[1], S))
                else:
                    cams.extend(c.into_buffer_data() for c in shutter_cameras(w, k, S, args.shutter))
            frames = gs.render_accumulate(cams, S, jitter=jitter_of(part, S))
            gs.synchronize()
            for k, frame in zip(part, frames.cpu().numpy()):
                path = args.out if k is None else args.out % k
                write_png(path, frame)
                print(f"{path}: {screen.width}x{screen.height}, the mean of {S} sub-frames "
                      + (f"(lens radius {dof[0]}, focus at {dof[1]})" if dof else f"(shutter {args.shutter})")
                      + (f", jittered over a {args.jitter}x{args.jitter} grid" if args.jitter else ""))
    elif trap is not None and fold is not None:
        import numpy as np
        indices = args.frames if args.frames is not None else [None]
        cams = [w.camera if k is None else orbit_camera(w, k) for k in indices]
        try:
            if args.trap_range == "auto":
                # the first frame once with the plane of u (one ray per pixel), and the middle nine tenths of what the trap
                # measures at its hits -- what render_geometry and eval_trap do for an unfolded scene
                gs.set_supersampling(1)
                gs.set_camera(cams[0])
                _, plane = gs.render_folded_trapped(fold, trap, u_plane=True)
                gs.set_supersampling(args.aa)
                u = plane.cpu().numpy().reshape(-1)
                u = u[np.isfinite(u)]
                if not u.size:
                    sys.exit("--trap-range auto: no ray of the first frame hits the scene, nothing to take a range from")
                lo, hi = (float(v) for v in np.percentile(u, [5.0, 95.0]))
                if not hi > lo:
                    hi = lo + 1.0  # (a trap that measures one distance everywhere: the first stop's colour)
                trap.scale, trap.bias = (float(v) for v in trap_range(lo, hi))
                print(f"--trap-range auto: {u.size} hits, distances {float(u.min()):.4g} .. {float(u.max()):.4g}, range {lo:.4g},{hi:.4g}")
            colour = gs.render_folded_trapped_batch(cams, fold, trap, light=light, ao=ao)
        except K.KifsError as e:
            sys.exit(f"--fold {args.fold} --trap {args.trap}: {e}")
        gs.synchronize()
        for k, frame in zip(indices, colour.cpu().numpy()):
            path = args.out if k is None else args.out % k
            write_png(path, frame)
            print(f"{path}: {screen.width}x{screen.height}, {K.PrimitiveShape(gui.primitive_shape).name} folded {fold.iterations} times "
                  f"(stages {fold.stage_bits()}, scale {fold.scale}, offset {tuple(fold.offset)}), orbit trap at {tuple(trap.centre)} "
                  f"(axes {trap.axes}, {trap.iterations} orbit points, scale {trap.scale:.6g}, bias {trap.bias:.6g}), stops "
                  f"{tuple(trap.mid)} and {tuple(trap.far)}"
                  + (f", lit from {tuple(light.direction)}" if light is not None else "")
                  + (f", ambient occlusion ({ao.samples} probes)" if ao is not None else "")
                  + (f", {args.aa}x{args.aa} supersampled" if args.aa > 1 else ""))
    elif trap is not None:
        import numpy as np
        indices = args.frames if args.frames is not None else [None]
        cams = [w.camera if k is None else orbit_camera(w, k) for k in indices]
        if args.trap_range == "auto":
            # where the first frame's rays hit (one ray per pixel), what the trap measures there, and its middle nine tenths
            gs.set_supersampling(1)
            gs.set_camera(cams[0])
            _, geometry = gs.render_geometry()
            gs.set_supersampling(args.aa)
            t = geometry.cpu().numpy()[..., 3].reshape(-1)
            hit = np.isfinite(t)
            if not hit.any():
                sys.exit("--trap-range auto: no ray of the first frame hits the scene, nothing to take a range from")
            rays = pixel_rays(screen, cams[0])[hit]
            u = gs.eval_trap(trap, rays[:, 0:3] + t[hit, None] * rays[:, 4:7])
            lo, hi = (float(v) for v in np.percentile(u[np.isfinite(u)], [5.0, 95.0]))
            if not hi > lo:
                hi = lo + 1.0  # (a trap that measures one distance everywhere: the first stop's colour)
            trap.scale, trap.bias = (float(v) for v in trap_range(lo, hi))
            print(f"--trap-range auto: {int(hit.sum())} hits, distances {float(u.min()):.4g} .. {float(u.max()):.4g}, range {lo:.4g},{hi:.4g}")
        try:
            colour = gs.render_trapped_batch(cams, trap, light=light, ao=ao)
        except K.KifsError as e:
            sys.exit(f"--trap {args.trap}: {e}")
        gs.synchronize()
        for k, frame in zip(indices, colour.cpu().numpy()):
            path = args.out if k is None else args.out % k
            write_png(path, frame)
            print(f"{path}: {screen.width}x{screen.height}, orbit trap at {tuple(trap.centre)} (axes {trap.axes}, {trap.iterations} orbit "
                  f"points, scale {trap.scale:.6g}, bias {trap.bias:.6g}), stops {tuple(trap.mid)} and {tuple(trap.far)}"
                  + (f", lit from {tuple(light.direction)}" if light is not None else "")
                  + (f", ambient occlusion ({ao.samples} probes)" if ao is not None else "")
                  + (f", {args.aa}x{args.aa} supersampled" if args.aa > 1 else ""))
    elif fold is not None:
        indices = args.frames if args.frames is not None else [None]
        cams = [w.camera if k is None else orbit_camera(w, k) for k in indices]
        try:
            colour = gs.render_folded_batch(cams, fold, light=light, ao=ao)
        except K.KifsError as e:
            sys.exit(f"--fold {args.fold}: {e}")
        gs.synchronize()
        for k, frame in zip(indices, colour.cpu().numpy()):
            path = args.out if k is None else args.out % k
            write_png(path, frame)
            print(f"{path}: {screen.width}x{screen.height}, {K.PrimitiveShape(gui.primitive_shape).name} folded {fold.iterations} times "
                  f"(stages {fold.stage_bits()}, scale {fold.scale}, offset {tuple(fold.offset)})"
                  + (f", lit from {tuple(light.direction)}" if light is not None else "")
                  + (f", ambient occlusion ({ao.samples} probes)" if ao is not None else "")
                  + (f", {args.aa}x{args.aa} supersampled" if args.aa > 1 else ""))
    elif light is not None:
        indices = args.frames if args.frames is not None else [None]
        cams = [w.camera if k is None else orbit_camera(w, k) for k in indices]
        try:
            colour = gs.render_lit_batch(cams, light, ao=ao)
        except K.KifsError as e:
            sys.exit(f"--light {args.light} --specular {args.specular}: {e}")
        gs.synchronize()
        for k, frame in zip(indices, colour.cpu().numpy()):
            path = args.out if k is None else args.out % k
            write_png(path, frame)
            print(f"{path}: {screen.width}x{screen.height}, lit from {tuple(light.direction)} (ambient {light.ambient}, diffuse "
                  f"{light.diffuse}" + (f", highlight {tuple(light.specular)} at 2^{light.shininess_log2}" if any(light.specular) else "")
                  + ")" + (f", ambient occlusion ({ao.samples} probes)" if ao is not None else "")
                  + (f", {args.aa}x{args.aa} supersampled" if args.aa > 1 else ""))
    elif ao is not None:
        import numpy as np
        indices = args.frames if args.frames is not None else [None]
        cams = [w.camera if k is None else orbit_camera(w, k) for k in indices]
        try:
            colour, plane = gs.render_occlusion_batch(cams, ao=ao, occlusion=bool(args.ao_png))
        except K.KifsError as e:
            sys.exit(f"--ao {args.ao}: {e}")
        gs.synchronize()
        for k, frame in zip(indices, colour.cpu().numpy()):
            path = args.out if k is None else args.out % k
            write_png(path, frame)
            print(f"{path}: {screen.width}x{screen.height}, ambient occlusion ({ao.samples} probes {ao.step} apart, decay "
                  f"{ao.decay}, strength {ao.strength})" + (f", {args.aa}x{args.aa} supersampled" if args.aa > 1 else ""))
        if args.ao_png:
            a = plane.cpu().numpy()[0]
            grey = np.where(np.isnan(a), 0.0, a * 255.0).astype(np.uint8)
            write_png(args.ao_png, np.dstack([grey, grey, grey, np.full_like(grey, 255)]))
            print(f"{args.ao_png}: {int((a < 1).sum())} pixels occluded, {int((a == 0).sum())} of them fully")
    elif aa_grid:
        # the whole grid: K x K sub-frames per frame that differ in their cell alone -- the supersampled frame's bytes
        S = args.aa * args.aa
        out = Path(args.out)
        if morph_to is not None:
            n = args.frames[0]
            guis = morph_options(gui, K.GuiData(**{**gui.__dict__, "constant": morph_to}), n)
            todo = [(str(out.with_name(f"{out.stem}_{i:03d}{out.suffix}")), w.camera, guis[i]) for i in range(n)]
        else:
            todo = [(args.out % k, orbit_camera(w, k), gui) for k in args.frames]
        per_call = max(1, K.MAX_BATCH // S)
        for first in range(0, len(todo), per_call):
            part = todo[first:first + per_call]
            frames = gs.render_accumulate([cam for _, cam, _ in part for _ in range(S)], S,
                                          options=[g for _, _, g in part for _ in range(S)], jitter=(args.aa, None))
            gs.synchronize()
            for (path, _, _), frame in zip(part, frames.cpu().numpy()):
                write_png(path, frame)
        print(f"{todo[0][0]} .. : {len(todo)} frames of {screen.width}x{screen.height}, {args.aa}x{args.aa} supersampled, up to "
              f"{per_call} frames per launch")
    elif morph_to is not None:
        n = args.frames[0]
        guis = morph_options(gui, K.GuiData(**{**gui.__dict__, "constant": morph_to}), n)
        out = Path(args.out)
        for first in range(0, n, K.MAX_BATCH):
            frames = gs.render_animation(guis[first:first + K.MAX_BATCH])
            gs.synchronize()
            for i, frame in enumerate(frames.cpu().numpy(), start=first):
                write_png(str(out.with_name(f"{out.stem}_{i:03d}{out.suffix}")), frame)
        print(f"{out.with_name(out.stem + '_000' + out.suffix)} .. : {n} frames of {screen.width}x{screen.height}, constant "
              f"{tuple(gui.constant)} -> {morph_to}")
    elif args.frames is None:
        write_png(args.out, gs.render())
        print(f"{args.out}: {screen.width}x{screen.height}, kernel {gs.last_kernel_ms():.3f} ms")
    else:
        for k in args.frames:
            gs.set_camera(orbit_camera(w, k))
            path = args.out % k
            write_png(path, gs.render())
            print(f"{path}: frame {k}, kernel {gs.last_kernel_ms():.3f} ms")
