"""The BASELINE.json workloads as scene descriptions (synthetic, deterministic).

Common settings: camera distance 5, phi = theta = 0
(CameraData::default, data.rs:105-113), max_distance 1000, epsilon 1e-4, fractal colour
sRGB 200 via the reference's /256 conversion, black background, sRGB colour target.
`iters` = (sdf_iters, normal_iters, fold_iters); the reference constants are (100, 10, 10).
"""
import math
from dataclasses import dataclass, field, replace

import numpy as np

from .graphics import CameraData, FractalGroup, GuiData, PrimitiveShape, ScreenData

JULIA_C = (-0.2, 0.6, 0.2, 0.2)  # (real, i, j, k) of BASELINE configs 1, 2, 4


@dataclass
class Workload:
    name: str
    screen: ScreenData
    gui: GuiData
    iters: tuple
    camera: CameraData = field(default_factory=CameraData)
    frames: int = 1
    gpus: int = 1
    extensions: dict = None  # keyword arguments of GraphicState.set_extensions (soft shadows)

    @property
    def pixels(self):
        return self.screen.width * self.screen.height


def _julia(max_iterations, c=JULIA_C):
    return GuiData(max_iterations=max_iterations, fractal_group=FractalGroup.JuliaSet, constant=c)


def _sierpinski(max_iterations):
    return GuiData(max_iterations=max_iterations, fractal_group=FractalGroup.KaleidoscopicIFS,
                   primitive_shape=PrimitiveShape.SierpinskiTetrahedron)


WORKLOADS = {
    # configs[0]: the reference's own CPU-runnable plumbing case
    "cfg1_julia_256": Workload("256x256 quaternion-Julia, 64 steps, 8 SDF iters",
                               ScreenData(256, 256), _julia(64), (8, 10, 10)),
    # configs[1]: the headline metric
    "cfg2_julia_1080p": Workload("1920x1080 quaternion-Julia, 256 steps, 12 SDF iters",
                                 ScreenData(1920, 1080), _julia(256), (12, 10, 10)),
    "cfg3_sierpinski_1080p": Workload("1920x1080 KIFS Sierpinski, 16 folds, 256 steps",
                                      ScreenData(1920, 1080), _sierpinski(256), (100, 10, 16)),
    "cfg4_julia_4096": Workload("4096x4096 quaternion-Julia, 512 steps, 16 SDF iters",
                                ScreenData(4096, 4096), _julia(512), (16, 10, 10), gpus=8),
    # configs[4] without the soft-shadow extension (absent from the reference)
    "cfg5_sierpinski_8k_orbit": Workload("7680x4320 KIFS Sierpinski orbit, 16 folds, 256 steps",
                                         ScreenData(7680, 4320), _sierpinski(256), (100, 10, 16),
                                         camera=CameraData(origin_distance=3.0, theta=0.3),
                                         frames=120, gpus=8),
    # configs[4] with the soft-shadow extension switched on (no reference counterpart)
    "cfg5_sierpinski_8k_orbit_shadows": Workload(
        "7680x4320 KIFS Sierpinski orbit, 16 folds, 256 steps, soft-shadow secondary rays",
        ScreenData(7680, 4320), _sierpinski(256), (100, 10, 16),
        camera=CameraData(origin_distance=3.0, theta=0.3), frames=120, gpus=8,
        extensions=dict(soft_shadow=True, shadow_steps=64, shadow_k=8.0, shadow_t0=0.02, shadow_max_t=10.0)),
    # the reference exactly as shipped: GUI-default constant, hard-coded iteration counts
    "ref_julia_1080p": Workload("1920x1080 Julia, reference constants (100/10), GUI default c",
                                ScreenData(1920, 1080),
                                _julia(256, c=(-0.1, 0.6, 0.9, -0.3)), (100, 10, 10)),
    # the reference's third pipeline and its last primitive
    "n1_genjulia_1080p": Workload("1920x1080 generalised Julia, power 8, reference constants (100/10)",
                                  ScreenData(1920, 1080),
                                  GuiData(max_iterations=256, fractal_group=FractalGroup.GeneralizedJuliaSet,
                                          power=8.0, constant=(-0.1, 0.6, 0.9, -0.3)), (100, 10, 10)),
    "n2_bunny_1080p": Workload("1920x1080 KIFS bunny (neural SDF), 256 steps",
                               ScreenData(1920, 1080),
                               GuiData(max_iterations=256, fractal_group=FractalGroup.KaleidoscopicIFS,
                                       primitive_shape=PrimitiveShape.Bunny), (100, 10, 10)),
}

HEADLINE = "cfg2_julia_1080p"


def orbit_camera(workload: Workload, frame: int) -> CameraData:
    """Frame k of the cfg-5 orbit: phi_k = 2*pi*k/frames, fixed theta and distance."""
    base = workload.camera
    frames = max(workload.frames, 120)
    return CameraData(origin_distance=base.origin_distance, min_distance=base.min_distance,
                      phi=2.0 * math.pi * frame / frames, theta=base.theta)


# what the frames of one animated launch must share (kifs_render_animation_async: one pipeline, one march budget)
MORPH_FIXED = ("max_iterations", "max_distance", "epsilon", "is_heatmap", "fractal_group", "primitive_shape")


def morph_options(gui_a: GuiData, gui_b: GuiData, n: int) -> list:
    """The `n` option sets of a morph from `gui_a` to `gui_b` for GraphicState.render_animation: frame i has
    constant and power a + (b - a) * t_i, t_i = i / (n - 1), every operation in f32 (the difference, t_i, the product,
    the sum); frame 0 is a's values exactly and frame n - 1 b's.  The colours are a's.  ValueError when a field the
    frames of one launch must share differs between the two."""
    if n < 1:
        raise ValueError("morph_options: at least one frame")
    for name in MORPH_FIXED:
        if getattr(gui_a, name) != getattr(gui_b, name):
            raise ValueError(f"morph_options: {name} may not vary within a sequence "
                             f"({getattr(gui_a, name)!r} against {getattr(gui_b, name)!r})")
    f32 = np.float32
    a = np.array(tuple(gui_a.constant) + (gui_a.power,), dtype=f32)
    b = np.array(tuple(gui_b.constant) + (gui_b.power,), dtype=f32)
    frames = []
    for i in range(n):
        if i == 0:
            v = a
        elif i == n - 1:
            v = b
        else:
            t = f32(i) / f32(n - 1)
            v = a + (b - a) * t
        frames.append(replace(gui_a, constant=tuple(float(x) for x in v[:4]), power=float(v[4])))
    return frames


def shutter_cameras(workload_or_orbit, frame: int, samples: int, shutter: float = 0.5) -> list:
    """The `samples` sub-frame cameras of orbit frame `frame` for GraphicState.render_accumulate (motion blur): the
    shutter is open for `shutter` x the angle between two frames of the orbit, centred on the frame, and sub-frame s
    sits in the middle of the s-th of `samples` equal parts of that interval:
        phi_s = phi + step * ((s + 0.5) / samples - 0.5),  phi = f32(2 pi frame / frames),  step = f32(shutter) * f32(2 pi / frames),
    every operation after those roundings in f32.  One sample is orbit_camera(frame)'s f32 angle itself, whatever the
    shutter.  `workload_or_orbit`: a Workload (its camera and max(frames, 120) frames per turn, as orbit_camera) or a
    (CameraData, frames per turn) pair."""
    if samples < 1:
        raise ValueError("shutter_cameras: at least one sub-frame")
    if isinstance(workload_or_orbit, Workload):
        base, frames = workload_or_orbit.camera, max(workload_or_orbit.frames, 120)
    else:
        base, frames = workload_or_orbit
    f32 = np.float32
    phi = f32(2.0 * math.pi * frame / frames)
    step = f32(shutter) * f32(2.0 * math.pi / frames)
    cams = []
    for s in range(samples):
        t = (f32(s) + f32(0.5)) / f32(samples) - f32(0.5)
        cams.append(CameraData(origin_distance=base.origin_distance, min_distance=base.min_distance,
                               phi=float(phi + step * t), theta=base.theta))
    return cams


LENS_GOLDEN_ANGLE = math.pi * (3.0 - math.sqrt(5.0))  # the turn between two points of lens_points


def lens_points(aperture: float, samples: int) -> np.ndarray:
    """The fixed point set of lens_cameras, (samples, 2) float32 offsets (a, b) in the lens plane: Vogel's spiral over
    the disc of radius `aperture` -- point s at radius aperture * sqrt(s / samples) and angle s * LENS_GOLDEN_ANGLE
    (radius and angle in f64, the offsets r cos, r sin rounded to f32).  Point 0 is the lens' centre: the pinhole."""
    pts = np.zeros((samples, 2), dtype=np.float32)
    for s in range(samples):
        r, a = aperture * math.sqrt(s / samples), s * LENS_GOLDEN_ANGLE
        pts[s] = (r * math.cos(a), r * math.sin(a))
    return pts


def lens_cameras(camera_data: CameraData, aperture: float, focus_distance: float, samples: int):
    """The `samples` sub-frame cameras of a thin lens for GraphicState.render_accumulate (depth of field), as a C array
    of raw CameraUniform images (graphics.camera_array takes it as it is).  With the pinhole image's origin o and
    matrix columns m0, m1, m2 (pixel (ux, uy) looks along ux m1 - uy m2 - m0: entry.wgsl:49-59), sub-frame s moves the
    origin by lens_points' (a, b) in the lens plane and re-aims the forward axis at the focus point:
        o_s = o + (a m1 + b m2),   m0_s = m0 + (a m1 + b m2) / focus_distance,   m1, m2 unchanged,
    every operation in f32, the sum in brackets first.  Every pixel's ray then still passes through the point the
    pinhole's ray reaches on the plane `focus_distance` in front of the camera: that plane stays sharp, everything else
    is spread over the lens.  (m0_s is deliberately not renormalised: the shear is what keeps the plane of focus a plane.)
    Sub-frame 0 is the pinhole image itself."""
    from .graphics import CameraUniform
    if samples < 1 or not focus_distance > 0.0:
        raise ValueError("lens_cameras: at least one sub-frame and a positive focus distance")
    f32 = np.float32
    base = camera_data.into_buffer_data() if hasattr(camera_data, "into_buffer_data") else camera_data
    o = np.array(base.origin[:], dtype=f32)
    m = [np.array(base.matrix[c][:3], dtype=f32) for c in range(3)]
    out = (CameraUniform * samples)()
    for s, (a, b) in enumerate(lens_points(aperture, samples)):
        shift = a * m[1] + b * m[2]
        o_s, m0_s = o + shift, m[0] + shift / f32(focus_distance)
        u = out[s]
        u.origin[:] = [float(v) for v in o_s]
        for c, col in enumerate((m0_s, m[1], m[2])):
            u.matrix[c][:] = [float(v) for v in col] + [0.0]
    return out


def light_direction(azimuth: float, elevation: float) -> tuple:
    """The unit vector towards a light at `azimuth` (radians about the z axis, from +x towards +y) and `elevation`
    (radians above the xy plane): a direction for Light / KifsLight."""
    ce = math.cos(elevation)
    v = np.array([ce * math.cos(azimuth), ce * math.sin(azimuth), math.sin(elevation)], dtype=np.float64)
    v = v / np.linalg.norm(v)
    return (float(v[0]), float(v[1]), float(v[2]))


def trap_range(lo: float, hi: float) -> tuple:
    """(scale, bias) for OrbitTrap / KifsOrbitTrap that put u = lo at t = 0 and u = hi at t = 1, as np.float32:
    scale = 1 / (hi - lo) and bias = -lo * scale, each operation in f32.  hi < lo inverts the gradient."""
    lo, hi = np.float32(lo), np.float32(hi)
    if not (np.isfinite(lo) and np.isfinite(hi)) or lo == hi:
        raise ValueError("trap_range: two different finite distances")
    scale = np.float32(np.float32(1.0) / np.float32(hi - lo))
    return scale, np.float32(np.float32(-lo) * scale)


def fold_rotation(*axis_angle_pairs) -> tuple:
    """The row-major 3 x 3 matrix for FoldSystem.rotation / KifsFoldSystem.rotation of a chain of axis rotations:
    fold_rotation(("y", 0.4), ("z", -0.2)) is R_y(0.4) R_z(-0.2) -- the last pair turns the point first.  An axis is
    "x", "y", "z" or 0, 1, 2, an angle is in radians.  Every factor is the library's kifs_host_rotation_matrix and every
    product its kifs_host_mat3_mul (f32, column-major); the result is transposed to the row-major order the record
    takes.  No pair: the identity."""
    import ctypes as C

    from ._lib import lib
    m = (C.c_float * 9)(1.0, 0.0, 0.0, 0.0, 1.0, 0.0, 0.0, 0.0, 1.0)
    for pair in axis_angle_pairs:
        axis, angle = pair
        index = {"x": 0, "y": 1, "z": 2}.get(axis, axis) if isinstance(axis, str) else axis
        if index not in (0, 1, 2):
            raise ValueError(f"fold_rotation: axis {axis!r} is not x, y, z or 0, 1, 2")
        if not math.isfinite(float(angle)):
            raise ValueError("fold_rotation: a finite angle in radians")
        r, out = (C.c_float * 9)(), (C.c_float * 9)()
        lib.kifs_host_rotation_matrix(int(index), float(angle), r)
        lib.kifs_host_mat3_mul(m, r, out)
        m = out
    return tuple(float(m[3 * c + r]) for r in range(3) for c in range(3))


def _fold_presets():
    from .graphics import FoldSystem
    return {
        # the Menger sponge: sort the folded point, scale by 3 about the corner, mirror z about its half offset
        "menger": (PrimitiveShape.Box, FoldSystem(stages=("abs", "sort", "mirror_z"), iterations=4, scale=3.0, offset=(1.0, 1.0, 1.0))),
        # an octahedral flake of boxes, turned a little every round
        "flake": (PrimitiveShape.Box, FoldSystem(stages=("abs", "sort", "rotate"), iterations=6, scale=2.0, offset=(1.0, 0.0, 0.0),
                                                 rotation=fold_rotation(("z", 0.25), ("y", 0.15)))),
        # a rotated tetrahedral flake of tori
        "tetra": (PrimitiveShape.Torus, FoldSystem(stages=("tetra", "rotate"), iterations=5, scale=2.0, offset=(1.0, 1.0, 1.0),
                                                   rotation=fold_rotation(("z", 0.3), ("x", 0.2)))),
    }


# name -> (base PrimitiveShape, FoldSystem)
FOLD_PRESETS = _fold_presets()


def pass_splits(total: int, per_pass: int = 64) -> list:
    """The pass sizes of a progressive frame of `total` sub-frames (GraphicState.render_accumulate_resume, Accumulator):
    total // per_pass passes of `per_pass` and, if anything is left, one of the remainder -- [64, 64, 22] for 150.  A
    pass holds at most MAX_ACCUMULATE = 64 sub-frames.  (shutter_cameras and lens_cameras take any number of samples: the
    cameras of a frame are made once for `total` and handed out pass by pass; jitter_cells gives at most g^2 distinct
    cells, so the passes of a frame take jitter_cells(g, n, frame=first sub-frame of the pass), which walks on through
    the grid and round again.)"""
    if total < 1 or not 1 <= per_pass <= 64:
        raise ValueError("pass_splits: at least one sub-frame, 1..64 per pass")
    return [per_pass] * (total // per_pass) + ([total % per_pass] if total % per_pass else [])


def grid_cells(g: int) -> list:
    """The g^2 cells (i, j) of the g x g grid inside a pixel in supersampling order, j outer and i inner: what
    GraphicState.render_accumulate(jitter=(g, None)) takes for samples = g^2."""
    if g < 1:
        raise ValueError("grid_cells: a grid of at least one cell")
    return [(n % g, n // g) for n in range(g * g)]


def jitter_stride(g: int) -> int:
    """The smallest integer >= 0.618 g^2 that is coprime to g^2: the step of jitter_cells through the numbered cells."""
    n = g * g
    a = math.ceil(0.618 * n)
    while math.gcd(a, n) != 1:
        a += 1
    return a


def jitter_cells(g: int, samples: int, frame: int = 0) -> list:
    """`samples` <= g^2 distinct cells (i, j) of the g x g grid for the sub-frames of output frame `frame`
    (GraphicState.render_accumulate's jitter): with the cells numbered n = j g + i, sub-frame s takes
    n_s = ((s + frame) * a) mod g^2, a = jitter_stride(g).  a is coprime to g^2, so the cells are distinct and
    samples == g^2 uses every cell exactly once; a step of about 0.618 of the grid keeps a sub-frame's cell unrelated to
    its time within the shutter interval or its place on the lens."""
    if g < 1:
        raise ValueError("jitter_cells: a grid of at least one cell")
    n = g * g
    if not 0 <= samples <= n:
        raise ValueError(f"jitter_cells: at most {n} distinct cells in a {g} x {g} grid, {samples} asked for")
    a = jitter_stride(g)
    return [((((s + frame) * a) % n) % g, (((s + frame) * a) % n) // g) for s in range(samples)]


# ---- rays for GraphicState.trace_rays (kifs_trace_rays_async) ------------------------------------------------------
def _fma32(a, b, c):
    """fma(a, b, c) of float32 arrays, correctly rounded, for ordinary magnitudes: the product is exact in f64, the sum is
    rounded to odd there (its rounding error from the two-sum), and 53 bits rounded to odd round to 24 as the exact value."""
    p = a.astype(np.float64) * b.astype(np.float64)
    c = np.asarray(c, dtype=np.float64)
    s = p + c
    bb = s - p
    err = (p - (s - bb)) + (c - bb)                      # exact: p + c = s + err
    bits = s.view(np.int64).copy()
    inexact = err != 0.0
    towards_zero = inexact & ((err < 0.0) == (s > 0.0))  # the exact value lies between s and zero: truncate
    bits -= towards_zero.astype(np.int64)                # (sign-magnitude: one less is one step towards zero)
    bits |= inexact.astype(np.int64)
    return bits.view(np.float64).astype(np.float32)


def pixel_rays(screen, camera) -> np.ndarray:
    """The (H * W, 8) float32 rays of a frame in KifsRay layout, row by row: the origin is the camera's and the direction
    of pixel (x, y) is, bit for bit, ray_direction of kifs_scene.hpp (entry.wgsl:49-59) -- the same f32 operations in
    the same order: px = x + 0.5, uv.x = (2 px) / height - aspect, uv.y = (2 py) / height - 1 (divisions by the height,
    no reciprocal), d = (uv.x m1 - uv.y m2) - m0 per component, l = sqrt(fma(d.z, d.z, fma(d.y, d.y, d.x d.x))), d / l.
    `screen`: ScreenData or a ScreenUniform image; `camera`: CameraData or a CameraUniform image (a raw one may be
    sheared, as lens_cameras' are)."""
    f32 = np.float32
    s = screen.into_buffer_data() if hasattr(screen, "into_buffer_data") else screen
    c = camera.into_buffer_data() if hasattr(camera, "into_buffer_data") else camera
    w, h = int(s.width), int(s.height)
    height, aspect = f32(s.height), f32(s.aspect_ratio)
    o = np.array(c.origin[:], dtype=f32)
    m0, m1, m2 = (np.array(c.matrix[k][:3], dtype=f32) for k in range(3))
    px = np.arange(w, dtype=f32) + f32(0.5)
    py = np.arange(h, dtype=f32) + f32(0.5)
    uvx = np.broadcast_to(((f32(2.0) * px) / height - aspect)[None, :], (h, w))
    uvy = np.broadcast_to(((f32(2.0) * py) / height - f32(1.0))[:, None], (h, w))
    d = [(uvx * m1[k] - uvy * m2[k]) - m0[k] for k in range(3)]
    length = np.sqrt(_fma32(d[2], d[2], _fma32(d[1], d[1], d[0] * d[0])))
    rays = np.zeros((h * w, 8), dtype=f32)
    rays[:, 0:3] = o
    for k in range(3):
        rays[:, 4 + k] = (d[k] / length).reshape(-1)
    return rays


def panorama_rays(origin, width: int, height: int) -> np.ndarray:
    """The (height * width, 8) float32 rays of an equirectangular picture seen from `origin`, row by row: longitude runs
    over the columns and latitude over the rows, z is up (the axis the orbit camera turns about).  Pixel (i, j) looks along
        lon = 2 pi (i + 0.5) / width - pi,   lat = pi / 2 - pi (j + 0.5) / height,
        d = (cos lat cos lon, cos lat sin lon, sin lat),
    computed in f64 and rounded to f32 (unit to rounding).  Data, not contract: any set of rays is as good."""
    if width < 1 or height < 1:
        raise ValueError("panorama_rays: at least one column and one row")
    lon = 2.0 * math.pi * (np.arange(width, dtype=np.float64) + 0.5) / width - math.pi
    lat = math.pi / 2.0 - math.pi * (np.arange(height, dtype=np.float64) + 0.5) / height
    cl = np.cos(lat)[:, None]
    rays = np.zeros((height * width, 8), dtype=np.float32)
    rays[:, 0:3] = np.asarray(origin, dtype=np.float32)
    rays[:, 4] = (cl * np.cos(lon)[None, :]).reshape(-1)
    rays[:, 5] = (cl * np.sin(lon)[None, :]).reshape(-1)
    rays[:, 6] = np.broadcast_to(np.sin(lat)[:, None], (height, width)).reshape(-1)
    return rays
