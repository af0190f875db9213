"""Loader of tests/fold_reference.c: the expected frame of kifs_render_folded_async and the expected values of
kifs_eval_fold from the unmodified oracle's public pieces.  Compiled on first use with the host compiler and
-ffp-contract=off into a temporary directory, linked against the oracle library the session uses (as
tests/trap_reference.py).  Also the fold systems and scenes the fold tests share."""
import ctypes as C
import functools
import math
import shutil
import subprocess
import tempfile
from concurrent.futures import ThreadPoolExecutor
from pathlib import Path

import numpy as np

import aa_reference as AA
import lighting_reference as LR
from helpers import oracle_uniforms

SRC = Path(__file__).resolve().parent / "fold_reference.c"
ORACLE_DIR = Path(__file__).resolve().parent.parent / "oracle"
f32 = np.float32

ABS, SORT, TETRA, ROTATE, MIRROR_Z = 1, 2, 4, 8, 16
IDENTITY = (1.0, 0.0, 0.0, 0.0, 1.0, 0.0, 0.0, 0.0, 1.0)


class FoldC(C.Structure):  # KfrFold == KifsFoldSystem
    _fields_ = [("stages", C.c_uint32), ("iterations", C.c_int32), ("scale", C.c_float), ("offset", C.c_float * 3),
                ("rotation", C.c_float * 9)]


def make_fold(stages=0, iterations=0, scale=2.0, offset=(1.0, 1.0, 1.0), rotation=IDENTITY):
    return FoldC(int(stages), int(iterations), float(scale), (C.c_float * 3)(*[float(v) for v in offset]),
                 (C.c_float * 9)(*[float(v) for v in rotation]))


def fold(spec):
    return spec if isinstance(spec, FoldC) else make_fold(**spec)


def rot(axis, angle):
    """Row-major rotation about a coordinate axis by `angle` radians, entries rounded to f32 (test data: the matrix is
    used as given, so any finite matrix does)."""
    c, s = math.cos(angle), math.sin(angle)
    m = {"x": (1, 0, 0, 0, c, -s, 0, s, c), "y": (c, 0, s, 0, 1, 0, -s, 0, c), "z": (c, -s, 0, s, c, 0, 0, 0, 1)}[axis]
    return tuple(float(f32(v)) for v in m)


def rot2(a, b):
    """Row-major product a b of two row-major matrices, entries rounded to f32."""
    A, B = np.array(a, dtype=np.float64).reshape(3, 3), np.array(b, dtype=np.float64).reshape(3, 3)
    return tuple(float(f32(v)) for v in (A @ B).reshape(-1))


# The named test systems, each with the scene of tests/geometry_cases.py it is rendered on (its natural base).
MENGER = dict(stages=ABS | SORT | MIRROR_Z, iterations=3, scale=3.0, offset=(1.0, 1.0, 1.0))
FLAKE = dict(stages=ABS | ROTATE, iterations=4, scale=1.8, offset=(1.0, 1.0, 0.5), rotation=rot("y", 0.4))
TETRA_TORUS = dict(stages=TETRA | ROTATE, iterations=4, scale=2.0, offset=(1.0, 1.0, 1.0), rotation=rot2(rot("z", 0.3), rot("x", 0.2)))
TETRA_SPHERE = dict(stages=TETRA, iterations=5, scale=2.0, offset=(1.0, 1.0, 1.0))
# name -> (base scene, system, camera).  NEAR is the `near` camera of tests/geometry_cases.py, (3.5, 0.6, 0.5), moved to
# distance 2.6.  From outside, the sponge's silhouette is the box's -- its tunnels run along the axes and a perspective
# view from 2.6 sees through none of them -- so the Menger system's frame is taken from INSIDE its central chamber, where
# the solid box is hit everywhere and the sponge shows its tunnels' mouths; "menger_near" is the outside view, whose hit
# pattern equals the box's and whose shading does not.
NEAR = dict(origin_distance=2.6, phi=0.6, theta=0.5)
CHAMBER = dict(origin_distance=0.3, phi=0.3, theta=0.15)
NAMED = {"menger": ("box", MENGER, CHAMBER), "menger_near": ("box", MENGER, NEAR), "flake": ("box", FLAKE, NEAR),
         "tetra_torus": ("torus", TETRA_TORUS, NEAR), "tetra_sphere": ("sphere", TETRA_SPHERE, NEAR)}
# All five stages at once, N = 3: the system of the every-pipeline test.
ALL_STAGES = dict(stages=31, iterations=3, scale=2.0, offset=(1.0, 0.8, 0.6), rotation=rot2(rot("y", 0.35), rot("z", -0.25)))
# Two balls of radius 0.5 at x = +-1.5, outside the unit sphere's cull radius.  The camera stands on the +x axis 0.2 off
# the near ball, which hides the far one: every hit lies on the near ball's outer cap, |p| >= 1.89, and most of the rays
# that reach it pass the origin at more than the cull radius -- a launch that kept the base's cull drops them.
WIDE = dict(stages=ABS, iterations=1, scale=2.0, offset=(3.0, 0.0, 0.0))
WIDE_CAMERA = dict(origin_distance=2.2, phi=0.0, theta=0.0)


@functools.lru_cache(maxsize=None)
def _load(variant):
    cc = shutil.which("cc") or shutil.which("gcc") or shutil.which("clang")
    assert cc is not None, "no C compiler"
    out = Path(tempfile.mkdtemp(prefix="kifs_fold_reference_")) / "libfold_reference.so"
    flags = ["-O2", "-ffp-contract=off", "-fno-fast-math", "-std=c99", "-shared", "-fPIC", f"-I{ORACLE_DIR}"]
    link = [f"-L{ORACLE_DIR}", f"-l:{variant}", f"-Wl,-rpath,{ORACLE_DIR}", "-lm"]
    # (-march=native: a hardware fmaf where there is one; libm's software fmaf is exact either way)
    p = subprocess.run([cc, *flags, "-march=native", "-o", str(out), str(SRC), *link], capture_output=True, text=True)
    if p.returncode != 0:
        p = subprocess.run([cc, *flags, "-o", str(out), str(SRC), *link], capture_output=True, text=True)
        assert p.returncode == 0, p.stderr
    L = C.CDLL(str(out))
    L.kfr_constants.restype = None
    L.kfr_constants.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p]
    L.kfr_fold_point.restype = None
    L.kfr_fold_point.argtypes = [C.c_void_p] * 5
    L.kfr_sdf.restype = C.c_float
    L.kfr_sdf.argtypes = [C.c_void_p] * 4
    L.kfr_eval_many.restype = None
    L.kfr_eval_many.argtypes = [C.c_void_p] * 4 + [C.c_int, C.c_void_p, C.c_void_p]
    L.kfr_march_rows.restype = C.c_int
    L.kfr_march_rows.argtypes = [C.c_void_p] * 8 + [C.c_int, C.c_int] + [C.c_void_p] * 3
    L.kfr_encode.restype = None
    L.kfr_encode.argtypes = [C.c_void_p, C.c_size_t, C.c_int, C.c_void_p]
    return L


def library(O):
    return _load(O.lib()._variant)


def constants(O, spec):
    """(t, h) as the host side computes them."""
    t = (C.c_float * 3)()
    h = C.c_float()
    f = fold(spec)
    library(O).kfr_constants(C.byref(f), t, C.byref(h))
    return np.array(list(t), dtype=f32), f32(h.value)


def fold_point(O, options, spec, p):
    """(folded point, acc) of one position."""
    q = (C.c_float * 3)()
    acc = C.c_float()
    f = fold(spec)
    library(O).kfr_fold_point(C.byref(options), C.byref(f), (C.c_float * 3)(*[float(v) for v in p]), q, C.byref(acc))
    return np.array(list(q), dtype=f32), f32(acc.value)


def eval_points(O, options, it, spec, points, sdf=True, normal=True):
    """(sdf (n,), normal (n, 3)) float32 of (n, 3) float32 positions; None for what is not asked for."""
    pts = np.ascontiguousarray(points, dtype=np.float32).reshape(-1, 3)
    n = len(pts)
    s = np.zeros(n, dtype=np.float32) if sdf else None
    nr = np.zeros((n, 3), dtype=np.float32) if normal else None
    f = fold(spec)
    L = library(O)

    def chunk(i0):
        i1 = min(i0 + 128, n)
        L.kfr_eval_many(C.byref(options), C.byref(it), C.byref(f), pts[i0:i1].ctypes.data, i1 - i0,
                        s[i0:i1].ctypes.data if sdf else None, nr[i0:i1].ctypes.data if normal else None)

    with ThreadPoolExecutor(16) as ex:
        list(ex.map(chunk, range(0, n, 128)))
    return s, nr


class Frame:
    """What the model holds of rows [y0, y1): rgb (rows, W, 3) float32 linear, hit (rows, W) bool, pos (rows, W, 3)
    float32."""

    def __init__(self, rgb, hit, pos):
        self.rgb, self.hit, self.pos = rgb, hit, pos


def march(O, screen, camera, options, it, spec, light=None, ao=None, ext=None, y0=0, y1=None):
    """Frame of rows [y0, y1) for oracle uniform structs (`screen` may be a virtual screen); `light` None: the
    reference's light.  Rows run on a few threads (ctypes releases the GIL)."""
    L = library(O)
    w, h = int(screen.width), int(screen.height)
    y1 = h if y1 is None else y1
    rows = y1 - y0
    rgb = np.zeros((rows, w, 3), dtype=np.float32)
    hit = np.zeros((rows, w), dtype=np.uint8)
    pos = np.zeros((rows, w, 3), dtype=np.float32)
    f = fold(spec)
    l = None if light is None else LR.light(light)
    t = LR.term(ao)
    e = C.byref(ext) if ext is not None else None
    lp = C.byref(l) if l is not None else None
    a = C.byref(t) if t is not None else None

    def chunk(r0):
        r1 = min(r0 + 2, rows)
        rc = L.kfr_march_rows(C.byref(screen), C.byref(camera), C.byref(options), C.byref(it), e, C.byref(f), lp, a, y0 + r0,
                              y0 + r1, rgb[r0:r1].ctypes.data, hit[r0:r1].ctypes.data, pos[r0:r1].ctypes.data)
        assert rc == 0

    with ThreadPoolExecutor(16) as ex:
        list(ex.map(chunk, range(0, rows, 2)))
    return Frame(rgb, hit.astype(bool), pos)


def encode(O, rgb, encode_mode):
    """(rows, W, 3) float32 linear -> (rows, W, 4) uint8 through kor_encode_channel, alpha 255."""
    c = np.ascontiguousarray(rgb, dtype=np.float32)
    out = np.zeros(c.shape[:2] + (4,), dtype=np.uint8)
    library(O).kfr_encode(c.ctypes.data, c.shape[0] * c.shape[1], int(encode_mode), out.ctypes.data)
    return out


def folded_frame(O, K, screen, camera, gui, iters, spec, light=None, ao=None, ext=None, y0=0, y1=None):
    """march() for product-side scene objects (ScreenData, CameraData, GuiData or an OptionsUniform image)."""
    s, c, o = oracle_uniforms(O, K, (screen, camera, gui))
    return march(O, s, c, o, O.iters(*iters), spec, light, ao, ext, y0, y1)


def supersampled_bytes(O, K, screen, camera, gui, iters, spec, k, light=None, ao=None, encode_mode=1, ext=None):
    """The expected bytes at supersampling factor k: the modelled samples of the virtual screen k W x k H, resolved in
    np.float32 in the contract's order (tests/aa_reference.py) and encoded."""
    s, c, o = oracle_uniforms(O, K, (screen, camera, gui))
    samples = march(O, AA.virtual_screen(O, s, k), c, o, O.iters(*iters), spec, light, ao, ext)
    return encode(O, AA.resolve(samples.rgb, k), encode_mode)


def named_scene(K, cases, name, width, height):
    """(scene, system) of a named test system: its base's scene with the system's camera."""
    base, spec, cam = NAMED[name]
    screen, _, gui, iters = cases(K, width, height)[base]
    return (screen, K.CameraData(**cam), gui, iters), spec


def wide_scene(K, cases, width, height):
    screen, _, gui, iters = cases(K, width, height)["sphere"]
    return (screen, K.CameraData(**WIDE_CAMERA), gui, iters), WIDE


def closest_approach(origin, points):
    """Distance from the coordinate origin of the lines from `origin` through each of `points`, f64."""
    o = np.asarray(origin, dtype=np.float64)
    d = np.asarray(points, dtype=np.float64) - o
    d = d / np.linalg.norm(d, axis=1, keepdims=True)
    return np.linalg.norm(np.cross(np.broadcast_to(o, d.shape), d), axis=1)


same_bits = LR.same_bits
