"""Loader of tests/trap_reference.c: the expected frame of kifs_render_trapped_async and the expected u of kifs_eval_trap
from the unmodified oracle's public pieces.  Compiled on first use with the host compiler and -ffp-contract=off into a
temporary directory, linked against the oracle library the session uses (as tests/lighting_reference.py)."""
import ctypes as C
import functools
import shutil
import subprocess
import tempfile
from concurrent.futures import ThreadPoolExecutor
from pathlib import Path

import numpy as np

import aa_reference as AA
import lighting_reference as LR
from helpers import oracle_uniforms

SRC = Path(__file__).resolve().parent / "trap_reference.c"
ORACLE_DIR = Path(__file__).resolve().parent.parent / "oracle"
f32 = np.float32


class TrapC(C.Structure):  # KtrTrap == KifsOrbitTrap
    _fields_ = [("centre", C.c_float * 4), ("axes", C.c_uint32), ("iterations", C.c_int32), ("scale", C.c_float),
                ("bias", C.c_float), ("mid", C.c_float * 3), ("far", C.c_float * 3)]


def trap_range(lo, hi):
    """(scale, bias) that map u = lo to t = 0 and u = hi to t = 1: scale = 1 / (hi - lo), bias = -lo * scale, each
    operation in f32."""
    lo, hi = f32(lo), f32(hi)
    scale = f32(f32(1.0) / f32(hi - lo))
    return scale, f32(f32(-lo) * scale)


# The stops of the test traps, linear RGB: an orange and a blue.
MID = (1.0, 0.2622507, 0.0)
FAR = (0.0069954, 0.0451862, 0.5775804)


def make_trap(centre=(0.0, 0.0, 0.0, 0.0), axes=15, iterations=8, scale=0.0, bias=0.0, mid=MID, far=FAR):
    return TrapC((C.c_float * 4)(*[float(v) for v in centre]), int(axes), int(iterations), float(scale), float(bias),
                 (C.c_float * 3)(*[float(v) for v in mid]), (C.c_float * 3)(*[float(v) for v in far]))


def _ranged(lo, hi, **kw):
    s, b = trap_range(lo, hi)
    return dict(kw, scale=float(s), bias=float(b), mid=MID, far=FAR)


# The two test traps: J for the Julia groups (a point trap at the origin of orbit space, eight orbit points), S for the
# KIFS group (the corner (1,1,1) of the tetrahedron in x, y, z, six folds).
J = _ranged(0.3, 0.9, centre=(0.0, 0.0, 0.0, 0.0), axes=15, iterations=8)
S = _ranged(0.0, 2.0, centre=(1.0, 1.0, 1.0, 0.0), axes=7, iterations=6)


def for_scene(name):
    """The test trap of a scene of geometry_cases: J for the two Julia groups, S for the KIFS group."""
    return J if name in ("julia_24", "julia_25", "genjulia") else S


def trap(spec):
    return spec if isinstance(spec, TrapC) else make_trap(**spec)


@functools.lru_cache(maxsize=None)
def _load(variant):
    cc = shutil.which("cc") or shutil.which("gcc") or shutil.which("clang")
    assert cc is not None, "no C compiler"
    out = Path(tempfile.mkdtemp(prefix="kifs_trap_reference_")) / "libtrap_reference.so"
    flags = ["-O2", "-ffp-contract=off", "-fno-fast-math", "-std=c99", "-shared", "-fPIC", f"-I{ORACLE_DIR}"]
    link = [f"-L{ORACLE_DIR}", f"-l:{variant}", f"-Wl,-rpath,{ORACLE_DIR}", "-lm"]
    # (-march=native: a hardware fmaf where there is one; libm's software fmaf is exact either way)
    p = subprocess.run([cc, *flags, "-march=native", "-o", str(out), str(SRC), *link], capture_output=True, text=True)
    if p.returncode != 0:
        p = subprocess.run([cc, *flags, "-o", str(out), str(SRC), *link], capture_output=True, text=True)
        assert p.returncode == 0, p.stderr
    L = C.CDLL(str(out))
    L.ktr_trap_u.restype = C.c_float
    L.ktr_trap_u.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p]
    L.ktr_trap_u_many.restype = None
    L.ktr_trap_u_many.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p]
    L.ktr_colour.restype = C.c_float
    L.ktr_colour.argtypes = [C.c_void_p, C.c_void_p, C.c_float, C.c_void_p]
    L.ktr_march_rows.restype = C.c_int
    L.ktr_march_rows.argtypes = [C.c_void_p] * 8 + [C.c_int, C.c_int] + [C.c_void_p] * 4
    L.ktr_encode.restype = None
    L.ktr_encode.argtypes = [C.c_void_p, C.c_size_t, C.c_int, C.c_void_p]
    return L


def library(O):
    return _load(O.lib()._variant)


def eval_u(O, options, spec, points):
    """u of (n, 3) float32 positions for an oracle Options struct: (n,) float32."""
    pts = np.ascontiguousarray(points, dtype=np.float32).reshape(-1, 3)
    u = np.zeros(len(pts), dtype=np.float32)
    t = trap(spec)
    library(O).ktr_trap_u_many(C.byref(options), C.byref(t), pts.ctypes.data, len(pts), u.ctypes.data)
    return u


def colour(O, options, spec, u):
    """(t, col) of the gradient at u."""
    col = (C.c_float * 3)()
    t = trap(spec)
    tt = library(O).ktr_colour(C.byref(options), C.byref(t), float(u), col)
    return np.float32(tt), np.array(list(col), dtype=np.float32)


class Frame:
    """What the model holds of rows [y0, y1): rgb (rows, W, 3) float32 linear, hit (rows, W) bool, pos (rows, W, 3)
    float32, and per pixel u and t (rows, W) float32 (0 off the surface and in heatmap mode)."""

    def __init__(self, rgb, hit, pos, ut):
        self.rgb, self.hit, self.pos = rgb, hit, pos
        self.u, self.t = ut[..., 0], ut[..., 1]


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
    ut = np.zeros((rows, w, 2), dtype=np.float32)
    tr = trap(spec)
    l = None if light is None else LR.light(light)
    t = LR.term(ao)
    e = C.byref(ext) if ext is not None else None
    lp = C.byref(l) if l is not None else None
    a = C.byref(t) if t is not None else None

    def chunk(r0):
        r1 = min(r0 + 4, rows)
        rc = L.ktr_march_rows(C.byref(screen), C.byref(camera), C.byref(options), C.byref(it), e, C.byref(tr), lp, a, y0 + r0,
                              y0 + r1, rgb[r0:r1].ctypes.data, hit[r0:r1].ctypes.data, pos[r0:r1].ctypes.data,
                              ut[r0:r1].ctypes.data)
        assert rc == 0

    with ThreadPoolExecutor(16) as ex:
        list(ex.map(chunk, range(0, rows, 4)))
    return Frame(rgb, hit.astype(bool), pos, ut)


def encode(O, rgb, encode_mode):
    """(rows, W, 3) float32 linear -> (rows, W, 4) uint8 through kor_encode_channel, alpha 255."""
    c = np.ascontiguousarray(rgb, dtype=np.float32)
    out = np.zeros(c.shape[:2] + (4,), dtype=np.uint8)
    library(O).ktr_encode(c.ctypes.data, c.shape[0] * c.shape[1], int(encode_mode), out.ctypes.data)
    return out


def trapped_frame(O, K, screen, camera, gui, iters, spec, light=None, ao=None, ext=None, y0=0, y1=None):
    """march() for product-side scene objects (ScreenData, CameraData, GuiData or an OptionsUniform image)."""
    s, c, o = oracle_uniforms(O, K, (screen, camera, gui))
    return march(O, s, c, o, O.iters(*iters), spec, light, ao, ext, y0, y1)


def supersampled_bytes(O, K, screen, camera, gui, iters, spec, k, light=None, ao=None, encode_mode=1, ext=None):
    """The expected bytes at supersampling factor k: the modelled samples of the virtual screen k W x k H, resolved in
    np.float32 in the contract's order (tests/aa_reference.py) and encoded."""
    s, c, o = oracle_uniforms(O, K, (screen, camera, gui))
    samples = march(O, AA.virtual_screen(O, s, k), c, o, O.iters(*iters), spec, light, ao, ext)
    return encode(O, AA.resolve(samples.rgb, k), encode_mode)


same_bits = LR.same_bits
