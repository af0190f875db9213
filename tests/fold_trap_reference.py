"""Loader of tests/fold_trap_reference.c: the expected frame and plane of kifs_render_folded_trapped_async and the expected
u of kifs_eval_fold_trap from the unmodified oracle's public pieces.  Compiled on first use with the host compiler and
-ffp-contract=off into a temporary directory, linked against the oracle library the session uses (as
tests/fold_reference.py).  Also the named frames the tests share, each with the trap whose range comes from the model's
own u at the frame's hits."""
import ctypes as C
import functools
import shutil
import subprocess
import tempfile
from concurrent.futures import ThreadPoolExecutor
from pathlib import Path

import numpy as np

import aa_reference as AA
import fold_reference as FR
import lighting_reference as LR
import trap_reference as TR
from helpers import oracle_uniforms

SRC = Path(__file__).resolve().parent / "fold_trap_reference.c"
ORACLE_DIR = Path(__file__).resolve().parent.parent / "oracle"
f32 = np.float32

# name -> (the named system of tests/fold_reference.py, the trap without its range): the Menger system from inside its
# chamber with a plane trap (x = 0, three fold points), the flake with a point trap at its scaling's fixed point, the
# tetra torus with a line trap (the z axis: x and y take part).
NAMED = {"menger": ("menger", dict(centre=(0.0, 0.0, 0.0, 0.0), axes=1, iterations=3)),
         "flake": ("flake", dict(centre=(1.0, 1.0, 0.5, 0.0), axes=15, iterations=4)),
         "tetra_torus": ("tetra_torus", dict(centre=(0.0, 0.0, 0.0, 0.0), axes=3, iterations=4))}
# The point trap of the every-pipeline test, K = 8 (five more points than FR.ALL_STAGES has rounds: the Sierpinski base
# continues the orbit), with a fixed range.
POINT8 = dict(centre=(0.0, 0.0, 0.0, 0.0), axes=15, iterations=8, scale=0.5, bias=0.0, mid=TR.MID, far=TR.FAR)


@functools.lru_cache(maxsize=None)
def _load(variant):
    cc = shutil.which("cc") or shutil.which("gcc") or shutil.which("clang")
    assert cc is not None, "no C compiler"
    out = Path(tempfile.mkdtemp(prefix="kifs_fold_trap_reference_")) / "libfold_trap_reference.so"
    flags = ["-O2", "-ffp-contract=off", "-fno-fast-math", "-std=c99", "-shared", "-fPIC", f"-I{ORACLE_DIR}", f"-I{SRC.parent}"]
    link = [f"-L{ORACLE_DIR}", f"-l:{variant}", f"-Wl,-rpath,{ORACLE_DIR}", "-lm"]
    # (-march=native: a hardware fmaf where there is one; libm's software fmaf is exact either way)
    p = subprocess.run([cc, *flags, "-march=native", "-o", str(out), str(SRC), *link], capture_output=True, text=True)
    if p.returncode != 0:
        p = subprocess.run([cc, *flags, "-o", str(out), str(SRC), *link], capture_output=True, text=True)
        assert p.returncode == 0, p.stderr
    L = C.CDLL(str(out))
    L.kft_trap_u.restype = C.c_float
    L.kft_trap_u.argtypes = [C.c_void_p] * 5
    L.kft_trap_u_many.restype = None
    L.kft_trap_u_many.argtypes = [C.c_void_p] * 4 + [C.c_int, C.c_void_p, C.c_void_p]
    L.kft_colour.restype = C.c_float
    L.kft_colour.argtypes = [C.c_void_p, C.c_void_p, C.c_float, C.c_void_p]
    L.kft_march_rows.restype = C.c_int
    L.kft_march_rows.argtypes = [C.c_void_p] * 9 + [C.c_int, C.c_int] + [C.c_void_p] * 4
    return L


def library(O):
    return _load(O.lib()._variant)


def eval_u(O, options, fold, trap, points, info=False):
    """u of (n, 3) float32 positions for an oracle Options struct: (n,) float32; with `info` also an (n, 3) int32 array
    -- where the least distance was attained (0: z_0, 1: a fold point, 2: a base point), whether the stop rule cut the
    orbit, and the fold rounds that ran among those that take part."""
    pts = np.ascontiguousarray(points, dtype=np.float32).reshape(-1, 3)
    u = np.zeros(len(pts), dtype=np.float32)
    inf = np.zeros((len(pts), 3), dtype=np.int32)
    f, t = FR.fold(fold), TR.trap(trap)
    library(O).kft_trap_u_many(C.byref(options), C.byref(f), C.byref(t), pts.ctypes.data, len(pts), u.ctypes.data, inf.ctypes.data)
    return (u, inf) if info else u


class Frame:
    """What the model holds of rows [y0, y1): rgb (rows, W, 3) float32 linear, hit (rows, W) bool, pos (rows, W, 3)
    float32, and the plane u (rows, W) float32: a hit's u, +inf on a miss."""

    def __init__(self, rgb, hit, pos, u):
        self.rgb, self.hit, self.pos, self.u = rgb, hit, pos, u


def march(O, screen, camera, options, it, fold, trap, light=None, ao=None, ext=None, y0=0, y1=None):
    """Frame of rows [y0, y1) for oracle uniform structs (`screen` may be a virtual screen); `light` None: the
    reference's light.  Rows run on a few threads (ctypes releases the GIL)."""
    L = library(O)
    w, h = int(screen.width), int(screen.height)
    y1 = h if y1 is None else y1
    rows = y1 - y0
    rgb = np.zeros((rows, w, 3), dtype=np.float32)
    hit = np.zeros((rows, w), dtype=np.uint8)
    pos = np.zeros((rows, w, 3), dtype=np.float32)
    u = np.zeros((rows, w), dtype=np.float32)
    f, tr = FR.fold(fold), TR.trap(trap)
    l = None if light is None else LR.light(light)
    t = LR.term(ao)
    e = C.byref(ext) if ext is not None else None
    lp = C.byref(l) if l is not None else None
    a = C.byref(t) if t is not None else None

    def chunk(r0):
        r1 = min(r0 + 2, rows)
        rc = L.kft_march_rows(C.byref(screen), C.byref(camera), C.byref(options), C.byref(it), e, C.byref(f), C.byref(tr), lp, a,
                              y0 + r0, y0 + r1, rgb[r0:r1].ctypes.data, hit[r0:r1].ctypes.data, pos[r0:r1].ctypes.data,
                              u[r0:r1].ctypes.data)
        assert rc == 0

    with ThreadPoolExecutor(16) as ex:
        list(ex.map(chunk, range(0, rows, 2)))
    return Frame(rgb, hit.astype(bool), pos, u)


encode = FR.encode


def frame(O, K, screen, camera, gui, iters, fold, trap, light=None, ao=None, ext=None, y0=0, y1=None):
    """march() for product-side scene objects (ScreenData, CameraData, GuiData or an OptionsUniform image)."""
    s, c, o = oracle_uniforms(O, K, (screen, camera, gui))
    return march(O, s, c, o, O.iters(*iters), fold, trap, light, ao, ext, y0, y1)


def supersampled_bytes(O, K, screen, camera, gui, iters, fold, trap, k, light=None, ao=None, encode_mode=1, ext=None):
    """The expected bytes at supersampling factor k: the modelled samples of the virtual screen k W x k H, resolved in
    np.float32 in the contract's order (tests/aa_reference.py) and encoded."""
    s, c, o = oracle_uniforms(O, K, (screen, camera, gui))
    samples = march(O, AA.virtual_screen(O, s, k), c, o, O.iters(*iters), fold, trap, light, ao, ext)
    return encode(O, AA.resolve(samples.rgb, k), encode_mode)


def ranged(trap, u):
    """`trap` with scale and bias that map the 5th percentile of the finite `u` to t = 0 and the 95th to t = 1, and the
    test stops: both segments of the gradient are used."""
    v = np.asarray(u, dtype=np.float64)
    v = v[np.isfinite(v)]
    lo, hi = np.percentile(v, 5), np.percentile(v, 95)
    assert hi > lo
    s, b = TR.trap_range(lo, hi)
    return dict(trap, scale=float(s), bias=float(b), mid=TR.MID, far=TR.FAR)


@functools.lru_cache(maxsize=None)
def _named(O, K, cases, name, width, height):
    system, trap = NAMED[name]
    scene, fold = FR.named_scene(K, cases, system, width, height)
    screen, cam, gui, iters = scene
    probe = frame(O, K, screen, cam, gui, iters, fold, dict(trap, scale=0.0, bias=0.0, mid=TR.MID, far=TR.FAR))
    return scene, fold, ranged(trap, probe.u[probe.hit])


def named_scene(O, K, cases, name, width, height):
    """(scene, system, trap) of a named test frame; the trap's range is the 5th..95th percentile of the model's own u at
    the frame's hits."""
    return _named(O, K, cases, name, width, height)


same_bits = LR.same_bits


# ---- the evaluation cases of kifs_eval_fold_trap that the CPU guards and the GPU test share
EVAL_PIPELINES = ["sphere", "sierpinski", "bunny"]
EVAL_N = (0, 1, 7, 24)
EVAL_K = (0, 1, 8, 32)   # with EVAL_N: K < N, K = N and K > N
# Three stage masks.  Scale 3 with a small max_distance lets the stop rule cut orbits.
EVAL_SYSTEMS = [dict(stages=FR.ABS | FR.SORT | FR.MIRROR_Z, scale=3.0, offset=(1.0, 1.0, 1.0)),
                dict(stages=FR.TETRA | FR.ROTATE, scale=2.0, offset=(1.0, 1.0, 1.0), rotation=FR.TETRA_TORUS["rotation"]),
                dict(FR.ALL_STAGES, scale=1.7)]
# Three trap kinds: a point, a line (x and z take part) and a plane (y alone).
EVAL_TRAPS = [dict(centre=(0.5, 0.5, 0.5, 0.0), axes=15), dict(centre=(1.0, 0.0, -0.5, 0.0), axes=5), dict(centre=(0.0, 0.75, 0.0, 0.0), axes=2)]
EVAL_MAX_DISTANCE = 6.0
EVAL_POINTS = 2048


def eval_points(name):
    """The 2048 seeded positions of a pipeline's evaluation cases, inside |p| < 2.5."""
    rng = np.random.default_rng([0xf01d7a9, EVAL_PIPELINES.index(name)])
    v = rng.normal(size=(EVAL_POINTS, 3))
    return (v / np.linalg.norm(v, axis=1, keepdims=True) * (2.5 * rng.uniform(0.0, 1.0, (EVAL_POINTS, 1)) ** (1.0 / 3.0))).astype(np.float32)


def eval_scene(K, cases, name):
    """The pipeline's scene of tests/geometry_cases.py with the evaluation cases' max_distance."""
    screen, cam, gui, iters = cases(K, 102, 45)[name]
    return screen, cam, K.GuiData(**{**gui.__dict__, "max_distance": EVAL_MAX_DISTANCE}), iters


def eval_cases():
    """(fold, trap) of every evaluation case of a pipeline."""
    for N in EVAL_N:
        for Kt in EVAL_K:
            for system in EVAL_SYSTEMS:
                for trap in EVAL_TRAPS:
                    yield dict(system, iterations=N), dict(trap, iterations=Kt, scale=0.0, bias=0.0, mid=TR.MID, far=TR.FAR)
