"""Loader of tests/lighting_reference.c: the expected frame of kifs_render_lit_async from the unmodified oracle's public
pieces.  Compiled on first use with the host compiler and -ffp-contract=off into a temporary directory, linked against the
oracle library the session uses (as tests/occlusion_reference.py)."""
import ctypes as C
import functools
import shutil
import subprocess
import tempfile
from concurrent.futures import ThreadPoolExecutor
from pathlib import Path

import numpy as np

import aa_reference as AA
from helpers import oracle_uniforms

SRC = Path(__file__).resolve().parent / "lighting_reference.c"
ORACLE_DIR = Path(__file__).resolve().parent.parent / "oracle"


class LightC(C.Structure):  # KlrLight == KifsLight
    _fields_ = [("direction", C.c_float * 3), ("ambient", C.c_float), ("diffuse", C.c_float), ("specular", C.c_float * 3),
                ("shininess_log2", C.c_int32)]


class Term(C.Structure):  # KlrTerm == KifsAmbientOcclusion
    _fields_ = [("samples", C.c_int32), ("step", C.c_float), ("decay", C.c_float), ("strength", C.c_float)]


def make_light(direction=(1.0, 1.0, 1.0), ambient=0.1, diffuse=0.9, specular=(0.0, 0.0, 0.0), shininess_log2=5):
    return LightC((C.c_float * 3)(*[float(v) for v in direction]), float(ambient), float(diffuse),
                  (C.c_float * 3)(*[float(v) for v in specular]), int(shininess_log2))


def _unit32(v):
    """normalize((x, y, z)) in f64, rounded to f32: the test light's direction as the issue states it."""
    v = np.asarray(v, dtype=np.float64)
    return tuple(float(x) for x in (v / np.linalg.norm(v)).astype(np.float32))


REFERENCE = dict(direction=(1.0, 1.0, 1.0), ambient=0.1, diffuse=0.9, specular=(0.0, 0.0, 0.0), shininess_log2=5)
A_DIRECTION = _unit32((-0.55, 0.75, 0.36))
# The test light A with its highlight (e = 3), and at e = 5 for the test that runs everything at once.
A = dict(direction=A_DIRECTION, ambient=0.15, diffuse=0.85, specular=(0.6, 0.6, 0.5), shininess_log2=3)
A5 = dict(A, shininess_log2=5)
# A second light from another side, for the restatement's second set of hits.
B = dict(direction=_unit32((0.3, -0.5, 0.8)), ambient=0.05, diffuse=0.7, specular=(0.2, 0.4, 0.9), shininess_log2=5)


def light(spec):
    return spec if isinstance(spec, LightC) else make_light(**spec)


def term(ao):
    if ao is None or isinstance(ao, Term):
        return ao
    return Term(int(ao[0]), float(ao[1]), float(ao[2]), float(ao[3]))


@functools.lru_cache(maxsize=None)
def _load(variant):
    cc = shutil.which("cc") or shutil.which("gcc") or shutil.which("clang")
    assert cc is not None, "no C compiler"
    out = Path(tempfile.mkdtemp(prefix="kifs_lighting_reference_")) / "liblighting_reference.so"
    flags = ["-O2", "-ffp-contract=off", "-fno-fast-math", "-std=c99", "-shared", "-fPIC", f"-I{ORACLE_DIR}"]
    link = [f"-L{ORACLE_DIR}", f"-l:{variant}", f"-Wl,-rpath,{ORACLE_DIR}", "-lm"]
    # (-march=native: a hardware fmaf where there is one; libm's software fmaf is exact either way)
    p = subprocess.run([cc, *flags, "-march=native", "-o", str(out), str(SRC), *link], capture_output=True, text=True)
    if p.returncode != 0:
        p = subprocess.run([cc, *flags, "-o", str(out), str(SRC), *link], capture_output=True, text=True)
        assert p.returncode == 0, p.stderr
    L = C.CDLL(str(out))
    L.klr_unit.restype = None
    L.klr_unit.argtypes = [C.c_void_p, C.c_void_p]
    L.klr_direct.restype = C.c_float
    L.klr_direct.argtypes = [C.c_void_p, C.c_void_p]
    L.klr_highlight.restype = C.c_float
    L.klr_highlight.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p]
    L.klr_march_rows.restype = C.c_int
    L.klr_march_rows.argtypes = [C.c_void_p] * 7 + [C.c_int, C.c_int] + [C.c_void_p] * 5
    L.klr_encode.restype = None
    L.klr_encode.argtypes = [C.c_void_p, C.c_size_t, C.c_int, C.c_void_p]
    return L


def library(O):
    return _load(O.lib()._variant)


def _vec(v):
    return (C.c_float * 3)(*[float(x) for x in v])


def unit(O, spec):
    out = (C.c_float * 3)()
    l = light(spec)
    library(O).klr_unit(C.byref(l), out)
    return np.array(list(out), dtype=np.float32)


def direct(O, spec, n):
    l = light(spec)
    return np.float32(library(O).klr_direct(C.byref(l), _vec(n)))


def highlight(O, spec, n, d):
    l = light(spec)
    return np.float32(library(O).klr_highlight(C.byref(l), _vec(n), _vec(d)))


class Frame:
    """What the model holds of rows [y0, y1): rgb (rows, W, 3) float32 linear, hit (rows, W) bool, normal and pos
    (rows, W, 3) float32, and per pixel lit0, s, sh and a (rows, W) float32."""

    def __init__(self, rgb, hit, normal, pos, terms):
        self.rgb, self.hit, self.normal, self.pos = rgb, hit, normal, pos
        self.lit0, self.s, self.sh, self.a = (terms[..., i] for i in range(4))


def march(O, screen, camera, options, it, spec, ao=None, ext=None, y0=0, y1=None):
    """Frame of rows [y0, y1) for oracle uniform structs (`screen` may be a virtual screen); rows run on a few threads
    (ctypes releases the GIL)."""
    L = library(O)
    w, h = int(screen.width), int(screen.height)
    y1 = h if y1 is None else y1
    rows = y1 - y0
    rgb = np.zeros((rows, w, 3), dtype=np.float32)
    hit = np.zeros((rows, w), dtype=np.uint8)
    normal = np.zeros((rows, w, 3), dtype=np.float32)
    pos = np.zeros((rows, w, 3), dtype=np.float32)
    terms = np.zeros((rows, w, 4), dtype=np.float32)
    l, t = light(spec), term(ao)
    e = C.byref(ext) if ext is not None else None
    a = C.byref(t) if t is not None else None

    def chunk(r0):
        r1 = min(r0 + 4, rows)
        rc = L.klr_march_rows(C.byref(screen), C.byref(camera), C.byref(options), C.byref(it), e, C.byref(l), a, y0 + r0, y0 + r1,
                              rgb[r0:r1].ctypes.data, hit[r0:r1].ctypes.data, normal[r0:r1].ctypes.data,
                              pos[r0:r1].ctypes.data, terms[r0:r1].ctypes.data)
        assert rc == 0

    with ThreadPoolExecutor(16) as ex:
        list(ex.map(chunk, range(0, rows, 4)))
    return Frame(rgb, hit.astype(bool), normal, pos, terms)


def encode(O, rgb, encode_mode):
    """(rows, W, 3) float32 linear -> (rows, W, 4) uint8 through kor_encode_channel, alpha 255."""
    c = np.ascontiguousarray(rgb, dtype=np.float32)
    out = np.zeros(c.shape[:2] + (4,), dtype=np.uint8)
    library(O).klr_encode(c.ctypes.data, c.shape[0] * c.shape[1], int(encode_mode), out.ctypes.data)
    return out


def lit_frame(O, K, screen, camera, gui, iters, spec, ao=None, ext=None, y0=0, y1=None):
    """march() for product-side scene objects (ScreenData, CameraData, GuiData or an OptionsUniform image)."""
    s, c, o = oracle_uniforms(O, K, (screen, camera, gui))
    return march(O, s, c, o, O.iters(*iters), spec, ao, ext, y0, y1)


def supersampled_bytes(O, K, screen, camera, gui, iters, spec, k, ao=None, encode_mode=1, ext=None):
    """The expected bytes at supersampling factor k: the modelled samples of the virtual screen k W x k H, resolved in
    np.float32 in the contract's order (tests/aa_reference.py) and encoded."""
    s, c, o = oracle_uniforms(O, K, (screen, camera, gui))
    samples = march(O, AA.virtual_screen(O, s, k), c, o, O.iters(*iters), spec, ao, ext)
    return encode(O, AA.resolve(samples.rgb, k), encode_mode)


def same_bits(a, b):
    """Boolean array: f32 values equal by bit pattern, any NaN equal to any NaN."""
    a = np.ascontiguousarray(a, dtype=np.float32)
    b = np.ascontiguousarray(b, dtype=np.float32)
    return (a.view(np.uint32) == b.view(np.uint32)) | (np.isnan(a) & np.isnan(b))
