"""Loader of tests/occlusion_reference.c: the expected frame and plane of kifs_render_occlusion_async from the unmodified
oracle's public pieces.  Compiled on first use with the host compiler and -ffp-contract=off into a temporary directory,
linked against the oracle library the session uses (as tests/geometry_reference.py)."""
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

SRC = Path(__file__).resolve().parent / "occlusion_reference.c"
ORACLE_DIR = Path(__file__).resolve().parent.parent / "oracle"
DEFAULT = (5, 0.02, 0.75, 4.0)   # the defaults of AmbientOcclusion
DEEP = (16, 0.01, 1.0, 1.0)      # many probes, no decay: clamps creases to 0


class Term(C.Structure):  # KocTerm == KifsAmbientOcclusion
    _fields_ = [("samples", C.c_int32), ("step", C.c_float), ("decay", C.c_float), ("strength", C.c_float)]


@functools.lru_cache(maxsize=None)
def _load(variant):
    cc = shutil.which("cc") or shutil.which("gcc") or shutil.which("clang")
    assert cc is not None, "no C compiler"
    out = Path(tempfile.mkdtemp(prefix="kifs_occlusion_reference_")) / "libocclusion_reference.so"
    flags = ["-O2", "-ffp-contract=off", "-fno-fast-math", "-std=c99", "-shared", "-fPIC", f"-I{ORACLE_DIR}"]
    link = [f"-L{ORACLE_DIR}", f"-l:{variant}", f"-Wl,-rpath,{ORACLE_DIR}", "-lm"]
    # (-march=native: a hardware fmaf where there is one; libm's software fmaf is exact either way)
    p = subprocess.run([cc, *flags, "-march=native", "-o", str(out), str(SRC), *link], capture_output=True, text=True)
    if p.returncode != 0:
        p = subprocess.run([cc, *flags, "-o", str(out), str(SRC), *link], capture_output=True, text=True)
        assert p.returncode == 0, p.stderr
    L = C.CDLL(str(out))
    L.koc_factor.restype = C.c_float
    L.koc_factor.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
    L.koc_march_rows.restype = C.c_int
    L.koc_march_rows.argtypes = [C.c_void_p] * 6 + [C.c_int, C.c_int] + [C.c_void_p] * 5
    L.koc_encode.restype = None
    L.koc_encode.argtypes = [C.c_void_p, C.c_size_t, C.c_int, C.c_void_p]
    return L


def library(O):
    return _load(O.lib()._variant)


def term(ao):
    return ao if isinstance(ao, Term) else Term(int(ao[0]), float(ao[1]), float(ao[2]), float(ao[3]))


def factor(O, options, it, ao, p, n):
    """The factor of one hit: p and n are three floats each."""
    pp = (C.c_float * 3)(*[float(v) for v in p])
    nn = (C.c_float * 3)(*[float(v) for v in n])
    t = term(ao)
    return np.float32(library(O).koc_factor(C.byref(options), C.byref(it), C.byref(t), pp, nn))


class Frame:
    """What the model holds of rows [y0, y1): rgb (rows, W, 3) float32 linear, plane (rows, W) float32, hit (rows, W) bool,
    normal and pos (rows, W, 3) float32."""

    def __init__(self, rgb, plane, hit, normal, pos):
        self.rgb, self.plane, self.hit, self.normal, self.pos = rgb, plane, hit, normal, pos


def march(O, screen, camera, options, it, ao, ext=None, y0=0, y1=None):
    """Frame of rows [y0, y1) for oracle uniform structs (`screen` may be a virtual screen); rows run on a few threads
    (ctypes releases the GIL)."""
    L = library(O)
    w, h = int(screen.width), int(screen.height)
    y1 = h if y1 is None else y1
    rows = y1 - y0
    rgb = np.zeros((rows, w, 3), dtype=np.float32)
    plane = np.zeros((rows, w), dtype=np.float32)
    hit = np.zeros((rows, w), dtype=np.uint8)
    normal = np.zeros((rows, w, 3), dtype=np.float32)
    pos = np.zeros((rows, w, 3), dtype=np.float32)
    t = term(ao)
    e = C.byref(ext) if ext is not None else None

    def chunk(r0):
        r1 = min(r0 + 4, rows)
        rc = L.koc_march_rows(C.byref(screen), C.byref(camera), C.byref(options), C.byref(it), e, C.byref(t), y0 + r0, y0 + r1,
                              rgb[r0:r1].ctypes.data, plane[r0:r1].ctypes.data, hit[r0:r1].ctypes.data,
                              normal[r0:r1].ctypes.data, pos[r0:r1].ctypes.data)
        assert rc == 0

    with ThreadPoolExecutor(16) as ex:
        list(ex.map(chunk, range(0, rows, 4)))
    return Frame(rgb, plane, hit.astype(bool), normal, pos)


def encode(O, rgb, encode_mode):
    """(rows, W, 3) float32 linear -> (rows, W, 4) uint8 through kor_encode_channel, alpha 255."""
    c = np.ascontiguousarray(rgb, dtype=np.float32)
    out = np.zeros(c.shape[:2] + (4,), dtype=np.uint8)
    library(O).koc_encode(c.ctypes.data, c.shape[0] * c.shape[1], int(encode_mode), out.ctypes.data)
    return out


def occlusion_frame(O, K, screen, camera, gui, iters, ao, ext=None, y0=0, y1=None):
    """march() for product-side scene objects (ScreenData, CameraData, GuiData or an OptionsUniform image)."""
    s, c, o = oracle_uniforms(O, K, (screen, camera, gui))
    return march(O, s, c, o, O.iters(*iters), ao, ext, y0, y1)


def supersampled_bytes(O, K, screen, camera, gui, iters, ao, k, encode_mode=1, ext=None):
    """The expected bytes at supersampling factor k: the modelled samples of the virtual screen k W x k H, resolved in
    np.float32 in the contract's order (tests/aa_reference.py) and encoded."""
    s, c, o = oracle_uniforms(O, K, (screen, camera, gui))
    samples = march(O, AA.virtual_screen(O, s, k), c, o, O.iters(*iters), ao, ext)
    return encode(O, AA.resolve(samples.rgb, k), encode_mode)


def same_bits(a, b):
    """Boolean array: f32 values equal by bit pattern, any NaN equal to any NaN."""
    a = np.ascontiguousarray(a, dtype=np.float32)
    b = np.ascontiguousarray(b, dtype=np.float32)
    return (a.view(np.uint32) == b.view(np.uint32)) | (np.isnan(a) & np.isnan(b))
