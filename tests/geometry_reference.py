"""Loader of tests/geometry_reference.c: the expected geometry plane of kifs_render_geometry_async from the unmodified
oracle's public pieces.  Compiled on first use with the host compiler and -ffp-contract=off into a temporary
directory, linked against the oracle library the session uses."""
import ctypes as C
import functools
import shutil
import subprocess
import tempfile
from concurrent.futures import ThreadPoolExecutor
from pathlib import Path

import numpy as np

from helpers import oracle_uniforms

SRC = Path(__file__).resolve().parent / "geometry_reference.c"
ORACLE_DIR = Path(__file__).resolve().parent.parent / "oracle"
MISS = np.array([0, 0, 0, 0x7f800000], dtype=np.uint32)  # (0, 0, 0, +inf)


@functools.lru_cache(maxsize=None)
def _load(variant):
    cc = shutil.which("cc") or shutil.which("gcc") or shutil.which("clang")
    assert cc is not None, "no C compiler"
    out = Path(tempfile.mkdtemp(prefix="kifs_geometry_reference_")) / "libgeometry_reference.so"
    flags = ["-O2", "-ffp-contract=off", "-fno-fast-math", "-std=c99", "-shared", "-fPIC", f"-I{ORACLE_DIR}"]
    link = [f"-L{ORACLE_DIR}", f"-l:{variant}", f"-Wl,-rpath,{ORACLE_DIR}", "-lm"]
    # (-march=native: a hardware fmaf where there is one; libm's software fmaf is exact either way)
    p = subprocess.run([cc, *flags, "-march=native", "-o", str(out), str(SRC), *link], capture_output=True, text=True)
    if p.returncode != 0:
        p = subprocess.run([cc, *flags, "-o", str(out), str(SRC), *link], capture_output=True, text=True)
        assert p.returncode == 0, p.stderr
    L = C.CDLL(str(out))
    L.kgr_march_rows.restype = C.c_int
    L.kgr_march_rows.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_void_p,
                                 C.c_void_p]
    L.kgr_colour_from_geometry.restype = None
    L.kgr_colour_from_geometry.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p]
    return L


def library(O):
    return _load(O.lib()._variant)


def march(O, screen, camera, options, it, y0=0, y1=None):
    """(geometry float32 rows x W x 4, hit bool rows x W, loop counter uint16 rows x W) of rows [y0, y1) for oracle
    uniform structs; rows run on a few threads (ctypes releases the GIL)."""
    L = library(O)
    w, h = int(screen.width), int(screen.height)
    y1 = h if y1 is None else y1
    rows = y1 - y0
    geom = np.zeros((rows, w, 4), dtype=np.float32)
    hit = np.zeros((rows, w), dtype=np.uint8)
    steps = np.zeros((rows, w), dtype=np.uint16)

    def chunk(r0):
        r1 = min(r0 + 4, rows)
        rc = L.kgr_march_rows(C.byref(screen), C.byref(camera), C.byref(options), C.byref(it), y0 + r0, y0 + r1,
                              geom[r0:r1].ctypes.data, hit[r0:r1].ctypes.data, steps[r0:r1].ctypes.data)
        assert rc == 0

    with ThreadPoolExecutor(16) as ex:
        list(ex.map(chunk, range(0, rows, 4)))
    return geom, hit.astype(bool), steps


def geometry_frame(O, K, screen, camera, gui, iters, y0=0, y1=None):
    """march() for product-side scene objects (ScreenData, CameraData, GuiData or an OptionsUniform image)."""
    s, c, o = oracle_uniforms(O, K, (screen, camera, gui))
    return march(O, s, c, o, O.iters(*iters), y0, y1)


def colour_from_geometry(O, options, geom, hit):
    """(rows, W, 3) float32: the contract's shading of the texels (no heatmap, no shadows)."""
    L = library(O)
    g = np.ascontiguousarray(geom, dtype=np.float32)
    m = np.ascontiguousarray(hit, dtype=np.uint8)
    rgb = np.zeros(g.shape[:2] + (3,), dtype=np.float32)
    L.kgr_colour_from_geometry(C.byref(options), g.ctypes.data, m.ctypes.data, m.size, rgb.ctypes.data)
    return rgb


def same_bits(a, b):
    """Boolean array: f32 values equal by bit pattern, any NaN equal to any NaN."""
    a = np.ascontiguousarray(a, dtype=np.float32)
    b = np.ascontiguousarray(b, dtype=np.float32)
    return (a.view(np.uint32) == b.view(np.uint32)) | (np.isnan(a) & np.isnan(b))
