"""Loader of tests/ray_reference.c: the expected output of kifs_trace_rays_async from the unmodified oracle's public
pieces.  Compiled on first use with the host compiler and -ffp-contract=off into a temporary directory, linked against
the oracle library the session uses (as tests/geometry_reference.py builds its file)."""
import ctypes as C
import functools
import shutil
import subprocess
import tempfile
from concurrent.futures import ThreadPoolExecutor
from pathlib import Path

import numpy as np

from helpers import oracle_uniforms

SRC = Path(__file__).resolve().parent / "ray_reference.c"
ORACLE_DIR = Path(__file__).resolve().parent.parent / "oracle"
MISS = np.array([0, 0, 0, 0x7f800000], dtype=np.uint32)  # (0, 0, 0, +inf)


@functools.lru_cache(maxsize=None)
def _load(variant):
    cc = shutil.which("cc") or shutil.which("gcc") or shutil.which("clang")
    assert cc is not None, "no C compiler"
    out = Path(tempfile.mkdtemp(prefix="kifs_ray_reference_")) / "libray_reference.so"
    flags = ["-O2", "-ffp-contract=off", "-fno-fast-math", "-std=c99", "-shared", "-fPIC", f"-I{ORACLE_DIR}"]
    link = [f"-L{ORACLE_DIR}", f"-l:{variant}", f"-Wl,-rpath,{ORACLE_DIR}", "-lm"]
    # (-march=native: a hardware fmaf where there is one; libm's software fmaf is exact either way)
    p = subprocess.run([cc, *flags, "-march=native", "-o", str(out), str(SRC), *link], capture_output=True, text=True)
    if p.returncode != 0:
        p = subprocess.run([cc, *flags, "-o", str(out), str(SRC), *link], capture_output=True, text=True)
        assert p.returncode == 0, p.stderr
    L = C.CDLL(str(out))
    L.krr_trace.restype = C.c_int
    L.krr_trace.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_size_t, C.c_void_p, C.c_void_p, C.c_void_p]
    return L


def trace(O, options, it, rays, encode=1):
    """(geometry float32 n x 4, rgba uint8 n x 4, loop counter uint16 n) of the (n, 8) float32 rays for oracle uniform
    structs; chunks of rays run on a few threads (ctypes releases the GIL)."""
    L = _load(O.lib()._variant)
    rays = np.ascontiguousarray(rays, dtype=np.float32)
    assert rays.ndim == 2 and rays.shape[1] == 8
    n = rays.shape[0]
    geom = np.zeros((n, 4), dtype=np.float32)
    rgba = np.zeros((n, 4), dtype=np.uint8)
    steps = np.zeros(n, dtype=np.uint16)
    step = 128

    def chunk(k0):
        k1 = min(k0 + step, n)
        rc = L.krr_trace(C.byref(options), C.byref(it), encode, rays[k0:k1].ctypes.data, k1 - k0, geom[k0:k1].ctypes.data,
                         rgba[k0:k1].ctypes.data, steps[k0:k1].ctypes.data)
        assert rc == 0

    with ThreadPoolExecutor(16) as ex:
        list(ex.map(chunk, range(0, n, step)))
    return geom, rgba, steps


def trace_scene(O, K, gui, iters, rays, encode=1, heatmap=None):
    """trace() for a product-side GuiData (or an OptionsUniform image); `heatmap` overrides the image's flag."""
    screen, camera = K.ScreenData(8, 8), K.CameraData()
    _, _, o = oracle_uniforms(O, K, (screen, camera, gui))
    if heatmap is not None:
        o.is_heatmap = 1 if heatmap else 0
    return trace(O, o, O.iters(*iters), rays, encode)


def hits(geom):
    """Boolean (n,): the texel is not the miss texel's t."""
    return np.ascontiguousarray(geom, dtype=np.float32).view(np.uint32)[:, 3] != MISS[3]
