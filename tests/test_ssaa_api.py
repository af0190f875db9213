"""k x k supersampled anti-aliasing (kifs_set_supersampling), the parts a machine without a GPU can check: the ABI
surface, argument checking, the Python and CLI surface, and the test suite's own reference resolve."""
import ctypes as C
import re
import subprocess
import sys
from pathlib import Path

import numpy as np
import pytest

import aa_reference as AA
from helpers import oracle_frame

ROOT = Path(__file__).resolve().parent.parent
HEADER = (ROOT / "include" / "kifs_hip.h").read_text()


def test_header_declares_the_supersampling_surface():
    assert re.search(r"^int kifs_set_supersampling\(kifs_ctx\* ctx, int factor\);", HEADER, re.M)
    assert re.search(r"^int kifs_multi_set_supersampling\(kifs_multi\* m, int factor\);", HEADER, re.M)
    assert re.search(r"^#define KIFS_MAX_SUPERSAMPLING 4$", HEADER, re.M)
    assert re.search(r"KIFS_KERNEL_SSAA = 5\b", HEADER)
    assert re.search(r"^#define KIFS_ABI_VERSION 4$", HEADER, re.M)


def test_setters_reject_null_and_bad_factors(kifs):
    from kifs_raymarching_amd._lib import lib
    assert lib.kifs_set_supersampling(None, 2) == 7
    assert lib.kifs_multi_set_supersampling(None, 2) == 7
    assert lib.kifs_set_supersampling(None, 1) == 7


def test_python_surface(kifs):
    assert callable(getattr(kifs.GraphicState, "set_supersampling", None))
    assert callable(getattr(kifs.MultiGraphicState, "set_supersampling", None))
    assert kifs.GraphicState.KERNEL_NAMES[5] == "render_ssaa_kernel"


def test_render_tool_offers_aa(kifs):
    p = subprocess.run([sys.executable, str(ROOT / "tools" / "render.py"), "--help"], capture_output=True, text=True,
                       timeout=120)
    assert p.returncode == 0, p.stderr
    assert "--aa" in p.stdout


def test_resolve_order_is_the_contracts():
    """j outer, i inner, f32 throughout: a case where the order matters in the last bit."""
    k = 2
    lin = np.zeros((2, 2, 3), dtype=np.float32)
    lin[0, 0], lin[0, 1], lin[1, 0], lin[1, 1] = 1.0, 2.0 ** -24, 2.0 ** -24, 0.0  # (j, i) = (0,0) (0,1) (1,0) (1,1)
    got = AA.resolve(lin, k)[0, 0, 0]
    acc = np.float32(1.0)
    for v in (2.0 ** -24, 2.0 ** -24, 0.0):
        acc = np.float32(acc + np.float32(v))
    assert got == np.float32(acc / np.float32(4.0))


@pytest.mark.parametrize("scene", ["julia", "sierpinski"])
@pytest.mark.parametrize("encode", [1, 0])
def test_reference_resolve_at_k1_is_the_oracle_frame(kifs, oracle, scene, encode):
    """The suite's own reference: at k = 1 its resolve of the per-pixel linear colours equals oracle.render."""
    from kifs_raymarching_amd.configs import JULIA_C
    screen = kifs.ScreenData(48, 30)
    cam = kifs.CameraData(origin_distance=3.0, phi=0.4, theta=0.2)
    if scene == "julia":
        gui = kifs.GuiData(max_iterations=64, fractal_group=kifs.FractalGroup.JuliaSet, constant=JULIA_C)
        iters = (12, 10, 10)
    else:
        gui = kifs.GuiData(primitive_shape=kifs.PrimitiveShape.SierpinskiTetrahedron, background_color=(10, 40, 90))
        iters = (100, 10, 10)
    want = oracle_frame(oracle, kifs, screen, cam, gui, iters, encode=encode)
    got = AA.aa_frame(oracle, kifs, screen, cam, gui, iters, 1, encode)
    assert got.shape == want.shape and (got == want).all()
    assert (want[..., :3] != want[0, 0, :3]).any()
