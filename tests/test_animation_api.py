"""Animated batches (kifs_render_animation_async), the parts a machine without a GPU can check: the ABI surface, the
Python and CLI surface, configs.morph_options against a NumPy f32 model, and that hipcc compiled anim::render_kernel
for every pipeline, each instantiation with a claim in the kernel-form table."""
import ctypes as C
import re
import subprocess
import sys
from dataclasses import replace
from pathlib import Path

import numpy as np
import pytest

from kernel_report import kernel_report

ROOT = Path(__file__).resolve().parent.parent
HEADER = (ROOT / "include" / "kifs_hip.h").read_text()


def test_header_declares_the_animation_surface():
    flat = re.sub(r"\s+", " ", re.sub(r"/\*.*?\*/", "", HEADER, flags=re.S))
    assert ("int kifs_render_animation_async(kifs_ctx* ctx, void* hip_stream, int count, const KifsCameraUniform* cameras, "
            "const KifsOptionsUniform* options, uint8_t* const* dev_outs_rgba8, size_t pitch_bytes, int y0, int y1, "
            "int encode);") in flat
    assert re.search(r"KIFS_KERNEL_ANIMATION = 8\b", HEADER)
    assert re.search(r"^#define KIFS_ABI_VERSION 4$", HEADER, re.M)


def test_library_exports_and_python_binds_it(kifs):
    from kifs_raymarching_amd import graphics
    from kifs_raymarching_amd._lib import LIB_PATH, SIGNATURES, lib
    assert hasattr(C.CDLL(str(LIB_PATH)), "kifs_render_animation_async")
    res, args = SIGNATURES["kifs_render_animation_async"]
    assert res is C.c_int and len(args) == 10
    assert lib.kifs_abi_version() == 4
    assert lib.kifs_render_animation_async(None, None, 1, None, None, None, 0, 0, 0, 1) == 7  # BAD_ARG, no crash
    assert callable(getattr(kifs.GraphicState, "render_animation", None))
    assert kifs.GraphicState.KERNEL_NAMES[8] == "render_animation_kernel"
    assert graphics.ANIMATION_RING == int(re.search(r"^#define KIFS_ANIMATION_RING (\d+)$", HEADER, re.M).group(1))
    arr = kifs.options_array([kifs.GuiData(power=3.0), kifs.GuiData(power=4.0).into_buffer_data()])
    assert len(arr) == 2 and arr[0].power == 3.0 and arr[1].power == 4.0 and kifs.options_array(arr) is arr


def test_render_tool_offers_the_morph(kifs):
    p = subprocess.run([sys.executable, str(ROOT / "tools" / "render.py"), "--help"], capture_output=True, text=True,
                       timeout=120)
    assert p.returncode == 0, p.stderr
    assert "--morph-to" in p.stdout and "--frames" in p.stdout


def _model(a, b, n):
    """Frame i of the morph in NumPy f32: a + (b - a) * (i / (n - 1)), every operation rounded to f32; the endpoints are
    the inputs themselves."""
    f32 = np.float32
    a, b = np.asarray(a, dtype=f32), np.asarray(b, dtype=f32)
    rows = []
    for i in range(n):
        if i == 0:
            rows.append(a)
        elif i == n - 1:
            rows.append(b)
        else:
            t = f32(f32(i) / f32(n - 1))
            rows.append((a + ((b - a).astype(f32) * t).astype(f32)).astype(f32))
    return np.stack(rows)


@pytest.mark.parametrize("n", [1, 2, 3, 7, 48])
def test_morph_options_against_the_f32_model(n, kifs):
    from kifs_raymarching_amd.configs import morph_options
    G, FG = kifs.GuiData, kifs.FractalGroup
    a = G(max_iterations=96, fractal_group=FG.GeneralizedJuliaSet, power=2.0, constant=(-0.2, 0.6, 0.2, 0.2),
          fractal_color=(250, 120, 60), background_color=(5, 5, 30))
    b = replace(a, power=8.5, constant=(0.3, 0.1, -0.7, 0.45), fractal_color=(1, 2, 3), background_color=(9, 9, 9))
    got = morph_options(a, b, n)
    assert len(got) == n and all(isinstance(g, G) for g in got)
    want = _model(tuple(a.constant) + (a.power,), tuple(b.constant) + (b.power,), n)
    for i, g in enumerate(got):
        u = g.into_buffer_data()  # what the library receives: f32 images
        have = np.array(list(u.constant) + [u.power], dtype=np.float32)
        assert (have.view(np.uint32) == want[i].view(np.uint32)).all(), (i, have, want[i])
        # the colours come from a; nothing else moves
        assert g.fractal_color == a.fractal_color and g.background_color == a.background_color
        assert replace(g, constant=a.constant, power=a.power) == a
    assert kifs.uniform_bytes(got[0].into_buffer_data()) == kifs.uniform_bytes(a.into_buffer_data())
    if n > 1:
        end = replace(b, fractal_color=a.fractal_color, background_color=a.background_color)
        assert kifs.uniform_bytes(got[-1].into_buffer_data()) == kifs.uniform_bytes(end.into_buffer_data())
    if n > 2:
        assert len({g.constant for g in got}) == n  # a morph that moves


@pytest.mark.parametrize("field, other", [("max_iterations", 97), ("max_distance", 999.0), ("epsilon", 0.0002),
                                          ("is_heatmap", True), ("fractal_group", 1), ("primitive_shape", 3)])
def test_morph_options_refuses_a_field_that_may_not_vary(field, other, kifs):
    from kifs_raymarching_amd.configs import morph_options
    a = kifs.GuiData(max_iterations=96, fractal_group=kifs.FractalGroup.GeneralizedJuliaSet)
    if field == "fractal_group":
        other = kifs.FractalGroup(other)
    if field == "primitive_shape":
        other = kifs.PrimitiveShape(other)
    with pytest.raises(ValueError, match=field):
        morph_options(a, replace(a, **{field: other}), 4)
    with pytest.raises(ValueError):
        morph_options(a, a, 0)
    assert len(morph_options(a, replace(a, power=5.0, fractal_color=(1, 1, 1)), 4)) == 4


def test_every_pipeline_is_compiled_and_claimed_in_the_form_table():
    from geometry_cases import PIPELINES
    names = [n for n in kernel_report() if "kifs::anim::render_kernel<" in n]
    got = sorted(re.search(r"render_kernel<(\d+), (\d+)>", n).groups() for n in names)
    # the ten pipelines of the geometry cases: two Julia variants, the generalised Julia set, six primitives, PRIM_OTHER
    want = sorted([("1", "0"), ("1", "1"), ("2", "0")] + [("0", str(p)) for p in range(7)])
    assert got == want and len(names) == len(PIPELINES) == 10, names
    from kernel_forms import ANIMATION_FORMS
    from test_kernel_form_coverage import RENDER  # the form table's own pattern
    assert all(RENDER.search(n) for n in names) and sorted(names) == sorted(ANIMATION_FORMS)
