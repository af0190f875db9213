"""Orbit-trap colouring (kifs_render_trapped_async, kifs_eval_trap), the parts a machine without a GPU can check: the
header's text, the struct's layout against the header, the kernel argument's size, the ctypes binding, the Python layer's
validation and its feeding of the library 64 frames at a time (with a fake library), configs.trap_range in f32, the
refusals that need no device, and that hipcc compiled trap::render_kernel for every pipeline without scratch memory."""
import ctypes as C
import inspect
import re
import subprocess
from pathlib import Path

import numpy as np
import pytest

import trap_reference as TR
from kernel_report import kernel_report

ROOT = Path(__file__).resolve().parent.parent
HEADER = (ROOT / "include" / "kifs_hip.h").read_text()
BAD_ARG = 7


def test_header_declares_the_trapped_surface():
    flat = re.sub(r"\s+", " ", re.sub(r"/\*.*?\*/", "", HEADER, flags=re.S))
    assert ("int kifs_render_trapped_async(kifs_ctx* ctx, void* hip_stream, int count, const KifsCameraUniform* cameras, "
            "uint8_t* const* dev_outs_rgba8, size_t pitch_bytes, const KifsOrbitTrap* trap, const KifsLight* light , "
            "const KifsAmbientOcclusion* ao , int y0, int y1, int encode);") in flat
    assert "int kifs_eval_trap(kifs_ctx* ctx, const KifsOrbitTrap* trap, const float* points_xyz, int n, float* u_out);" in flat
    assert ("typedef struct KifsOrbitTrap { float centre[4]; uint32_t axes; int32_t iterations; float scale, bias; float mid[3]; "
            "float far[3]; } KifsOrbitTrap;") in flat
    assert re.search(r"^#define KIFS_MAX_TRAP_ITERATIONS 32$", HEADER, re.M)
    assert re.search(r"^#define KIFS_MAX_TRAP_BATCH 64$", HEADER, re.M)
    assert re.search(r"^#define KIFS_ABI_VERSION 4$", HEADER, re.M)
    block = HEADER[HEADER.index("extension: orbit-trap surface colouring"):HEADER.index("#define KIFS_MAX_TRAP_ITERATIONS")]
    assert HEADER.index("extension: a configurable light") < HEADER.index("extension: orbit-trap surface colouring")  # after the lit call
    for word in ("orbit", "distance", "gradient", "shading", "identity", "refusals", "scope"):  # the contract's paragraphs
        assert re.search(rf"^ \*   {word}\b", block, re.M), word
    for text in ("fma(e_i, e_i, d)", "(d(z_k) < m) ? d(z_k) : m", "fma(scale, u, bias)", "fma(f, s_{j+1} - s_j, s_j)", "(a) scale = bias = 0",
                 "(b) mid = far = fractal_color", "tests/trap_reference.c", "a plane of u", "more than three stops", "per-frame traps"):
        assert text in block, text


def test_struct_layout_in_c(tmp_path):
    src = tmp_path / "t.c"
    fields = ("centre", "axes", "iterations", "scale", "bias", "mid", "far")
    src.write_text('#include "kifs_hip.h"\n#include <stdio.h>\n#include <stddef.h>\n'
                   'int main(void){printf("%zu", sizeof(KifsOrbitTrap));'
                   + "".join(f'printf(" %zu", offsetof(KifsOrbitTrap, {f}));' for f in fields) + 'printf("\\n");return 0;}\n')
    exe = tmp_path / "t"
    subprocess.run(["gcc", "-std=c99", "-Wall", "-Werror", "-pedantic", f"-I{ROOT / 'include'}", str(src), "-o", str(exe)], check=True)
    out = [int(v) for v in subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.split()]
    assert out == [56, 0, 16, 20, 24, 28, 32, 44]
    from kifs_raymarching_amd._lib import KifsOrbitTrapC
    assert C.sizeof(KifsOrbitTrapC) == 56 and C.sizeof(TR.TrapC) == 56
    assert [getattr(KifsOrbitTrapC, f).offset for f in fields] == out[1:] == [getattr(TR.TrapC, f).offset for f in fields]


def test_kernel_argument_fits(tmp_path):
    """trap::Params is light::Params and the 56-byte record behind it: 4024 + 56 = 4080 of the 4096 bytes a kernel
    argument may have, the light, the term and its flag at light::Params' offsets."""
    src = tmp_path / "t.cpp"
    src.write_text('#include <cstddef>\n#include <cstdint>\n#include <cstdio>\n#include "kifs_params.hpp"\n'
                   'using namespace kifs;\n'
                   'int main(){std::printf("%zu %zu %zu %zu %zu %zu %zu %zu %zu\\n", sizeof(light::Params), sizeof(trap::Trap), sizeof(trap::Params),'
                   'offsetof(light::Params, light), offsetof(trap::Params, light), offsetof(light::Params, has_ao), offsetof(trap::Params, has_ao),'
                   'offsetof(trap::Params, trap), sizeof(trap::EvalParams));}\n')
    exe = tmp_path / "t"
    subprocess.run(["g++", "-std=c++17", "-Wno-invalid-offsetof", f"-I{ROOT / 'kifs_raymarching_amd' / 'csrc'}", str(src), "-o", str(exe)], check=True)
    lit, trap, params, l0, l1, a0, a1, t1, ev = (int(v) for v in subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.split())
    assert (lit, trap, params) == (4024, 56, 4080) and l0 == l1 and a0 == a1 and t1 == 4024 and ev <= 4096


def test_library_exports_and_python_binds_it(kifs):
    from kifs_raymarching_amd import _lib
    from kifs_raymarching_amd._lib import LIB_PATH, SIGNATURES, AmbientOcclusionC, KifsLightC, KifsOrbitTrapC, lib
    raw = C.CDLL(str(LIB_PATH))
    assert hasattr(raw, "kifs_render_trapped_async") and hasattr(raw, "kifs_eval_trap")
    res, args = SIGNATURES["kifs_render_trapped_async"]
    assert res is C.c_int and len(args) == 12
    assert args[6] is C.POINTER(KifsOrbitTrapC) and args[7] is C.POINTER(KifsLightC) and args[8] is C.POINTER(AmbientOcclusionC)
    assert args[9:] == [C.c_int, C.c_int, C.c_int]
    res, args = SIGNATURES["kifs_eval_trap"]
    assert res is C.c_int and len(args) == 5 and args[1] is C.POINTER(KifsOrbitTrapC) and args[3] is C.c_int
    assert (_lib.MAX_TRAP_ITERATIONS, _lib.MAX_TRAP_BATCH) == (32, 64)
    assert lib.kifs_abi_version() == 4
    assert len(kifs.GraphicState.KERNEL_NAMES) == 10  # not a feedback launch: no new KifsKernel value
    assert "OrbitTrap" in kifs.__all__
    sig = inspect.signature(kifs.GraphicState.render_trapped_batch)
    assert list(sig.parameters)[:5] == ["self", "cameras", "trap", "light", "ao"]
    assert sig.parameters["light"].default is None and sig.parameters["ao"].default is None
    sig = inspect.signature(kifs.GraphicState.render_trapped)
    assert list(sig.parameters)[:4] == ["self", "trap", "light", "ao"]
    assert list(inspect.signature(kifs.GraphicState.eval_trap).parameters) == ["self", "trap", "points"]


def test_orbit_trap_converts_its_colours_as_the_options_do(kifs):
    t = kifs.OrbitTrap(centre=(0.5, -1, 2, 0.25), axes=9, iterations=32, scale=2.5, bias=-0.5, mid=(255, 140, 0), far=(20, 60, 200))
    u = t.into_buffer_data()
    o = kifs.GuiData(fractal_color=(255, 140, 0), background_color=(20, 60, 200)).into_buffer_data()
    assert list(u.mid) == list(o.fractal_color) and list(u.far) == list(o.background_color)
    assert (list(u.centre), u.axes, u.iterations, u.scale, u.bias) == ([0.5, -1.0, 2.0, 0.25], 9, 32, 2.5, -0.5)
    d = kifs.OrbitTrap()
    assert (tuple(d.centre), d.axes, d.iterations) == ((0.0, 0.0, 0.0, 0.0), 15, 8)
    nan, inf = float("nan"), float("inf")
    for bad in (dict(centre=(0, 0, 0)), dict(centre=(0, nan, 0, 0)), dict(centre=(inf, 0, 0, 0)), dict(axes=0), dict(axes=16), dict(axes=1.5),
                dict(iterations=-1), dict(iterations=33), dict(iterations=2.5), dict(scale=nan), dict(scale=1e39), dict(bias=-inf),
                dict(mid=(0, 0)), dict(mid=(0, 0, 256)), dict(far=(-1, 0, 0)), dict(far=(0.5, 0, 0))):
        with pytest.raises(ValueError):
            kifs.OrbitTrap(**bad).into_buffer_data()
    for good in (dict(axes=1), dict(axes=15), dict(iterations=0), dict(scale=-3.0), dict(bias=7.0), dict(mid=(0, 0, 0), far=(255, 255, 255))):
        kifs.OrbitTrap(**good).into_buffer_data()


class _FakeLibrary:
    """kifs_render_trapped_async recorded, everything else the real library's."""

    def __init__(self, real):
        self.real, self.calls = real, []

    def __getattr__(self, name):
        return getattr(self.real, name)

    def kifs_destroy(self, ctx):  # (the object under test holds no context of the real library's)
        assert ctx == 0x1234

    def kifs_render_trapped_async(self, ctx, stream, count, cams, outs, pitch, trap, light, ao, y0, y1, encode):
        views = None if cams is None else [bytes(memoryview(cams[i]).cast("B")) for i in range(count)]
        self.calls.append(dict(ctx=ctx, stream=stream, count=count, cams=views, outs=[int(outs[i]) for i in range(count)], pitch=pitch,
                               trap=bytes(memoryview(trap._obj).cast("B")), light=None if light is None else bytes(memoryview(light._obj).cast("B")),
                               ao=None if ao is None else bytes(memoryview(ao._obj).cast("B")), band=(y0, y1), encode=encode))
        return 0


def test_the_python_layer_validates_and_feeds_the_library_64_at_a_time(kifs, monkeypatch):
    import torch
    from kifs_raymarching_amd import graphics
    fake = _FakeLibrary(graphics.lib)
    monkeypatch.setattr(graphics, "lib", fake)
    g = object.__new__(kifs.GraphicState)  # no device: the launches go to the fake
    g._ctx, g.device, g.screen_data = 0x1234, 0, kifs.ScreenData(10, 6)
    cams = [kifs.CameraData(origin_distance=3.0 + 0.01 * i, phi=0.1 * i) for i in range(150)]
    colour = torch.zeros((150, 6, 10, 4), dtype=torch.uint8)
    trap = kifs.OrbitTrap(axes=7, iterations=6)
    light = kifs.Light(direction=(0.0, 1.0, 0.5), ambient=0.2)
    ao = kifs.AmbientOcclusion(samples=3)
    assert g.render_trapped_batch(cams, trap, light=light, ao=ao, colour=colour, encode=0) is colour
    assert [c["count"] for c in fake.calls] == [64, 64, 22]
    base = colour.data_ptr()
    images = [kifs.uniform_bytes(c.into_buffer_data()) for c in cams]
    first = 0
    for c in fake.calls:
        assert c["outs"] == [base + (first + i) * 240 for i in range(c["count"])] and c["cams"] == images[first:first + c["count"]]
        assert c["ctx"] == 0x1234 and c["stream"] is None and c["pitch"] == 40 and c["band"] == (0, 6) and c["encode"] == 0
        assert c["trap"] == kifs.uniform_bytes(trap.into_buffer_data()) and c["light"] == kifs.uniform_bytes(light.into_buffer_data())
        assert c["ao"] == kifs.uniform_bytes(ao.into_buffer_data())
        first += c["count"]
    # no light, no term, a band, the context's camera
    fake.calls.clear()
    band = torch.zeros((1, 2, 10, 4), dtype=torch.uint8)
    g.render_trapped_batch(None, trap, colour=band, y0=3, y1=5)
    assert len(fake.calls) == 1
    c = fake.calls[0]
    assert c["count"] == 1 and c["cams"] is None and c["light"] is None and c["ao"] is None and c["band"] == (3, 5) and c["encode"] == 1
    # refused before the library is asked
    fake.calls.clear()
    with pytest.raises(ValueError):
        g.render_trapped_batch([], trap, colour=colour)
    with pytest.raises(ValueError):
        g.render_trapped_batch(cams, trap, colour=colour[:149])
    with pytest.raises(ValueError):
        g.render_trapped_batch(cams, trap, colour=colour.to(torch.int8))
    with pytest.raises(ValueError):
        g.render_trapped_batch(cams, kifs.OrbitTrap(axes=0), colour=colour)
    with pytest.raises(ValueError):
        g.render_trapped_batch(cams, kifs.OrbitTrap(iterations=33), colour=colour)
    assert fake.calls == []
    g._ctx = None  # (nothing to destroy)


def test_trap_range_in_f32(kifs):
    from kifs_raymarching_amd.configs import trap_range
    f32 = np.float32
    for lo, hi in ((0.3, 0.9), (0.0, 2.0), (0.1, 0.7), (1.25, 0.5), (-0.4, 3.3), (1e-3, 1e3)):
        s, b = trap_range(lo, hi)
        assert type(s) is f32 and type(b) is f32
        want_s = f32(f32(1.0) / f32(f32(hi) - f32(lo)))
        want_b = f32(f32(-f32(lo)) * want_s)
        assert s.tobytes() == want_s.tobytes() and b.tobytes() == want_b.tobytes(), (lo, hi)
        rs, rb = TR.trap_range(lo, hi)  # the reference's
        assert s.tobytes() == rs.tobytes() and b.tobytes() == rb.tobytes()
    s, b = trap_range(0.3, 0.9)
    assert (float(s), float(b)) == (float(f32(1.6666667)), float(f32(-0.50000006)))  # not the f64 quotient's -0.5
    s, b = trap_range(0.0, 2.0)
    assert (float(s), abs(float(b))) == (0.5, 0.0)
    for bad in ((1.0, 1.0), (float("nan"), 1.0), (0.0, float("inf"))):
        with pytest.raises(ValueError):
            trap_range(*bad)


def test_refusals_without_a_device(kifs):
    """A null context is refused before anything else is looked at."""
    from kifs_raymarching_amd._lib import lib
    trap = kifs.OrbitTrap().into_buffer_data()
    outs = (C.c_void_p * 1)(16)
    assert lib.kifs_render_trapped_async(None, None, 1, None, None, 0, None, None, None, 0, 0, 1) == BAD_ARG
    assert lib.kifs_render_trapped_async(None, None, 1, None, outs, 64, C.byref(trap), None, None, 0, 1, 1) == BAD_ARG
    assert lib.kifs_eval_trap(None, C.byref(trap), None, 0, None) == BAD_ARG


def test_every_pipeline_is_compiled_without_scratch(kifs):
    from geometry_cases import PIPELINES
    from test_kernel_resources import _budget  # the resource test holds the new kernels to the render kernels' budgets
    report = kernel_report()
    names = [n for n in report if "trap::render_kernel<" in n]
    assert len(names) == len(PIPELINES) == 10, names
    pairs = sorted(tuple(int(v) for v in re.search(r"render_kernel<(\d+), (\d+)>", n).groups()) for n in names)
    assert pairs == sorted([(1, 0), (1, 1), (2, 0)] + [(0, p) for p in range(7)])  # as dispatch_pipeline<2> picks them
    for n in names:
        r = report[n]
        g, p = (int(v) for v in re.search(r"render_kernel<(\d+), (\d+)>", n).groups())
        want = (224, 2) if (g, p) == (0, 5) else (80, 6) if g in (1, 2) else (64, 6)
        assert _budget(n) == want, (n, _budget(n))
        assert int(r["ScratchSize [bytes/lane]"]) == 0 and int(r["VGPRs Spill"]) == 0 and r.get("Dynamic Stack") == "False", (n, r)
        assert int(r["VGPRs"]) <= want[0] and int(r["AGPRs"]) == 0 and int(r["Occupancy [waves/SIMD]"]) >= want[1], (n, r)
    evals = [n for n in report if "trap::eval_kernel<" in n]
    assert len(evals) == 9, evals  # one per pipeline; the two Julia forms of the march share theirs
    for n in evals:
        assert int(report[n]["ScratchSize [bytes/lane]"]) == 0 and int(report[n]["VGPRs Spill"]) == 0, (n, report[n])
