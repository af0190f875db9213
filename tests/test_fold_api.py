"""Kaleidoscopic IFS scenes (kifs_render_folded_async, kifs_eval_fold), the parts a machine without a GPU can check: the
header's text, the struct's layout against the header, the kernel argument's size, the ctypes binding, the Python layer's
validation and its feeding of the library 64 frames at a time (with a fake library), configs.fold_rotation against
kifs_host_rotation_matrix, the presets, the refusals that need no device, and that hipcc compiled fold::render_kernel for
every KIFS primitive without scratch memory."""
import ctypes as C
import inspect
import math
import re
import subprocess
from pathlib import Path

import numpy as np
import pytest

import fold_reference as FR
from kernel_report import kernel_report

ROOT = Path(__file__).resolve().parent.parent
HEADER = (ROOT / "include" / "kifs_hip.h").read_text()
BAD_ARG = 7


def test_header_declares_the_folded_surface():
    flat = re.sub(r"\s+", " ", re.sub(r"/\*.*?\*/", "", HEADER, flags=re.S))
    assert ("int kifs_render_folded_async(kifs_ctx* ctx, void* hip_stream, int count, const KifsCameraUniform* cameras, "
            "uint8_t* const* dev_outs_rgba8, size_t pitch_bytes, const KifsFoldSystem* fold, const KifsLight* light , "
            "const KifsAmbientOcclusion* ao , int y0, int y1, int encode);") in flat
    assert ("int kifs_eval_fold(kifs_ctx* ctx, const KifsFoldSystem* fold, const float* points_xyz, int n, float* sdf_out, "
            "float* normal_out_xyz);") in flat
    assert ("typedef struct KifsFoldSystem { uint32_t stages; int32_t iterations; float scale; float offset[3]; float rotation[9]; } "
            "KifsFoldSystem;") in flat
    assert ("enum KifsFoldStage { KIFS_FOLD_ABS = 1, KIFS_FOLD_SORT = 2, KIFS_FOLD_TETRA = 4, KIFS_FOLD_ROTATE = 8, "
            "KIFS_FOLD_MIRROR_Z = 16 };") in flat
    assert re.search(r"^#define KIFS_MAX_FOLD_ITERATIONS 24$", HEADER, re.M)
    assert re.search(r"^#define KIFS_MAX_FOLD_BATCH 64$", HEADER, re.M)
    assert re.search(r"^#define KIFS_ABI_VERSION 4$", HEADER, re.M)
    block = HEADER[HEADER.index("extension: kaleidoscopic IFS scenes"):HEADER.index("#define KIFS_MAX_FOLD_ITERATIONS")]
    assert HEADER.index("extension: orbit-trap surface colouring") < HEADER.index("extension: kaleidoscopic IFS scenes")  # after the trapped call
    for word in ("host", "estimate", "frame", "culls", "identity", "refusals", "scope"):  # the contract's paragraphs
        assert re.search(rf"^ \*   {word}\b", block, re.M), word
    for text in ("t_i = -(k * offset[i])", "h = 0.5 * t_z", "if (x < y) swap(x, y)", "fma(R[2], p.z, fma(R[1], p.y, R[0]*p.x))",
                 "p_i = fma(scale, p_i, t_i)", "p.z = |p.z - h| + h", "acc = acc * scale", "base(p) / acc", "x / 1.0f is x",
                 "tests/fold_reference.c", "per-frame systems", "a trap on a folded", "negative scales", "all three off"):
        assert text in block, text


def test_struct_layout_in_c(tmp_path):
    src = tmp_path / "t.c"
    fields = ("stages", "iterations", "scale", "offset", "rotation")
    src.write_text('#include "kifs_hip.h"\n#include <stdio.h>\n#include <stddef.h>\n'
                   'int main(void){printf("%zu", sizeof(KifsFoldSystem));'
                   + "".join(f'printf(" %zu", offsetof(KifsFoldSystem, {f}));' for f in fields)
                   + 'printf(" %d %d %d %d %d\\n", KIFS_FOLD_ABS, KIFS_FOLD_SORT, KIFS_FOLD_TETRA, KIFS_FOLD_ROTATE, KIFS_FOLD_MIRROR_Z);return 0;}\n')
    exe = tmp_path / "t"
    subprocess.run(["gcc", "-std=c99", "-Wall", "-Werror", "-pedantic", f"-I{ROOT / 'include'}", str(src), "-o", str(exe)], check=True)
    out = [int(v) for v in subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.split()]
    assert out == [60, 0, 4, 8, 12, 24, 1, 2, 4, 8, 16]
    from kifs_raymarching_amd._lib import FOLD_STAGES, KifsFoldSystemC
    assert C.sizeof(KifsFoldSystemC) == 60 and C.sizeof(FR.FoldC) == 60
    assert [getattr(KifsFoldSystemC, f).offset for f in fields] == out[1:6] == [getattr(FR.FoldC, f).offset for f in fields]
    assert FOLD_STAGES == dict(abs=1, sort=2, tetra=4, rotate=8, mirror_z=16)
    assert (FR.ABS, FR.SORT, FR.TETRA, FR.ROTATE, FR.MIRROR_Z) == (1, 2, 4, 8, 16)


def test_kernel_argument_fits(tmp_path):
    """fold::Params is light::Params and the 64-byte record behind it: 4024 + 64 = 4088 of the 4096 bytes a kernel
    argument may have, the light, the term and its flag at light::Params' offsets."""
    src = tmp_path / "t.cpp"
    src.write_text('#include <cstddef>\n#include <cstdint>\n#include <cstdio>\n#include "kifs_params.hpp"\n'
                   'using namespace kifs;\n'
                   'int main(){std::printf("%zu %zu %zu %zu %zu %zu %zu %zu %zu %zu %zu\\n", sizeof(light::Params), sizeof(fold::Fold), sizeof(fold::Params),'
                   'offsetof(light::Params, light), offsetof(fold::Params, light), offsetof(light::Params, has_ao), offsetof(fold::Params, has_ao),'
                   'offsetof(fold::Params, fold), sizeof(fold::EvalParams), offsetof(light::Params, ao), offsetof(fold::Params, ao));}\n')
    exe = tmp_path / "t"
    subprocess.run(["g++", "-std=c++17", "-Wno-invalid-offsetof", f"-I{ROOT / 'kifs_raymarching_amd' / 'csrc'}", str(src), "-o", str(exe)], check=True)
    lit, fold, params, l0, l1, a0, a1, f1, ev, o0, o1 = (int(v) for v in subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.split())
    assert (lit, fold, params) == (4024, 64, 4088) and params <= 4096 and l0 == l1 and a0 == a1 and o0 == o1 and f1 == 4024 and ev <= 4096


def test_library_exports_and_python_binds_it(kifs):
    from kifs_raymarching_amd import _lib
    from kifs_raymarching_amd._lib import LIB_PATH, SIGNATURES, AmbientOcclusionC, KifsFoldSystemC, KifsLightC, lib
    raw = C.CDLL(str(LIB_PATH))
    assert hasattr(raw, "kifs_render_folded_async") and hasattr(raw, "kifs_eval_fold")
    res, args = SIGNATURES["kifs_render_folded_async"]
    assert res is C.c_int and len(args) == 12
    assert args[6] is C.POINTER(KifsFoldSystemC) and args[7] is C.POINTER(KifsLightC) and args[8] is C.POINTER(AmbientOcclusionC)
    assert args[9:] == [C.c_int, C.c_int, C.c_int]
    res, args = SIGNATURES["kifs_eval_fold"]
    assert res is C.c_int and len(args) == 6 and args[1] is C.POINTER(KifsFoldSystemC) and args[3] is C.c_int
    assert (_lib.MAX_FOLD_ITERATIONS, _lib.MAX_FOLD_BATCH) == (24, 64)
    assert lib.kifs_abi_version() == 4
    assert len(kifs.GraphicState.KERNEL_NAMES) == 10  # not a feedback launch: no new KifsKernel value
    assert "FoldSystem" in kifs.__all__
    sig = inspect.signature(kifs.GraphicState.render_folded_batch)
    assert list(sig.parameters)[:5] == ["self", "cameras", "fold", "light", "ao"]
    assert sig.parameters["light"].default is None and sig.parameters["ao"].default is None
    sig = inspect.signature(kifs.GraphicState.render_folded)
    assert list(sig.parameters)[:4] == ["self", "fold", "light", "ao"]
    assert list(inspect.signature(kifs.GraphicState.eval_fold).parameters)[:3] == ["self", "fold", "points"]


def test_fold_system_takes_names_or_bits_and_refuses_what_the_library_would(kifs):
    f = kifs.FoldSystem(stages=("abs", "sort", "mirror_z"), iterations=3, scale=3.0, offset=(1, 1, 1))
    u = f.into_buffer_data()
    assert (u.stages, u.iterations, u.scale, list(u.offset), list(u.rotation)) == (19, 3, 3.0, [1.0, 1.0, 1.0], list(FR.IDENTITY))
    assert kifs.FoldSystem(stages="tetra|rotate").stage_bits() == 12 and kifs.FoldSystem(stages="ABS, Sort").stage_bits() == 3
    assert kifs.FoldSystem(stages=31).stage_bits() == 31 and kifs.FoldSystem(stages=[]).stage_bits() == 0
    d = kifs.FoldSystem()
    assert (d.stage_bits(), d.iterations, d.scale, tuple(d.offset)) == (0, 0, 2.0, (1.0, 1.0, 1.0))  # folds nothing
    m = np.arange(9, dtype=np.float64).reshape(3, 3)
    assert list(kifs.FoldSystem(stages="rotate", rotation=m).into_buffer_data().rotation) == [float(v) for v in range(9)]  # row-major, as given
    nan, inf = float("nan"), float("inf")
    nan_matrix = (nan,) + FR.IDENTITY[1:]
    for bad in (dict(stages=32), dict(stages=-1), dict(stages=1.5), dict(stages="fold"), dict(stages=("abs", "mirror")),
                dict(iterations=-1), dict(iterations=25), dict(iterations=2.5), dict(scale=0.5), dict(scale=16.5), dict(scale=nan),
                dict(scale=inf), dict(offset=(0, 0)), dict(offset=(0, nan, 0)), dict(offset=(1e39, 0, 0)), dict(rotation=(1, 0, 0)),
                dict(stages="rotate", rotation=nan_matrix), dict(stages=8, rotation=(inf,) + FR.IDENTITY[1:])):
        with pytest.raises(ValueError):
            kifs.FoldSystem(**bad).into_buffer_data()
    for good in (dict(stages=0), dict(stages=31), dict(iterations=0), dict(iterations=24), dict(scale=1.0), dict(scale=16.0),
                 dict(stages="abs", rotation=nan_matrix)):  # a matrix that is not read may hold anything
        kifs.FoldSystem(**good).into_buffer_data()


class _FakeLibrary:
    """kifs_render_folded_async recorded, everything else the real library's."""

    def __init__(self, real):
        self.real, self.calls = real, []

    def __getattr__(self, name):
        return getattr(self.real, name)

    def kifs_destroy(self, ctx):  # (the object under test holds no context of the real library's)
        assert ctx == 0x1234

    def kifs_render_folded_async(self, ctx, stream, count, cams, outs, pitch, fold, light, ao, y0, y1, encode):
        views = None if cams is None else [bytes(memoryview(cams[i]).cast("B")) for i in range(count)]
        self.calls.append(dict(ctx=ctx, stream=stream, count=count, cams=views, outs=[int(outs[i]) for i in range(count)], pitch=pitch,
                               fold=bytes(memoryview(fold._obj).cast("B")), light=None if light is None else bytes(memoryview(light._obj).cast("B")),
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
    fold = kifs.FoldSystem(stages=("tetra", "rotate"), iterations=5, rotation=FR.rot("z", 0.3))
    light = kifs.Light(direction=(0.0, 1.0, 0.5), ambient=0.2)
    ao = kifs.AmbientOcclusion(samples=3)
    assert g.render_folded_batch(cams, fold, light=light, ao=ao, colour=colour, encode=0) is colour
    assert [c["count"] for c in fake.calls] == [64, 64, 22]
    base = colour.data_ptr()
    images = [kifs.uniform_bytes(c.into_buffer_data()) for c in cams]
    first = 0
    for c in fake.calls:
        assert c["outs"] == [base + (first + i) * 240 for i in range(c["count"])] and c["cams"] == images[first:first + c["count"]]
        assert c["ctx"] == 0x1234 and c["stream"] is None and c["pitch"] == 40 and c["band"] == (0, 6) and c["encode"] == 0
        assert c["fold"] == kifs.uniform_bytes(fold.into_buffer_data()) and c["light"] == kifs.uniform_bytes(light.into_buffer_data())
        assert c["ao"] == kifs.uniform_bytes(ao.into_buffer_data())
        first += c["count"]
    # no light, no term, a band, the context's camera
    fake.calls.clear()
    band = torch.zeros((1, 2, 10, 4), dtype=torch.uint8)
    g.render_folded_batch(None, fold, colour=band, y0=3, y1=5)
    assert len(fake.calls) == 1
    c = fake.calls[0]
    assert c["count"] == 1 and c["cams"] is None and c["light"] is None and c["ao"] is None and c["band"] == (3, 5) and c["encode"] == 1
    # refused before the library is asked
    fake.calls.clear()
    with pytest.raises(ValueError):
        g.render_folded_batch([], fold, colour=colour)
    with pytest.raises(ValueError):
        g.render_folded_batch(cams, fold, colour=colour[:149])
    with pytest.raises(ValueError):
        g.render_folded_batch(cams, fold, colour=colour.to(torch.int8))
    with pytest.raises(ValueError):
        g.render_folded_batch(cams, kifs.FoldSystem(stages=32), colour=colour)
    with pytest.raises(ValueError):
        g.render_folded_batch(cams, kifs.FoldSystem(iterations=25), colour=colour)
    assert fake.calls == []
    g._ctx = None  # (nothing to destroy)


def test_fold_rotation_is_the_librarys_matrices_row_major(kifs):
    from kifs_raymarching_amd._lib import lib
    from kifs_raymarching_amd.configs import fold_rotation

    def host(axis, angle):
        m = (C.c_float * 9)()
        lib.kifs_host_rotation_matrix(axis, angle, m)
        return m

    def row_major(m):
        return tuple(float(m[3 * c + r]) for r in range(3) for c in range(3))

    assert fold_rotation() == FR.IDENTITY
    for axis, name in enumerate("xyz"):
        for angle in (0.0, 0.4, -1.3, math.pi / 2):
            assert fold_rotation((name, angle)) == row_major(host(axis, angle)) == fold_rotation((axis, angle))
            # ... which is the rotation the reference's convention gives, to f32 rounding
            assert np.allclose(fold_rotation((name, angle)), FR.rot(name, angle), atol=1e-6) or np.allclose(
                fold_rotation((name, angle)), FR.rot(name, -angle), atol=1e-6)
    a, b, out = host(1, 0.4), host(2, -0.2), (C.c_float * 9)()
    lib.kifs_host_mat3_mul(a, b, out)
    assert fold_rotation(("y", 0.4), ("z", -0.2)) == row_major(out)
    R = np.array(fold_rotation(("y", 0.4), ("z", -0.2), ("x", 1.1)), dtype=np.float64).reshape(3, 3)
    assert np.allclose(R @ R.T, np.eye(3), atol=1e-6) and abs(np.linalg.det(R) - 1.0) < 1e-6
    for bad in (("w", 0.1), (3, 0.1), ("x", float("nan"))):
        with pytest.raises(ValueError):
            fold_rotation(bad)


def test_presets(kifs):
    from kifs_raymarching_amd.configs import FOLD_PRESETS
    assert {"menger", "flake", "tetra"} <= set(FOLD_PRESETS)
    for name, (shape, fold) in FOLD_PRESETS.items():
        assert isinstance(shape, kifs.PrimitiveShape) and isinstance(fold, kifs.FoldSystem)
        fold.into_buffer_data()
    shape, fold = FOLD_PRESETS["menger"]
    assert shape == kifs.PrimitiveShape.Box and (fold.stage_bits(), fold.scale, tuple(fold.offset)) == (19, 3.0, (1.0, 1.0, 1.0))
    shape, fold = FOLD_PRESETS["flake"]
    assert shape == kifs.PrimitiveShape.Box and fold.stage_bits() == FR.ABS | FR.SORT | FR.ROTATE
    shape, fold = FOLD_PRESETS["tetra"]
    assert shape == kifs.PrimitiveShape.Torus and fold.stage_bits() == FR.TETRA | FR.ROTATE


def test_refusals_without_a_device(kifs):
    """A null context is refused before anything else is looked at."""
    from kifs_raymarching_amd._lib import lib
    fold = kifs.FoldSystem().into_buffer_data()
    outs = (C.c_void_p * 1)(16)
    assert lib.kifs_render_folded_async(None, None, 1, None, None, 0, None, None, None, 0, 0, 1) == BAD_ARG
    assert lib.kifs_render_folded_async(None, None, 1, None, outs, 64, C.byref(fold), None, None, 0, 1, 1) == BAD_ARG
    assert lib.kifs_eval_fold(None, C.byref(fold), None, 0, None, None) == BAD_ARG


def test_every_primitive_is_compiled_without_scratch(kifs):
    from test_kernel_resources import _budget  # the resource test holds the new kernels to the render kernels' budgets
    report = kernel_report()
    names = [n for n in report if "fold::render_kernel<" in n]
    assert len(names) == 7, names
    pairs = sorted(tuple(int(v) for v in re.search(r"render_kernel<(\d+), (\d+)>", n).groups()) for n in names)
    assert pairs == [(0, p) for p in range(7)]  # the six primitives and the unknown id; no Julia form
    for n in names:
        r = report[n]
        g, p = (int(v) for v in re.search(r"render_kernel<(\d+), (\d+)>", n).groups())
        want = (224, 2) if (g, p) == (0, 5) else (64, 6)
        assert _budget(n) == want, (n, _budget(n))
        assert int(r["ScratchSize [bytes/lane]"]) == 0 and int(r["VGPRs Spill"]) == 0 and r.get("Dynamic Stack") == "False", (n, r)
        assert int(r["VGPRs"]) <= want[0] and int(r["AGPRs"]) == 0 and int(r["Occupancy [waves/SIMD]"]) >= want[1], (n, r)
    evals = [n for n in report if "fold::eval_kernel<" in n]
    assert len(evals) == 7, evals
    for n in evals:
        assert int(report[n]["ScratchSize [bytes/lane]"]) == 0 and int(report[n]["VGPRs Spill"]) == 0, (n, report[n])
