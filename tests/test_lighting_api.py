"""The configurable light (kifs_render_lit_async), the parts a machine without a GPU can check: the header's text, the ABI
version, the ctypes binding and the struct's layout, the Python surface, configs.light_direction, the refusals that need no
device, the kernel argument's size, and that hipcc compiled light::render_kernel for every pipeline inside the render
kernels' budgets."""
import ctypes as C
import inspect
import math
import re
import subprocess
from pathlib import Path

import numpy as np

from kernel_report import kernel_report

ROOT = Path(__file__).resolve().parent.parent
HEADER = (ROOT / "include" / "kifs_hip.h").read_text()
BAD_ARG = 7


def test_header_declares_the_lit_surface():
    flat = re.sub(r"\s+", " ", re.sub(r"/\*.*?\*/", "", HEADER, flags=re.S))
    assert ("int kifs_render_lit_async(kifs_ctx* ctx, void* hip_stream, int count, const KifsCameraUniform* cameras, "
            "uint8_t* const* dev_outs_rgba8, size_t pitch_bytes, const KifsLight* light, const KifsAmbientOcclusion* ao , "
            "int y0, int y1, int encode);") in flat
    assert ("typedef struct KifsLight { float direction[3]; float ambient; float diffuse; float specular[3]; "
            "int32_t shininess_log2; } KifsLight;") in flat
    assert re.search(r"^#define KIFS_MAX_SHININESS_LOG2 10$", HEADER, re.M)
    assert re.search(r"^#define KIFS_MAX_LIGHT_BATCH 64$", HEADER, re.M)
    assert re.search(r"^#define KIFS_ABI_VERSION 4$", HEADER, re.M)
    assert re.search(r"KIFS_KERNEL_ACCUMULATE = 9\b", HEADER) and not re.search(r"KIFS_KERNEL_\w+ = 10\b", HEADER)
    block = HEADER[HEADER.index("extension: a configurable light"):HEADER.index("#define KIFS_MAX_SHININESS_LOG2")]
    for word in ("hit", "other", "samples", "frames", "identity", "refusals", "launch", "scope"):  # the contract's paragraphs
        assert re.search(rf"^ \*   {word}\b", block, re.M), word
    for text in ("fma(light.diffuse, lit, light.ambient)", "normalize3(Lh - dir)", "(lit0 > 0) ? s * sh : 0", "(n.x + n.y) + n.z",
                 "tests/lighting_reference.c", "kifs_render_occlusion_async", "a second light"):
        assert text in block, text


def test_struct_layout_in_c(tmp_path):
    src = tmp_path / "t.c"
    src.write_text('#include "kifs_hip.h"\n#include <stdio.h>\n#include <stddef.h>\n'
                   'int main(void){printf("%zu %zu %zu %zu %zu %zu\\n", sizeof(KifsLight), offsetof(KifsLight, direction),'
                   'offsetof(KifsLight, ambient), offsetof(KifsLight, diffuse), offsetof(KifsLight, specular),'
                   'offsetof(KifsLight, shininess_log2));return 0;}\n')
    exe = tmp_path / "t"
    subprocess.run(["gcc", "-std=c99", "-Wall", "-Werror", "-pedantic", f"-I{ROOT / 'include'}", str(src), "-o", str(exe)], check=True)
    assert subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.split() == ["36", "0", "12", "16", "20", "32"]


def test_kernel_argument_fits(tmp_path):
    """light::Params is BatchParams + the light + the term + a flag, under the 4096 bytes a kernel argument may have."""
    src = tmp_path / "t.cpp"
    src.write_text('#include <cstdint>\n#include <cstdio>\n#include "kifs_params.hpp"\n'
                   'int main(){std::printf("%zu %zu %zu\\n", sizeof(kifs::BatchParams), sizeof(kifs::light::Light), sizeof(kifs::light::Params));}\n')
    exe = tmp_path / "t"
    subprocess.run(["g++", "-std=c++17", f"-I{ROOT / 'kifs_raymarching_amd' / 'csrc'}", str(src), "-o", str(exe)], check=True)
    batch, light, params = (int(v) for v in subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.split())
    assert batch == 3952 and light == 52 and batch + light + 16 + 4 <= params <= 4096


def test_library_exports_and_python_binds_it(kifs):
    from kifs_raymarching_amd import _lib
    from kifs_raymarching_amd._lib import LIB_PATH, SIGNATURES, AmbientOcclusionC, KifsLightC, lib
    assert hasattr(C.CDLL(str(LIB_PATH)), "kifs_render_lit_async")
    res, args = SIGNATURES["kifs_render_lit_async"]
    assert res is C.c_int and len(args) == 11
    assert args[2] is C.c_int and args[5] is C.c_size_t
    assert args[6] is C.POINTER(KifsLightC) and args[7] is C.POINTER(AmbientOcclusionC) and args[8:] == [C.c_int, C.c_int, C.c_int]
    assert C.sizeof(KifsLightC) == 36
    assert [f[0] for f in KifsLightC._fields_] == ["direction", "ambient", "diffuse", "specular", "shininess_log2"]
    assert (_lib.MAX_SHININESS_LOG2, _lib.MAX_LIGHT_BATCH) == (10, 64)
    assert lib.kifs_abi_version() == 4
    assert len(kifs.GraphicState.KERNEL_NAMES) == 10  # not a feedback launch: no new KifsKernel value
    light = kifs.Light()
    assert (tuple(light.direction), light.ambient, light.diffuse, tuple(light.specular), light.shininess_log2) == ((1, 1, 1), 0.1, 0.9, (0, 0, 0), 5)
    u = light.into_buffer_data()
    assert (list(u.direction), u.ambient, u.diffuse, list(u.specular), u.shininess_log2) == \
        ([1.0, 1.0, 1.0], C.c_float(0.1).value, C.c_float(0.9).value, [0.0, 0.0, 0.0], 5)
    assert "Light" in kifs.__all__
    sig = inspect.signature(kifs.GraphicState.render_lit_batch)
    assert list(sig.parameters)[:4] == ["self", "cameras", "light", "ao"] and sig.parameters["ao"].default is None
    sig = inspect.signature(kifs.GraphicState.render_lit)
    assert list(sig.parameters)[:3] == ["self", "light", "ao"] and sig.parameters["ao"].default is None


def test_light_direction_is_a_unit_vector(kifs):
    from kifs_raymarching_amd.configs import light_direction
    for az, el in ((0.0, 0.0), (0.7, 0.3), (-2.5, 1.2), (4.0, -0.9), (1.0, math.pi / 2)):
        v = np.array(light_direction(az, el))
        assert abs(np.linalg.norm(v) - 1.0) < 1e-12, (az, el)
        assert abs(v[2] - math.sin(el)) < 1e-12
        if abs(math.cos(el)) > 1e-9:
            assert abs(math.atan2(v[1], v[0]) - math.atan2(math.sin(az), math.cos(az))) < 1e-9, (az, el)
    assert np.allclose(light_direction(0.0, 0.0), (1, 0, 0)) and np.allclose(light_direction(math.pi / 2, 0.0), (0, 1, 0), atol=1e-15)
    assert np.allclose(light_direction(math.pi / 4, math.atan(1 / math.sqrt(2))), np.ones(3) / math.sqrt(3))  # the reference's light


def test_refusals_without_a_device(kifs):
    """A null context is refused before anything else is looked at."""
    from kifs_raymarching_amd._lib import AmbientOcclusionC, KifsLightC, lib
    light = kifs.Light().into_buffer_data()
    ao = AmbientOcclusionC(5, 0.02, 0.75, 4.0)
    assert lib.kifs_render_lit_async(None, None, 1, None, None, 0, None, None, 0, 0, 1) == BAD_ARG
    outs = (C.c_void_p * 1)(16)
    assert lib.kifs_render_lit_async(None, None, 1, None, outs, 64, C.byref(light), C.byref(ao), 0, 1, 1) == BAD_ARG
    assert isinstance(light, KifsLightC)


def test_every_pipeline_is_compiled_inside_the_render_budgets(kifs):
    from geometry_cases import PIPELINES
    from kernel_forms import LIGHTING_FORMS
    from test_kernel_form_coverage import RENDER  # the form table's own pattern: it claims the family (kernel_forms.LIGHTING_FORMS)
    from test_kernel_resources import _budget     # ... and the resource test grants it the render kernels' budgets
    report = kernel_report()
    names = [n for n in report if "light::render_kernel<" in n]
    assert len(names) == len(PIPELINES) == 10, names
    assert all(RENDER.search(n) for n in names) and sorted(names) == sorted(LIGHTING_FORMS)
    pairs = sorted(tuple(int(v) for v in re.search(r"render_kernel<(\d+), (\d+)>", n).groups()) for n in names)
    assert pairs == sorted([(1, 0), (1, 1), (2, 0)] + [(0, p) for p in range(7)])  # as dispatch_pipeline<2> picks them
    for n in names:
        r = report[n]
        g, p = (int(v) for v in re.search(r"render_kernel<(\d+), (\d+)>", n).groups())
        want = (224, 2) if (g, p) == (0, 5) else (80, 6) if g in (1, 2) else (64, 6)
        assert _budget(n) == want, (n, _budget(n))
        assert int(r["ScratchSize [bytes/lane]"]) == 0 and int(r["VGPRs Spill"]) == 0 and r.get("Dynamic Stack") == "False", (n, r)
        assert int(r["VGPRs"]) <= want[0] and int(r["AGPRs"]) == 0 and int(r["Occupancy [waves/SIMD]"]) >= want[1], (n, r)
        assert int(r["SGPRs Spill"]) <= (48 if g in (1, 2) else 4), (n, r)


def test_render_tool_refuses_what_the_lit_call_does_not_do():
    """--light and --specular with the accumulate, geometry or panorama switches: refused before a device is touched, with
    a message that says why."""
    import sys
    tool = str(ROOT / "tools" / "render.py")
    for extra, why in ((["--light", "1,2,3", "--geometry", "g.bin"], "shade with the reference's light"),
                       (["--specular", "1,1,1,3", "--motion-blur", "4", "--frames", "0", "1"], "shade with the reference's light"),
                       (["--light", "1,2,3", "--panorama", "0,0,2.5"], "nor a light of the caller's"),
                       (["--light", "1,2"], "three numbers X,Y,Z or five")):
        p = subprocess.run([sys.executable, tool, "cfg2_julia_1080p", "out.png", *extra], capture_output=True, text=True, timeout=120)
        assert p.returncode == 2 and why in p.stderr, (extra, p.returncode, p.stderr[-400:])
