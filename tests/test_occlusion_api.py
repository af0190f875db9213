"""Ambient occlusion (kifs_render_occlusion_async), the parts a machine without a GPU can check: the header's text, the
ABI version, the ctypes binding and the struct's size, the Python surface, the refusals that need no device, and that hipcc
compiled occl::render_kernel for every pipeline inside the render kernels' budgets."""
import ctypes as C
import inspect
import re
import subprocess
from pathlib import Path

from kernel_report import kernel_report

ROOT = Path(__file__).resolve().parent.parent
HEADER = (ROOT / "include" / "kifs_hip.h").read_text()
BAD_ARG = 7


def test_header_declares_the_occlusion_surface():
    flat = re.sub(r"\s+", " ", re.sub(r"/\*.*?\*/", "", HEADER, flags=re.S))
    assert ("int kifs_render_occlusion_async(kifs_ctx* ctx, void* hip_stream, int count, const KifsCameraUniform* cameras, "
            "uint8_t* const* dev_outs_rgba8, size_t pitch_bytes, const KifsAmbientOcclusion* ao, float* dev_occlusion, "
            "size_t occlusion_pitch_bytes, size_t occlusion_stride_bytes, int y0, int y1, int encode);") in flat
    assert ("typedef struct KifsAmbientOcclusion { int32_t samples; float step; float decay; float strength; } "
            "KifsAmbientOcclusion;") in flat
    assert re.search(r"^#define KIFS_MAX_AO_SAMPLES 16$", HEADER, re.M)
    assert re.search(r"^#define KIFS_MAX_OCCLUSION_BATCH 64$", HEADER, re.M)
    assert re.search(r"^#define KIFS_ABI_VERSION 4$", HEADER, re.M)
    assert re.search(r"KIFS_KERNEL_ACCUMULATE = 9\b", HEADER) and not re.search(r"KIFS_KERNEL_\w+ = 10\b", HEADER)
    block = HEADER[HEADER.index("extension: ambient occlusion"):HEADER.index("#define KIFS_MAX_AO_SAMPLES")]
    for word in ("factor", "colour", "samples", "plane", "frames", "refusals", "ordering", "launch"):  # the contract's paragraphs
        assert re.search(rf"^ \*   {word}\b", block, re.M), word
    assert "fma(h, n, p)" in block and "occ + w * (h - d)" in block and "tests/occlusion_reference.c" in block


def test_struct_is_sixteen_bytes_in_c(tmp_path):
    src = tmp_path / "t.c"
    src.write_text('#include "kifs_hip.h"\n#include <stdio.h>\n#include <stddef.h>\n'
                   'int main(void){printf("%zu %zu %zu %zu %zu\\n", sizeof(KifsAmbientOcclusion),'
                   'offsetof(KifsAmbientOcclusion, samples), offsetof(KifsAmbientOcclusion, step),'
                   'offsetof(KifsAmbientOcclusion, decay), offsetof(KifsAmbientOcclusion, strength));return 0;}\n')
    exe = tmp_path / "t"
    subprocess.run(["gcc", "-std=c99", "-Wall", "-Werror", "-pedantic", f"-I{ROOT / 'include'}", str(src), "-o", str(exe)], check=True)
    assert subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.split() == ["16", "0", "4", "8", "12"]


def test_library_exports_and_python_binds_it(kifs):
    from kifs_raymarching_amd import _lib
    from kifs_raymarching_amd._lib import LIB_PATH, SIGNATURES, AmbientOcclusionC, lib
    assert hasattr(C.CDLL(str(LIB_PATH)), "kifs_render_occlusion_async")
    res, args = SIGNATURES["kifs_render_occlusion_async"]
    assert res is C.c_int and len(args) == 13
    assert args[2] is C.c_int and args[5] is C.c_size_t and args[8] is C.c_size_t and args[9] is C.c_size_t
    assert args[6] is C.POINTER(AmbientOcclusionC) and args[10:] == [C.c_int, C.c_int, C.c_int]
    assert C.sizeof(AmbientOcclusionC) == 16
    assert [f[0] for f in AmbientOcclusionC._fields_] == ["samples", "step", "decay", "strength"]
    assert (_lib.MAX_AO_SAMPLES, _lib.MAX_OCCLUSION_BATCH) == (16, 64)
    assert lib.kifs_abi_version() == 4
    assert len(kifs.GraphicState.KERNEL_NAMES) == 10  # not a feedback launch: no new KifsKernel value
    ao = kifs.AmbientOcclusion()
    assert (ao.samples, ao.step, ao.decay, ao.strength) == (5, 0.02, 0.75, 4.0)
    u = ao.into_buffer_data()
    assert (u.samples, u.step, u.decay, u.strength) == (5, C.c_float(0.02).value, 0.75, 4.0)
    assert "AmbientOcclusion" in kifs.__all__
    sig = inspect.signature(kifs.GraphicState.render_occlusion_batch)
    assert list(sig.parameters)[:4] == ["self", "cameras", "ao", "occlusion"]
    assert sig.parameters["cameras"].default is None and sig.parameters["occlusion"].default is False
    sig = inspect.signature(kifs.GraphicState.render_occlusion)
    assert list(sig.parameters)[:3] == ["self", "ao", "occlusion"]


def test_refusals_without_a_device(kifs):
    """A null context is refused before anything else is looked at."""
    from kifs_raymarching_amd._lib import AmbientOcclusionC, lib
    ao = AmbientOcclusionC(5, 0.02, 0.75, 4.0)
    assert lib.kifs_render_occlusion_async(None, None, 1, None, None, 0, None, None, 0, 0, 0, 0, 1) == BAD_ARG
    outs = (C.c_void_p * 1)(16)
    assert lib.kifs_render_occlusion_async(None, None, 1, None, outs, 64, C.byref(ao), 16, 64, 64, 0, 1, 1) == BAD_ARG


def test_every_pipeline_is_compiled_inside_the_render_budgets(kifs):
    from geometry_cases import PIPELINES
    from kernel_forms import OCCLUSION_FORMS
    from test_kernel_form_coverage import RENDER  # the form table's own pattern: it claims the family (kernel_forms.OCCLUSION_FORMS)
    from test_kernel_resources import _budget     # ... and the resource test grants it the render kernels' budgets
    report = kernel_report()
    names = [n for n in report if "occl::render_kernel<" in n]
    assert len(names) == len(PIPELINES) == 10, names
    assert all(RENDER.search(n) for n in names) and sorted(names) == sorted(OCCLUSION_FORMS)
    pairs = sorted(tuple(int(v) for v in re.search(r"render_kernel<(\d+), (\d+)>", n).groups()) for n in names)
    assert pairs == sorted([(1, 0), (1, 1), (2, 0)] + [(0, p) for p in range(7)])  # as dispatch_pipeline<2> picks them
    for n in names:
        r = report[n]
        g, p = (int(v) for v in re.search(r"render_kernel<(\d+), (\d+)>", n).groups())
        want = (224, 2) if (g, p) == (0, 5) else (80, 6) if g in (1, 2) else (64, 6)
        assert _budget(n) == want, (n, _budget(n))
        assert int(r["ScratchSize [bytes/lane]"]) == 0 and int(r["VGPRs Spill"]) == 0 and r.get("Dynamic Stack") == "False", (n, r)
        assert int(r["VGPRs"]) <= want[0] and int(r["AGPRs"]) == 0 and int(r["Occupancy [waves/SIMD]"]) >= want[1], (n, r)
        assert int(r["SGPRs Spill"]) <= 4, (n, r)
