"""Ray queries (kifs_trace_rays_async), the parts a machine without a GPU can check: the ABI surface and its refusals, the
Python surface, and that hipcc compiled rays::trace_render_kernel for every pipeline -- ten instantiations inside the
render kernels' budgets, their (GROUP, PRIM) pairs the ones geometry_cases.PIPELINES dispatch to -- under a name the
resource test grants those budgets and the form-coverage pattern does not claim."""
import ctypes as C
import inspect
import re
from pathlib import Path

from kernel_report import kernel_report

import ray_forms as RF

ROOT = Path(__file__).resolve().parent.parent
HEADER = (ROOT / "include" / "kifs_hip.h").read_text()
BAD_ARG = 7


def test_header_declares_the_ray_surface():
    flat = re.sub(r"\s+", " ", re.sub(r"/\*.*?\*/", "", HEADER, flags=re.S))
    assert ("int kifs_trace_rays_async(kifs_ctx* ctx, void* hip_stream, const KifsRay* dev_rays, int n, "
            "float* dev_geometry , uint8_t* dev_rgba8 , int encode);") in flat
    assert "typedef struct KifsRay { float origin[3]; float reserved0; float direction[3]; float reserved1; } KifsRay;" in flat
    assert re.search(r"^#define KIFS_MAX_RAYS \(1 << 28\)$", HEADER, re.M)
    assert re.search(r"^#define KIFS_ABI_VERSION 4$", HEADER, re.M)
    assert re.search(r"KIFS_KERNEL_ACCUMULATE = 9\b", HEADER) and not re.search(r"KIFS_KERNEL_\w+ = 10\b", HEADER)
    block = HEADER[HEADER.index("extension: ray queries"):HEADER.index("typedef struct KifsRay")]
    for word in ("rays", "march", "direction", "state", "texel", "colour", "outputs", "non-finite", "refusals", "ordering",
                 "launch"):  # the contract's paragraphs
        assert re.search(rf"^ \*   {word}\b", block, re.M), word
    assert "NOT normalised" in block and "0, 0, 0, 0x7f800000" in block and "tests/ray_reference.c" in block


def test_library_exports_and_python_binds_it(kifs):
    from kifs_raymarching_amd import _lib
    from kifs_raymarching_amd._lib import LIB_PATH, SIGNATURES, KifsRay, lib
    assert hasattr(C.CDLL(str(LIB_PATH)), "kifs_trace_rays_async")
    res, args = SIGNATURES["kifs_trace_rays_async"]
    assert res is C.c_int and len(args) == 7 and args[3] is C.c_int and args[6] is C.c_int
    assert C.sizeof(KifsRay) == 32 and KifsRay.origin.offset == 0 and KifsRay.direction.offset == 16
    assert _lib.MAX_RAYS == 1 << 28
    assert lib.kifs_abi_version() == 4
    assert len(kifs.GraphicState.KERNEL_NAMES) == 10  # not a render launch: no new KifsKernel value
    sig = inspect.signature(kifs.GraphicState.trace_rays)
    assert list(sig.parameters) == ["self", "rays", "colours", "geometry", "encode", "stream"]
    assert sig.parameters["colours"].default is True and sig.parameters["geometry"].default is True
    assert sig.parameters["encode"].default == kifs.ENCODE_SRGB and sig.parameters["stream"].default is None
    from kifs_raymarching_amd import configs
    assert list(inspect.signature(configs.pixel_rays).parameters) == ["screen", "camera"]
    assert list(inspect.signature(configs.panorama_rays).parameters) == ["origin", "width", "height"]


def test_refusals_without_a_device(kifs):
    """A null context is refused before anything else is looked at."""
    from kifs_raymarching_amd._lib import lib
    assert lib.kifs_trace_rays_async(None, None, None, 0, None, None, 1) == BAD_ARG
    assert lib.kifs_trace_rays_async(None, None, 16, 1, 16, 16, 1) == BAD_ARG


def test_every_pipeline_is_compiled_inside_the_render_budgets(kifs):
    from geometry_cases import PIPELINES, cases
    from test_kernel_form_coverage import RENDER  # the form table's pattern must NOT claim the new family
    from test_kernel_resources import _budget     # ... and the resource test must grant it the render kernels' budgets
    report = kernel_report()
    names = [n for n in report if "trace_render_kernel<" in n]
    assert len(names) == len(PIPELINES) == 10, names
    assert sorted(names) == sorted(RF.RAY_FORMS)
    assert not any(RENDER.search(n) for n in names)
    for n in names:
        r = report[n]
        g, p = (int(v) for v in re.search(r"trace_render_kernel<(\d+), (\d+)>", n).groups())
        want = (224, 2) if (g, p) == (0, 5) else (80, 6) if g in (1, 2) else (64, 6)
        assert _budget(n) == want, (n, _budget(n))
        assert int(r["ScratchSize [bytes/lane]"]) == 0 and int(r["VGPRs Spill"]) == 0 and r.get("Dynamic Stack") == "False", (n, r)
        assert int(r["VGPRs"]) <= want[0] and int(r["AGPRs"]) == 0 and int(r["Occupancy [waves/SIMD]"]) >= want[1], (n, r)
        assert int(r["SGPRs Spill"]) <= (48 if g in (1, 2) else 4), (n, r)
    got = sorted(re.search(r"trace_render_kernel<(\d+), (\d+)>", n).groups() for n in names)
    want = []
    for pipeline, (_, _, gui, iters) in cases(kifs, 64, 48).items():
        u = gui.into_buffer_data()
        group, prim = int(u.fractal_group_id), int(u.primitive_id)
        pair = (1, int(iters[0] <= 24)) if group == 1 else (2, 0) if group == 2 else (0, min(prim, 6))
        want.append(tuple(str(v) for v in pair))
    assert sorted(want) == got and len(set(want)) == 10


def test_the_table_claims_name_cases_of_the_gpu_test(kifs):
    """As test_extension_claims_name_cases_of_the_extension_tests: test_every_pipeline_bit_exact of the GPU file runs every
    name of geometry_cases.PIPELINES, and each instantiation is claimed by the pipeline dispatch_pipeline takes it for."""
    from geometry_cases import PIPELINES, cases
    (file, forms), = RF.RAY_TESTS.items()
    text = (Path(__file__).resolve().parent / file).read_text()
    assert re.search(r"^from geometry_cases import [^\n]*\bPIPELINES\b", text, re.M)
    assert re.search(r'@pytest\.mark\.parametrize\("name", PIPELINES\)\s*\n(?:@pytest\.mark\.parametrize\([^\n]*\n)*'
                     r'def test_every_pipeline_bit_exact\(', text), "the parameter list of test_every_pipeline_bit_exact"
    assert len(forms) == 10 and sorted(forms.values()) == sorted(PIPELINES)
    scenes = cases(kifs, 64, 48)
    for name, pipeline in forms.items():
        _, _, gui, iters = scenes[pipeline]
        u = gui.into_buffer_data()
        group, prim = int(u.fractal_group_id), int(u.primitive_id)
        pair = (1, int(iters[0] <= 24)) if group == 1 else (2, 0) if group == 2 else (0, min(prim, 6))
        assert re.search(r"\btrace_render_kernel<(\d+), (\d+)>", name).groups() == tuple(str(v) for v in pair), (name, pipeline)
