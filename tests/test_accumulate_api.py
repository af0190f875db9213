"""Accumulated frames (kifs_render_accumulate_async), the parts a machine without a GPU can check: the ABI surface, the
Python and CLI surface, and that hipcc compiled accum::render_kernel for every pipeline -- ten instantiations, none with
scratch or spills, each with its claim in the kernel-form table (kernel_forms.ACCUMULATE_FORMS), and their (GROUP, PRIM)
pairs the ones geometry_cases.PIPELINES dispatch to."""
import ctypes as C
import re
import subprocess
import sys
from pathlib import Path

from kernel_report import kernel_report

ROOT = Path(__file__).resolve().parent.parent
HEADER = (ROOT / "include" / "kifs_hip.h").read_text()


def test_header_declares_the_accumulate_surface():
    flat = re.sub(r"\s+", " ", re.sub(r"/\*.*?\*/", "", HEADER, flags=re.S))
    assert ("int kifs_render_accumulate_async(kifs_ctx* ctx, void* hip_stream, int count, int samples, "
            "const KifsCameraUniform* cameras, const KifsOptionsUniform* options, uint8_t* const* dev_outs_rgba8, "
            "size_t pitch_bytes, int y0, int y1, int encode);") in flat
    assert re.search(r"^#define KIFS_MAX_ACCUMULATE 64$", HEADER, re.M)
    assert re.search(r"KIFS_KERNEL_ACCUMULATE = 9\b", HEADER)
    assert re.search(r"^#define KIFS_ABI_VERSION 4$", HEADER, re.M)


def test_library_exports_and_python_binds_it(kifs):
    from kifs_raymarching_amd import graphics
    from kifs_raymarching_amd._lib import LIB_PATH, SIGNATURES, lib
    assert hasattr(C.CDLL(str(LIB_PATH)), "kifs_render_accumulate_async")
    res, args = SIGNATURES["kifs_render_accumulate_async"]
    assert res is C.c_int and len(args) == 11
    assert lib.kifs_abi_version() == 4
    assert lib.kifs_render_accumulate_async(None, None, 1, 1, None, None, None, 0, 0, 0, 1) == 7  # BAD_ARG, no crash
    assert callable(getattr(kifs.GraphicState, "render_accumulate", None))
    assert kifs.GraphicState.KERNEL_NAMES[9] == "render_accumulate_kernel" and len(kifs.GraphicState.KERNEL_NAMES) == 10
    assert graphics.MAX_ACCUMULATE == kifs.MAX_ACCUMULATE == 64


def test_render_tool_offers_motion_blur_and_depth_of_field(kifs):
    p = subprocess.run([sys.executable, str(ROOT / "tools" / "render.py"), "--help"], capture_output=True, text=True,
                       timeout=120)
    assert p.returncode == 0, p.stderr
    for flag in ("--motion-blur", "--shutter", "--dof", "--samples", "--morph-to"):
        assert flag in p.stdout, flag


def test_every_pipeline_is_compiled_without_scratch_and_claimed_by_the_form_table(kifs):
    from geometry_cases import PIPELINES, cases
    from kernel_forms import ACCUMULATE_FORMS
    from test_kernel_form_coverage import RENDER  # the form table's own pattern
    report = kernel_report()
    names = [n for n in report if "kifs::accum::render_kernel<" in n]
    assert len(names) == len(PIPELINES) == 10, names
    assert all(RENDER.search(n) for n in names) and sorted(names) == sorted(ACCUMULATE_FORMS)
    for n in names:
        r = report[n]
        assert int(r["ScratchSize [bytes/lane]"]) == 0 and int(r["VGPRs Spill"]) == 0 and r.get("Dynamic Stack") == "False", (n, r)
    # the (GROUP, PRIM) pair dispatch_pipeline<2> takes for every pipeline's scene
    got = sorted(re.search(r"render_kernel<(\d+), (\d+)>", n).groups() for n in names)
    want = []
    for pipeline, (_, _, gui, iters) in cases(kifs, 64, 48).items():
        u = gui.into_buffer_data()
        group, prim = int(u.fractal_group_id), int(u.primitive_id)
        pair = (1, int(iters[0] <= 24)) if group == 1 else (2, 0) if group == 2 else (0, min(prim, 6))
        want.append(tuple(str(v) for v in pair))
    assert sorted(want) == got and len(set(want)) == 10
