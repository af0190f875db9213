"""Jittered accumulated frames (kifs_render_accumulate_jittered_async), the parts a machine without a GPU can check: the ABI
surface, the Python and CLI surface, and that hipcc compiled accum::jitter_render_kernel for every pipeline -- ten
instantiations, none with scratch, spills or a dynamic stack, each with its claim in the kernel-form table
(kernel_forms.JITTER_FORMS), their (GROUP, PRIM) pairs the ones geometry_cases.PIPELINES dispatch to -- beside accum::render_kernel's ten, which stay."""
import ctypes as C
import re
import subprocess
import sys
from pathlib import Path

from kernel_report import kernel_report

ROOT = Path(__file__).resolve().parent.parent
HEADER = (ROOT / "include" / "kifs_hip.h").read_text()


def test_header_declares_the_jittered_surface():
    flat = re.sub(r"\s+", " ", re.sub(r"/\*.*?\*/", "", HEADER, flags=re.S))
    assert ("int kifs_render_accumulate_jittered_async(kifs_ctx* ctx, void* hip_stream, int count, int samples, "
            "const KifsCameraUniform* cameras, const KifsOptionsUniform* options, int grid, const KifsSubpixel* cells , "
            "uint8_t* const* dev_outs_rgba8, size_t pitch_bytes, int y0, int y1, int encode);") in flat
    assert "typedef struct KifsSubpixel { uint8_t i, j; } KifsSubpixel;" in flat
    assert re.search(r"^#define KIFS_MAX_JITTER_GRID 8$", HEADER, re.M)
    assert re.search(r"^#define KIFS_ABI_VERSION 4$", HEADER, re.M)
    assert re.search(r"KIFS_KERNEL_ACCUMULATE = 9\b", HEADER) and not re.search(r"KIFS_KERNEL_\w+ = 10\b", HEADER)
    assert "out of scope, as for the other extensions" not in HEADER  # the accumulated calls point at the jittered one


def test_library_exports_and_python_binds_it(kifs):
    import inspect
    from kifs_raymarching_amd import _lib, configs, graphics
    from kifs_raymarching_amd._lib import LIB_PATH, SIGNATURES, lib
    assert hasattr(C.CDLL(str(LIB_PATH)), "kifs_render_accumulate_jittered_async")
    res, args = SIGNATURES["kifs_render_accumulate_jittered_async"]
    assert res is C.c_int and len(args) == 13
    assert lib.kifs_abi_version() == 4
    assert lib.kifs_render_accumulate_jittered_async(None, None, 1, 1, None, None, 1, None, None, 0, 0, 0, 1) == 7  # BAD_ARG
    assert C.sizeof(_lib.KifsSubpixel) == 2 and [f[0] for f in _lib.KifsSubpixel._fields_] == ["i", "j"]
    assert _lib.MAX_JITTER_GRID == graphics.MAX_JITTER_GRID == kifs.MAX_JITTER_GRID == 8
    sig = inspect.signature(kifs.GraphicState.render_accumulate)
    assert sig.parameters["jitter"].default is None
    assert len(kifs.GraphicState.KERNEL_NAMES) == 10  # the call reports KIFS_KERNEL_ACCUMULATE: no new value
    assert callable(configs.grid_cells) and callable(configs.jitter_cells)


def test_render_tool_offers_the_jitter(kifs):
    p = subprocess.run([sys.executable, str(ROOT / "tools" / "render.py"), "--help"], capture_output=True, text=True,
                       timeout=120)
    assert p.returncode == 0, p.stderr
    assert "--jitter" in p.stdout


def test_every_pipeline_is_compiled_without_scratch_and_claimed_by_the_form_table(kifs):
    from geometry_cases import PIPELINES, cases
    from kernel_forms import JITTER_FORMS
    from test_kernel_form_coverage import RENDER  # the form table's own pattern
    report = kernel_report()
    names = [n for n in report if "kifs::accum::jitter_render_kernel<" in n]
    assert len(names) == len(PIPELINES) == 10, names
    assert all(RENDER.search(n) for n in names) and sorted(names) == sorted(JITTER_FORMS)
    assert len([n for n in report if "kifs::accum::render_kernel<" in n]) == 10  # the unjittered kernel keeps its ten
    for n in names:
        r = report[n]
        assert int(r["ScratchSize [bytes/lane]"]) == 0 and int(r["VGPRs Spill"]) == 0 and r.get("Dynamic Stack") == "False", (n, r)
    got = sorted(re.search(r"jitter_render_kernel<(\d+), (\d+)>", n).groups() for n in names)
    want = []
    for pipeline, (_, _, gui, iters) in cases(kifs, 64, 48).items():
        u = gui.into_buffer_data()
        group, prim = int(u.fractal_group_id), int(u.primitive_id)
        pair = (1, int(iters[0] <= 24)) if group == 1 else (2, 0) if group == 2 else (0, min(prim, 6))
        want.append(tuple(str(v) for v in pair))
    assert sorted(want) == got and len(set(want)) == 10
