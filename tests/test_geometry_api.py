"""The geometry output (kifs_render_geometry_async), the parts a machine without a GPU can check: the ABI surface, the
Python and CLI surface, and that hipcc compiled geom::render_kernel for every pipeline under a name the kernel-form
table's pattern does not claim."""
import re
import subprocess
import sys
from pathlib import Path

from kernel_report import kernel_report

ROOT = Path(__file__).resolve().parent.parent
HEADER = (ROOT / "include" / "kifs_hip.h").read_text()


def test_header_declares_the_geometry_surface():
    flat = re.sub(r"\s+", " ", re.sub(r"/\*.*?\*/", "", HEADER, flags=re.S))
    assert ("int kifs_render_geometry_async(kifs_ctx* ctx, void* hip_stream, int count, const KifsCameraUniform* cameras, "
            "uint8_t* const* dev_outs_rgba8, size_t pitch_bytes, float* dev_geometry, size_t geometry_pitch_bytes, "
            "size_t geometry_stride_bytes, int y0, int y1, int encode);") in flat
    assert re.search(r"KIFS_KERNEL_GEOMETRY = 6\b", HEADER)
    assert re.search(r"^#define KIFS_ABI_VERSION 4$", HEADER, re.M)


def test_library_exports_and_python_binds_it(kifs):
    import ctypes as C
    from kifs_raymarching_amd._lib import LIB_PATH, SIGNATURES, lib
    assert hasattr(C.CDLL(str(LIB_PATH)), "kifs_render_geometry_async")
    res, args = SIGNATURES["kifs_render_geometry_async"]
    assert res is C.c_int and len(args) == 12
    assert lib.kifs_abi_version() == 4
    assert lib.kifs_render_geometry_async(None, None, 1, None, None, 0, None, 0, 0, 0, 0, 1) == 7  # BAD_ARG, no crash
    assert callable(getattr(kifs.GraphicState, "render_geometry", None))
    assert callable(getattr(kifs.GraphicState, "render_geometry_batch", None))
    assert kifs.GraphicState.KERNEL_NAMES[6] == "render_geometry_kernel"


def test_render_tool_offers_geometry(kifs):
    p = subprocess.run([sys.executable, str(ROOT / "tools" / "render.py"), "--help"], capture_output=True, text=True,
                       timeout=120)
    assert p.returncode == 0, p.stderr
    assert "--geometry" in p.stdout


def test_every_pipeline_is_compiled_and_claimed_in_the_form_table():
    names = [n for n in kernel_report() if "kifs::geom::render_kernel<" in n]
    got = sorted(re.search(r"render_kernel<(\d+), (\d+)>", n).groups() for n in names)
    want = sorted([("1", "0"), ("1", "1"), ("2", "0")] + [("0", str(p)) for p in range(7)])
    # ten: what launch_ssaa covers -- two Julia variants, the generalised Julia set, six primitives, PRIM_OTHER
    assert got == want and len(names) == 10, names
    from kernel_forms import GEOMETRY_FORMS
    from test_kernel_form_coverage import RENDER  # the form table's own pattern
    assert all(RENDER.search(n) for n in names) and sorted(names) == sorted(GEOMETRY_FORMS)
