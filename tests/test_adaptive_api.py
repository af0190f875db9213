"""The surface of adaptive anti-aliasing (kifs_render_adaptive_async) without a GPU: the header declares it, the ABI
version did not move, the library exports it and a null context is refused before any device is touched."""
import ctypes as C
import re
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
HEADER = (ROOT / "include" / "kifs_hip.h").read_text()


def test_header_declares_the_function_and_the_struct():
    body = re.sub(r"/\*.*?\*/", "", HEADER, flags=re.S)
    assert re.search(r"\bint\s+kifs_render_adaptive_async\s*\(\s*kifs_ctx\s*\*", body)
    m = re.search(r"typedef\s+struct\s+KifsAdaptiveAA\s*\{(.*?)\}\s*KifsAdaptiveAA\s*;", body, flags=re.S)
    assert m
    fields = [f.strip() for f in m.group(1).split(";") if f.strip()]
    assert fields == ["int32_t factor", "float normal_cos", "float depth_rel"]


def test_abi_version_is_still_4(kifs):
    from kifs_raymarching_amd._lib import lib
    assert re.search(r"^#define KIFS_ABI_VERSION 4$", HEADER, flags=re.M)
    assert lib.kifs_abi_version() == 4


def test_kernel_enum_value():
    body = re.sub(r"/\*.*?\*/", "", HEADER, flags=re.S)
    assert re.search(r"\bKIFS_KERNEL_ADAPTIVE\s*=\s*7\b", body)
    assert re.search(r"\bKIFS_KERNEL_GEOMETRY\s*=\s*6\b", body)


def test_library_exports_the_symbol_with_a_signature(kifs):
    from kifs_raymarching_amd._lib import LIB_PATH, SIGNATURES, AdaptiveAAC
    assert hasattr(C.CDLL(str(LIB_PATH)), "kifs_render_adaptive_async")
    assert "kifs_render_adaptive_async" in SIGNATURES
    assert C.sizeof(AdaptiveAAC) == 12
    assert kifs.GraphicState.KERNEL_NAMES[7] == "render_adaptive_kernel"
    assert callable(kifs.GraphicState.render_adaptive) and callable(kifs.GraphicState.render_adaptive_batch)


def test_null_arguments_are_refused_without_a_device(kifs):
    from kifs_raymarching_amd._lib import lib, AdaptiveAAC
    aa = AdaptiveAAC(2, 0.9, 0.05)
    outs = (C.c_void_p * 1)(64)
    assert lib.kifs_render_adaptive_async(None, None, 1, None, outs, 64, C.byref(aa), None, 1) == 7
