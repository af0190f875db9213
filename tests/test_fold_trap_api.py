"""Orbit-trap colouring of folded scenes (kifs_render_folded_trapped_async, kifs_eval_fold_trap), the parts a machine
without a GPU can check: the header's text, the record's and the kernel argument's sizes and offsets, the ctypes binding,
the Python layer's signatures, that the "deliberately absent" lists no longer name the composition, the render tool's
routing, the refusals that need no device, and that hipcc compiled
foldorbit::render_kernel for every KIFS primitive and the two evaluation kernels without scratch memory."""
import ctypes as C
import inspect
import re
import subprocess
from pathlib import Path

from kernel_report import kernel_report

ROOT = Path(__file__).resolve().parent.parent
HEADER = (ROOT / "include" / "kifs_hip.h").read_text()
BAD_ARG = 7


def test_header_declares_the_folded_trapped_surface():
    flat = re.sub(r"\s+", " ", re.sub(r"/\*.*?\*/", "", HEADER, flags=re.S))
    assert ("int kifs_render_folded_trapped_async(kifs_ctx* ctx, void* hip_stream, int count, const KifsCameraUniform* cameras, "
            "uint8_t* const* dev_outs_rgba8, size_t pitch_bytes, const KifsFoldSystem* fold, const KifsOrbitTrap* trap, "
            "const KifsLight* light , const KifsAmbientOcclusion* ao , float* dev_trap_u , size_t u_pitch_bytes, "
            "size_t u_stride_bytes, int y0, int y1, int encode);") in flat
    assert ("int kifs_eval_fold_trap(kifs_ctx* ctx, const KifsFoldSystem* fold, const KifsOrbitTrap* trap, const float* points_xyz, "
            "int n, float* u_out);") in flat
    assert re.search(r"^#define KIFS_MAX_FOLD_TRAP_BATCH 64$", HEADER, re.M)
    assert re.search(r"^#define KIFS_ABI_VERSION 4$", HEADER, re.M)
    start = HEADER.index("extension: orbit-trap colouring of folded scenes")
    assert HEADER.index("extension: kaleidoscopic IFS scenes") < start  # after the two calls it joins
    block = HEADER[start:HEADER.index("#define KIFS_MAX_FOLD_TRAP_BATCH")]
    for word in ("orbit", "distance", "colour", "frame", "plane", "identity", "refusals", "scope"):  # the contract's paragraphs
        assert re.search(rf"^ \*   {word}\b", block, re.M), word
    for text in ("z_0 = (p.x, p.y, p.z, 0)", "z_{j+1} = (p after MIRROR_Z, 0)", "k <= K", "K_b = max(K - N, 0)", "(d < m) ? d : m",
                 "u = sqrt(m)", "A miss stores +inf", "k > 1 a plane is refused", "(a) scale = bias = 0", "fold->iterations == 0",
                 "kifs_eval_trap's values", "KIFS_ERR_RUNTIME and launches nothing", "tests/fold_trap_reference.c"):
        assert text in block, text


def test_the_composition_is_no_longer_listed_as_absent():
    trap_block = HEADER[HEADER.index("extension: orbit-trap surface colouring"):HEADER.index("#define KIFS_MAX_TRAP_ITERATIONS")]
    fold_block = HEADER[HEADER.index("extension: kaleidoscopic IFS scenes"):HEADER.index("#define KIFS_MAX_FOLD_ITERATIONS")]
    for block in (trap_block, fold_block):
        scope = block[block.index(" *   scope"):]
        absent = scope[:scope.index("(No longer absent")] if "(No longer absent" in scope else scope
        assert "a trap on a folded" not in absent
    assert "kifs_render_folded_trapped_async" in fold_block
    for name in ("DESIGN.md", "INTEGRATION.md", "README.md"):
        assert "kifs_render_folded_trapped_async" in (ROOT / name).read_text(), name
    assert "5.20" in (ROOT / "DESIGN.md").read_text()


def test_record_and_kernel_argument_sizes(tmp_path):
    """The record is fold::Fold, trap::Trap and padding, 128 bytes; foldorbit::Params is light::Params' fields at their
    offsets and the record pointer, the plane pointer and its pitch and stride behind them: 4024 + 24 = 4048 of the 4096
    bytes a kernel argument may have -- where the two records themselves would have made 4144."""
    src = tmp_path / "t.cpp"
    src.write_text('#include <cstddef>\n#include <cstdint>\n#include <cstdio>\n#include "kifs_params.hpp"\n'
                   'using namespace kifs;\n'
                   'int main(){std::printf("%zu %zu %zu %zu %zu %zu %zu %zu %zu %zu %zu %zu %zu %zu %zu %zu\\n", sizeof(light::Params), sizeof(fold::Fold), sizeof(trap::Trap),'
                   'sizeof(foldorbit::Record), offsetof(foldorbit::Record, fold), offsetof(foldorbit::Record, trap), sizeof(foldorbit::Params),'
                   'offsetof(foldorbit::Params, light) - offsetof(light::Params, light), offsetof(foldorbit::Params, ao) - offsetof(light::Params, ao),'
                   'offsetof(foldorbit::Params, has_ao) - offsetof(light::Params, has_ao), offsetof(foldorbit::Params, record), offsetof(foldorbit::Params, plane),'
                   'offsetof(foldorbit::Params, pitch_words), offsetof(foldorbit::Params, stride_words), sizeof(foldorbit::EvalParams), sizeof(BatchParams));}\n')
    exe = tmp_path / "t"
    subprocess.run(["g++", "-std=c++17", "-Wno-invalid-offsetof", f"-I{ROOT / 'kifs_raymarching_amd' / 'csrc'}", str(src), "-o", str(exe)], check=True)
    v = [int(x) for x in subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.split()]
    lit, fold, trap, rec, rf, rt, params, dl, da, dh, o_rec, o_plane, o_pitch, o_stride, ev, batch = v
    assert (lit, fold, trap, rec, rf, rt) == (4024, 64, 56, 128, 0, 64)
    assert lit + fold + trap > 4096  # why the records travel in device memory
    assert params == 4048 and (dl, da, dh) == (0, 0, 0) and (o_rec, o_plane, o_pitch, o_stride) == (4024, 4032, 4040, 4044)
    assert ev <= 4096
    assert rec <= 64 * 512  # a slot of the scene-table ring holds it


def test_library_exports_and_python_binds_it(kifs):
    from kifs_raymarching_amd import _lib
    from kifs_raymarching_amd._lib import LIB_PATH, SIGNATURES, AmbientOcclusionC, KifsFoldSystemC, KifsLightC, KifsOrbitTrapC, lib
    raw = C.CDLL(str(LIB_PATH))
    assert hasattr(raw, "kifs_render_folded_trapped_async") and hasattr(raw, "kifs_eval_fold_trap")
    res, args = SIGNATURES["kifs_render_folded_trapped_async"]
    assert res is C.c_int and len(args) == 16
    assert args[6] is C.POINTER(KifsFoldSystemC) and args[7] is C.POINTER(KifsOrbitTrapC) and args[8] is C.POINTER(KifsLightC)
    assert args[9] is C.POINTER(AmbientOcclusionC) and args[10] is C.c_void_p and args[11:13] == [C.c_size_t, C.c_size_t]
    assert args[13:] == [C.c_int, C.c_int, C.c_int]
    res, args = SIGNATURES["kifs_eval_fold_trap"]
    assert res is C.c_int and len(args) == 6 and args[1] is C.POINTER(KifsFoldSystemC) and args[2] is C.POINTER(KifsOrbitTrapC)
    assert args[4] is C.c_int
    assert _lib.MAX_FOLD_TRAP_BATCH == 64 and kifs.MAX_FOLD_TRAP_BATCH == 64 and "MAX_FOLD_TRAP_BATCH" in kifs.__all__
    assert lib.kifs_abi_version() == 4
    assert len(kifs.GraphicState.KERNEL_NAMES) == 10  # not a feedback launch: no new KifsKernel value
    sig = inspect.signature(kifs.GraphicState.render_folded_trapped_batch)
    assert list(sig.parameters)[:7] == ["self", "cameras", "fold", "trap", "light", "ao", "u_plane"]
    assert sig.parameters["light"].default is None and sig.parameters["ao"].default is None and sig.parameters["u_plane"].default is False
    sig = inspect.signature(kifs.GraphicState.render_folded_trapped)
    assert list(sig.parameters)[:6] == ["self", "fold", "trap", "light", "ao", "u_plane"]
    assert list(inspect.signature(kifs.GraphicState.eval_fold_trap).parameters)[:4] == ["self", "fold", "trap", "points"]


def test_refusals_that_need_no_device(kifs):
    """A NULL context, system, trap or array is refused before anything touches a device."""
    from kifs_raymarching_amd._lib import lib
    f, t = kifs.FoldSystem(stages=("abs",), iterations=2).into_buffer_data(), kifs.OrbitTrap().into_buffer_data()
    outs = (C.c_void_p * 1)(16)
    call = lib.kifs_render_folded_trapped_async
    assert call(None, None, 1, None, outs, 64, C.byref(f), C.byref(t), None, None, None, 0, 0, 0, 4, 1) == BAD_ARG
    import numpy as np
    p, u = np.zeros(3, dtype=np.float32), np.zeros(1, dtype=np.float32)
    fp = lambda a: a.ctypes.data_as(C.POINTER(C.c_float))
    assert lib.kifs_eval_fold_trap(None, C.byref(f), C.byref(t), fp(p), 1, fp(u)) == BAD_ARG


def test_the_render_tool_takes_fold_and_trap_together():
    text = (ROOT / "tools" / "render.py").read_text()
    assert "render_folded_trapped_batch(cams, fold, trap" in text and "u_plane=True" in text
    assert "--morph-to and --trap" not in text.split("if args.fold is not None:")[1].split("elif args.fold_rotate")[0]
    assert "--ao-png goes without --fold" in text  # still refused


def test_every_instantiation_is_compiled_without_scratch():
    report = kernel_report()
    names = [n for n in report if "foldorbit::render_kernel<" in n]
    pairs = sorted(tuple(int(v) for v in re.search(r"render_kernel<(\d+), (\d+)>", n).groups()) for n in names)
    assert pairs == [(0, p) for p in range(7)], pairs  # the six primitives and the unknown id; no Julia form
    evals = sorted(n for n in report if "foldorbit::eval_kernel<" in n)
    assert len(evals) == 2 and all(re.search(r"eval_kernel<(0|4)>", n) for n in evals), evals  # the orbit alone: no base estimate
    for n in names + evals:
        r = report[n]
        assert int(r["ScratchSize [bytes/lane]"]) == 0 and int(r["VGPRs Spill"]) == 0 and r.get("Dynamic Stack") == "False", (n, r)
    for n in evals:
        r = report[n]
        assert int(r["VGPRs"]) <= 64 and int(r["Occupancy [waves/SIMD]"]) >= 8 and int(r["SGPRs Spill"]) == 0, (n, r)
    for n in names:
        g, p = (int(v) for v in re.search(r"render_kernel<(\d+), (\d+)>", n).groups())
        # (the bunny's estimate leaves few scalar registers: its build parks the two that fold::render_kernel<0, 5> parks)
        assert int(report[n]["SGPRs Spill"]) <= (2 if p == 5 else 0), (n, report[n])
