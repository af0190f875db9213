"""Progressive accumulation (kifs_render_accumulate_resume_async), the parts a machine without a GPU can check: the ABI
surface, the Python and CLI surface, and that hipcc compiled accum::carry_render_kernel for every pipeline -- ten
instantiations, none with scratch, spills or a dynamic stack, their (GROUP, PRIM) pairs the ones geometry_cases.PIPELINES
dispatch to -- beside the twenty kernels of the two accumulated calls, which stay."""
import ctypes as C
import re
import subprocess
import sys
from pathlib import Path

from kernel_report import kernel_report

ROOT = Path(__file__).resolve().parent.parent
HEADER = (ROOT / "include" / "kifs_hip.h").read_text()


def test_header_declares_the_progressive_surface():
    flat = re.sub(r"\s+", " ", re.sub(r"/\*.*?\*/", "", HEADER, flags=re.S))
    assert ("int kifs_render_accumulate_resume_async(kifs_ctx* ctx, void* hip_stream, int count, int samples, "
            "const KifsCameraUniform* cameras, const KifsOptionsUniform* options, int grid, const KifsSubpixel* cells, "
            "float* dev_sums, size_t sums_pitch_bytes, size_t sums_stride_bytes, uint32_t prior_samples, "
            "uint8_t* const* dev_outs_rgba8 , size_t pitch_bytes, int y0, int y1, int encode);") in flat
    assert re.search(r"^#define KIFS_MAX_PROGRESSIVE_SAMPLES 16777216u\b", HEADER, re.M)
    assert re.search(r"^#define KIFS_ABI_VERSION 4$", HEADER, re.M)
    assert re.search(r"KIFS_KERNEL_ACCUMULATE = 9\b", HEADER) and not re.search(r"KIFS_KERNEL_\w+ = 10\b", HEADER)
    for word in ("base", "plane", "fold", "picture", "identities", "refusals"):  # the contract's paragraphs
        assert re.search(rf"^ \*   {word}\b", HEADER, re.M), word


def test_library_exports_and_python_binds_it(kifs):
    import inspect
    from kifs_raymarching_amd import _lib, configs, graphics
    from kifs_raymarching_amd._lib import LIB_PATH, SIGNATURES, lib
    assert hasattr(C.CDLL(str(LIB_PATH)), "kifs_render_accumulate_resume_async")
    res, args = SIGNATURES["kifs_render_accumulate_resume_async"]
    assert res is C.c_int and len(args) == 17 and args[11] is C.c_uint32
    assert lib.kifs_abi_version() == 4
    assert lib.kifs_render_accumulate_resume_async(None, None, 1, 1, None, None, 1, None, None, 0, 0, 0, None, 0, 0, 0, 1) == 7
    assert _lib.MAX_PROGRESSIVE_SAMPLES == 1 << 24
    assert len(kifs.GraphicState.KERNEL_NAMES) == 10  # the call reports KIFS_KERNEL_ACCUMULATE: no new value
    sig = inspect.signature(kifs.GraphicState.render_accumulate_resume)
    assert list(sig.parameters)[1:5] == ["sums", "prior", "cameras", "samples"]
    assert sig.parameters["picture"].default is True and sig.parameters["jitter"].default is None
    assert sig.parameters["outs"].default is None and sig.parameters["options"].default is None
    assert kifs.Accumulator is graphics.Accumulator
    for name in ("add", "reset", "linear_mean"):
        assert callable(getattr(kifs.Accumulator, name))
    assert list(inspect.signature(kifs.Accumulator.__init__).parameters)[1:] == ["state", "count", "y0", "y1"]
    assert callable(configs.pass_splits)
    from kifs_raymarching_amd.viewer import ViewerSession
    assert inspect.signature(ViewerSession.__init__).parameters["refine"].default is None


def test_the_tools_offer_it(kifs):
    for tool, flag in (("render.py", "--spp"), ("view.py", "--refine")):
        p = subprocess.run([sys.executable, str(ROOT / "tools" / tool), "--help"], capture_output=True, text=True, timeout=120)
        assert p.returncode == 0, p.stderr
        assert flag in p.stdout, tool


def test_every_pipeline_is_compiled_without_scratch(kifs):
    from geometry_cases import PIPELINES, cases
    from test_kernel_form_coverage import RENDER  # the form table's own pattern: it claims the new family (kernel_forms.CARRY_FORMS)
    report = kernel_report()
    names = [n for n in report if "kifs::accum::carry_render_kernel<" in n]
    assert len(names) == len(PIPELINES) == 10, names
    assert all(RENDER.search(n) for n in names)
    assert len([n for n in report if "kifs::accum::render_kernel<" in n]) == 10  # the twenty existing names stay
    assert len([n for n in report if "kifs::accum::jitter_render_kernel<" in n]) == 10
    for n in names:
        r = report[n]
        assert int(r["ScratchSize [bytes/lane]"]) == 0 and int(r["VGPRs Spill"]) == 0 and r.get("Dynamic Stack") == "False", (n, r)
    got = sorted(re.search(r"carry_render_kernel<(\d+), (\d+)>", n).groups() for n in names)
    want = []
    for pipeline, (_, _, gui, iters) in cases(kifs, 64, 48).items():
        u = gui.into_buffer_data()
        group, prim = int(u.fractal_group_id), int(u.primitive_id)
        pair = (1, int(iters[0] <= 24)) if group == 1 else (2, 0) if group == 2 else (0, min(prim, 6))
        want.append(tuple(str(v) for v in pair))
    assert sorted(want) == got and len(set(want)) == 10


class _FakeState:
    """What Accumulator.add asks of its state, recorded: which of order_after and synchronize were called."""

    def __init__(self):
        self.calls = []

    def render_accumulate_resume(self, sums, prior, cameras, samples, stream=None, **kw):
        self.calls.append(("pass", prior, getattr(stream, "cuda_stream", stream)))
        return None

    def order_after(self, stream, producer):
        self.calls.append(("order_after", stream, producer))

    def synchronize(self):
        self.calls.append(("synchronize",))


class _Stream:
    def __init__(self, handle):
        self.cuda_stream = handle


def test_accumulator_orders_a_pass_after_the_previous_pass_on_another_stream(kifs):
    """No GPU: an Accumulator around a fake state.  Same stream: neither call; caller -> caller and caller -> own:
    kifs_order_after(new, last), no host wait; own -> caller: state.synchronize(), a host wait, because no handle names
    the context's own stream as a producer; after reset(): nothing, the stream is forgotten.  A torch stream and its raw
    handle are the same stream."""
    def accumulator():
        state = _FakeState()
        acc = kifs.Accumulator.__new__(kifs.Accumulator)  # (__init__ allocates the plane on a device)
        acc.state, acc.count, acc.y0, acc.y1, acc.sums = state, 1, 0, 8, None
        acc.reset()
        return acc, state

    cam = [kifs.CameraData()]
    A, B = 0x1000, 0x2000
    acc, st = accumulator()
    for stream in (_Stream(A), A, _Stream(A)):  # same stream, as an object and as a handle
        acc.add(cam, 1, stream=stream)
    assert st.calls == [("pass", 0, A), ("pass", 1, A), ("pass", 2, A)] and acc.total == 3
    acc, st = accumulator()
    acc.add(cam, 1, stream=None)
    acc.add(cam, 1)                       # own -> own
    assert st.calls == [("pass", 0, None), ("pass", 1, None)]
    acc, st = accumulator()
    acc.add(cam, 1, stream=_Stream(A))
    acc.add(cam, 1, stream=_Stream(B))    # caller -> caller
    acc.add(cam, 1, stream=None)          # caller -> own
    acc.add(cam, 1, stream=A)             # own -> caller
    acc.add(cam, 1, stream=A)
    assert st.calls == [("pass", 0, A), ("order_after", B, A), ("pass", 1, B), ("order_after", None, B), ("pass", 2, None),
                        ("synchronize",), ("pass", 3, A), ("pass", 4, A)]
    acc, st = accumulator()
    acc.add(cam, 1, stream=None)
    acc.reset()
    acc.add(cam, 1, stream=B)             # after reset(): the first pass again, ordered after nothing
    acc.add(cam, 1, stream=A)
    acc.reset()
    acc.add(cam, 1, stream=None)
    assert st.calls == [("pass", 0, None), ("pass", 0, B), ("order_after", A, B), ("pass", 1, A), ("pass", 0, None)]
