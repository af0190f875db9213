"""Converging accumulation (kifs_render_accumulate_converge_async), the parts a machine without a GPU can check: the ABI
surface and its refusals, the Python surface, and that hipcc compiled accum::converge_render_kernel for every pipeline --
ten instantiations, none with scratch, spills or a dynamic stack, their (GROUP, PRIM) pairs the ones
geometry_cases.PIPELINES dispatch to -- beside the thirty kernels of the three accumulated calls, which stay."""
import ctypes as C
import re
from pathlib import Path

from kernel_report import kernel_report

import converge_forms as CF

ROOT = Path(__file__).resolve().parent.parent
HEADER = (ROOT / "include" / "kifs_hip.h").read_text()
BAD_ARG = 7


def test_header_declares_the_converging_surface():
    flat = re.sub(r"\s+", " ", re.sub(r"/\*.*?\*/", "", HEADER, flags=re.S))
    assert ("int kifs_render_accumulate_converge_async(kifs_ctx* ctx, void* hip_stream, int count, int samples, "
            "const KifsCameraUniform* cameras, const KifsOptionsUniform* options, int grid, const KifsSubpixel* cells, "
            "float* dev_sums, size_t sums_pitch_bytes, size_t sums_stride_bytes, "
            "float* dev_moments, size_t moments_pitch_bytes, size_t moments_stride_bytes, "
            "int restart, const KifsConvergence* rule, uint32_t* dev_active_counts , "
            "uint8_t* const* dev_outs_rgba8 , size_t pitch_bytes, int y0, int y1, int encode);") in flat
    assert "typedef struct KifsConvergence { float tolerance; uint32_t min_samples; } KifsConvergence;" in flat
    assert re.search(r"^#define KIFS_ABI_VERSION 4$", HEADER, re.M)
    assert re.search(r"KIFS_KERNEL_ACCUMULATE = 9\b", HEADER) and not re.search(r"KIFS_KERNEL_\w+ = 10\b", HEADER)
    for word in ("base", "state", "rule", "pass", "picture", "counts", "identities", "refusals"):  # the contract's paragraphs
        assert re.search(rf"^ \*   {word}\b", HEADER, re.M), word
    # the rule is stated once, in the header's words
    for line in ("Y(c)       = (0.2126f*c.r + 0.7152f*c.g) + 0.0722f*c.b",
                 "L = Y(sum);  d = n*q - L*L;  b = (tolerance*tolerance) * ((n*n) * (n - 1.0f))",
                 "settled(p) = n >= float(min_samples)  &&  d <= b",
                 "active(p)  = !settled(p)  &&  n + float(samples) <= 16777216.0f"):
        assert HEADER.count(line) == 1, line
    assert "At tolerance 0 even identical samples need not settle" in HEADER


def test_library_exports_and_python_binds_it(kifs):
    import inspect
    from kifs_raymarching_amd import _lib, graphics
    from kifs_raymarching_amd._lib import LIB_PATH, SIGNATURES, KifsConvergence, lib
    assert hasattr(C.CDLL(str(LIB_PATH)), "kifs_render_accumulate_converge_async")
    res, args = SIGNATURES["kifs_render_accumulate_converge_async"]
    assert res is C.c_int and len(args) == 22 and args[14] is C.c_int
    assert C.sizeof(KifsConvergence) == 8 and KifsConvergence.tolerance.offset == 0 and KifsConvergence.min_samples.offset == 4
    assert lib.kifs_abi_version() == 4
    assert len(kifs.GraphicState.KERNEL_NAMES) == 10  # the call reports KIFS_KERNEL_ACCUMULATE: no new value
    sig = inspect.signature(kifs.GraphicState.render_accumulate_converge)
    assert list(sig.parameters)[1:8] == ["sums", "moments", "cameras", "samples", "rule", "restart", "counts"]
    assert sig.parameters["restart"].default is False and sig.parameters["counts"].default is None
    assert sig.parameters["picture"].default is True and sig.parameters["jitter"].default is None
    assert kifs.ConvergingAccumulator is graphics.ConvergingAccumulator and issubclass(kifs.ConvergingAccumulator, kifs.Accumulator)
    assert list(inspect.signature(kifs.ConvergingAccumulator.__init__).parameters)[1:] == ["state", "count", "y0", "y1", "tolerance",
                                                                                           "min_samples"]
    for name in ("add", "reset", "linear_mean", "active", "samples_per_pixel"):
        assert callable(getattr(kifs.ConvergingAccumulator, name))
    # the plain Accumulator is today's object
    assert list(inspect.signature(kifs.Accumulator.__init__).parameters)[1:] == ["state", "count", "y0", "y1"]
    assert not hasattr(kifs.Accumulator, "active")
    assert _lib.MAX_PROGRESSIVE_SAMPLES == 1 << 24


def test_refusals_without_a_device(kifs):
    """A null context is refused before anything else is looked at; every argument null with it."""
    from kifs_raymarching_amd._lib import KifsConvergence, lib
    rule = KifsConvergence(1 / 16, 4)
    assert lib.kifs_render_accumulate_converge_async(None, None, 1, 1, None, None, 1, None, None, 0, 0, None, 0, 0, 0, None, None, None,
                                                     0, 0, 0, 1) == BAD_ARG
    assert lib.kifs_render_accumulate_converge_async(None, None, 1, 1, None, None, 1, None, None, 0, 0, None, 0, 0, 1, C.byref(rule), None,
                                                     None, 0, 0, 0, 1) == BAD_ARG


class _FakeState:
    def __init__(self):
        self.calls = []

    def render_accumulate_converge(self, sums, moments, cameras, samples, rule, restart=False, counts=None, stream=None, **kw):
        self.calls.append(("pass", bool(restart), rule, getattr(stream, "cuda_stream", stream)))
        return None

    def order_after(self, stream, producer):
        self.calls.append(("order_after", stream, producer))

    def synchronize(self):
        self.calls.append(("synchronize",))


def test_converging_accumulator_restarts_after_reset_and_orders_streams(kifs):
    """No GPU: a ConvergingAccumulator around a fake state.  The first pass after reset() restarts; passes on other streams
    are ordered as Accumulator orders them; total counts the sub-frames offered."""
    state = _FakeState()
    acc = kifs.ConvergingAccumulator.__new__(kifs.ConvergingAccumulator)  # (__init__ allocates the planes on a device)
    acc.state, acc.count, acc.y0, acc.y1, acc.sums, acc.moments, acc.counts = state, 1, 0, 8, None, None, None
    acc.tolerance, acc.min_samples = 0.25, 6
    acc.reset()
    cam = [kifs.CameraData()] * 2
    A = 0x1000
    acc.add(cam, 2)
    acc.add(cam, 2, stream=A)
    acc.add(cam, 2, stream=A)
    acc.reset()
    acc.add(cam, 2, stream=A)
    acc.add(cam, 2)
    rule = (0.25, 6)
    assert state.calls == [("pass", True, rule, None), ("synchronize",), ("pass", False, rule, A), ("pass", False, rule, A),
                           ("pass", True, rule, A), ("order_after", None, A), ("pass", False, rule, None)]
    assert acc.total == 4


def test_every_pipeline_is_compiled_without_scratch(kifs):
    from geometry_cases import PIPELINES, cases
    from test_kernel_form_coverage import RENDER  # the form table's pattern must NOT claim the new family
    report = kernel_report()
    names = [n for n in report if "kifs::accum::converge_render_kernel<" in n]
    assert len(names) == len(PIPELINES) == 10, names
    assert sorted(names) == sorted(CF.CONVERGE_FORMS)
    assert not any(RENDER.search(n) for n in names)
    for family in ("render_kernel<", "jitter_render_kernel<", "carry_render_kernel<"):  # the thirty existing names stay
        assert len([n for n in report if f"kifs::accum::{family}" in n]) == 10, family
    for n in names:
        r = report[n]
        assert int(r["ScratchSize [bytes/lane]"]) == 0 and int(r["VGPRs Spill"]) == 0 and r.get("Dynamic Stack") == "False", (n, r)
    got = sorted(re.search(r"converge_render_kernel<(\d+), (\d+)>", n).groups() for n in names)
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
    (file, forms), = CF.CONVERGE_TESTS.items()
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
        assert re.search(r"\bconverge_render_kernel<(\d+), (\d+)>", name).groups() == tuple(str(v) for v in pair), (name, pipeline)
