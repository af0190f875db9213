"""Host-side mirror of the reference's scene model and `GraphicState`, over the C ABI.

Same names, argument meaning and error behaviour as the reference so that tests read
like the reference's own (paths under src/ of LesbianLemon/kifs-raymarching):

  FractalGroup, PrimitiveShape          data/scene.rs:4-45
  ScreenData, CameraData, GuiData       data.rs:51-160   (+ .into_buffer_data())
  GraphicState                          render/graphics.rs:25-326
      update_screen_data / zoom_camera / rotate_camera / update_options / render

All arithmetic happens in the library (C++ host model, HIP kernels); this file only
moves bytes.  PyTorch, when used, is plumbing: tensors give device memory and streams.
"""
import ctypes as C
from dataclasses import dataclass, field
from enum import IntEnum

import numpy as np

from . import _lib

MAX_BATCH = 512  # KIFS_MAX_BATCH of include/kifs_hip.h
SPARSE_RECORD_BYTES = 1040  # KIFS_SPARSE_RECORD_BYTES
STRIPE_ROWS = 8  # KIFS_STRIPE_ROWS
ANIMATION_RING = 4  # KIFS_ANIMATION_RING
MAX_ACCUMULATE = 64  # KIFS_MAX_ACCUMULATE
MAX_JITTER_GRID = _lib.MAX_JITTER_GRID  # KIFS_MAX_JITTER_GRID
from ._lib import (AdaptiveAAC, AmbientOcclusionC, KifsLightC, KifsOrbitTrapC, KifsFoldSystemC, CameraDataC, CameraUniform, ExtensionsC, GuiDataC, KifsError, KifsSubpixel, OptionsUniform,
                   ScreenUniform, check, lib)

ENCODE_UNORM = _lib.ENCODE_UNORM
ENCODE_SRGB = _lib.ENCODE_SRGB


class FractalGroup(IntEnum):  # data/scene.rs:4-11
    KaleidoscopicIFS = 0
    JuliaSet = 1
    GeneralizedJuliaSet = 2

    @classmethod
    def from_id(cls, i):
        try:
            return cls(i)
        except ValueError:
            return None


class PrimitiveShape(IntEnum):  # data/scene.rs:35-45
    Sphere = 0
    Cylinder = 1
    Box = 2
    Torus = 3
    SierpinskiTetrahedron = 4
    Bunny = 5

    @classmethod
    def from_id(cls, i):
        try:
            return cls(i)
        except ValueError:
            return None


@dataclass
class ScreenData:  # data.rs:51-55
    width: int = 0
    height: int = 0

    def into_buffer_data(self) -> ScreenUniform:  # data.rs:66-81
        u = ScreenUniform()
        check(lib.kifs_host_screen(self.width, self.height, C.byref(u)), "ScreenData")
        return u


@dataclass
class CameraData:  # data.rs:83-113
    origin_distance: float = 5.0
    min_distance: float = 2.0
    phi: float = 0.0    # angles.0
    theta: float = 0.0  # angles.1

    def _c(self) -> CameraDataC:
        return CameraDataC(self.origin_distance, self.min_distance, self.phi, self.theta)

    def _take(self, c: CameraDataC):
        self.origin_distance, self.min_distance = c.origin_distance, c.min_distance
        self.phi, self.theta = c.phi, c.theta

    def camera_matrix(self) -> np.ndarray:
        """3x3, element [r, c]; columns are the camera basis (data.rs:91-98)."""
        m = (C.c_float * 9)()
        c = self._c()
        lib.kifs_host_camera_matrix(C.byref(c), m)
        return np.array(m[:], dtype=np.float32).reshape(3, 3).T.copy()

    def into_buffer_data(self) -> CameraUniform:  # data.rs:115-129
        u = CameraUniform()
        c = self._c()
        check(lib.kifs_host_camera(C.byref(c), C.byref(u)), "CameraData")
        return u


@dataclass
class GuiData:  # data.rs:131-160 (defaults = GuiData::default)
    max_iterations: int = 256
    max_distance: float = 1000.0
    epsilon: float = 0.0001
    fractal_color: tuple = (200, 200, 200)
    background_color: tuple = (0, 0, 0)
    is_heatmap: bool = False
    fractal_group: FractalGroup = FractalGroup.KaleidoscopicIFS
    primitive_shape: PrimitiveShape = PrimitiveShape.Sphere
    power: float = 2.0
    constant: tuple = (-0.1, 0.6, 0.9, -0.3)

    def into_buffer_data(self) -> OptionsUniform:
        """OptionsData::from(GuiData).into_buffer_data() (data.rs:176-220)."""
        g = GuiDataC()
        g.max_iterations = int(self.max_iterations)
        g.max_distance = self.max_distance
        g.epsilon = self.epsilon
        g.fractal_color = (C.c_uint8 * 3)(*self.fractal_color)
        g.background_color = (C.c_uint8 * 3)(*self.background_color)
        g.is_heatmap = 1 if self.is_heatmap else 0
        g.fractal_group = int(self.fractal_group)
        g.primitive_shape = int(self.primitive_shape)
        g.power = self.power
        g.constant = (C.c_float * 4)(*self.constant)
        u = OptionsUniform()
        check(lib.kifs_host_options(C.byref(g), C.byref(u)), "GuiData")
        return u


@dataclass
class AmbientOcclusion:  # KifsAmbientOcclusion: the term of kifs_render_occlusion_async
    samples: int = 5       # probes along the normal, 1..KIFS_MAX_AO_SAMPLES
    step: float = 0.02     # their spacing, scene units
    decay: float = 0.75    # weight of probe i + 1 over probe i, (0, 1]
    strength: float = 4.0  # >= 0; 0: the plain frame

    def into_buffer_data(self) -> AmbientOcclusionC:
        return AmbientOcclusionC(int(self.samples), float(self.step), float(self.decay), float(self.strength))


@dataclass
class Light:  # KifsLight: the light of kifs_render_lit_async; the defaults are the reference's light, no highlight
    direction: tuple = (1.0, 1.0, 1.0)     # towards the light; as given in the direct term, normalised for shadow and highlight
    ambient: float = 0.1                   # >= 0
    diffuse: float = 0.9                   # >= 0
    specular: tuple = (0.0, 0.0, 0.0)      # linear RGB weight of the highlight, >= 0; all zero: none
    shininess_log2: int = 5                # the Blinn-Phong exponent is 2 ** shininess_log2, 0..KIFS_MAX_SHININESS_LOG2

    def into_buffer_data(self) -> KifsLightC:
        return KifsLightC((C.c_float * 3)(*[float(v) for v in self.direction]), float(self.ambient), float(self.diffuse),
                          (C.c_float * 3)(*[float(v) for v in self.specular]), int(self.shininess_log2))


@dataclass
class OrbitTrap:  # KifsOrbitTrap: the trap of kifs_render_trapped_async; the gradient's first stop is the options' fractal_color
    centre: tuple = (0.0, 0.0, 0.0, 0.0)   # the trap point in orbit space (x, y, z, w)
    axes: int = 15                         # bit i set: component i takes part in the distance; 15: a point, one bit: a plane
    iterations: int = 8                    # orbit points after the hit point's own, 0..KIFS_MAX_TRAP_ITERATIONS
    scale: float = 1.0                     # t = clamp(scale * u + bias): configs.trap_range(lo, hi) makes the pair
    bias: float = 0.0
    mid: tuple = (255, 140, 0)             # sRGB bytes like GuiData's colours: the stop at t = 1/2
    far: tuple = (20, 60, 200)             # ... and at t = 1

    def into_buffer_data(self) -> KifsOrbitTrapC:
        """The record the library takes; refuses here what it would refuse.  The colours go through the conversion the
        options' colours go through (kifs_host_options)."""
        centre = [float(v) for v in self.centre]
        if len(centre) != 4 or not all(np.isfinite(centre)):
            raise ValueError("OrbitTrap: centre is four finite numbers (x, y, z, w)")
        if int(self.axes) != self.axes or not 1 <= int(self.axes) <= 15:
            raise ValueError("OrbitTrap: axes is a mask of the components x = 1, y = 2, z = 4, w = 8: 1..15")
        if int(self.iterations) != self.iterations or not 0 <= int(self.iterations) <= _lib.MAX_TRAP_ITERATIONS:
            raise ValueError(f"OrbitTrap: 0..{_lib.MAX_TRAP_ITERATIONS} iterations")
        if not all(abs(float(v)) <= 3.4028234663852886e38 for v in (self.scale, self.bias)):  # (false for a NaN)
            raise ValueError("OrbitTrap: scale and bias are finite in float32")
        for name in ("mid", "far"):
            v = getattr(self, name)
            if len(v) != 3 or any(int(b) != b or not 0 <= int(b) <= 255 for b in v):
                raise ValueError(f"OrbitTrap: {name} is three sRGB bytes")
        g = GuiDataC()
        lib.kifs_host_gui_default(C.byref(g))
        g.fractal_color = (C.c_uint8 * 3)(*[int(b) for b in self.mid])
        g.background_color = (C.c_uint8 * 3)(*[int(b) for b in self.far])
        u = OptionsUniform()
        check(lib.kifs_host_options(C.byref(g), C.byref(u)), "OrbitTrap")
        return KifsOrbitTrapC((C.c_float * 4)(*centre), int(self.axes), int(self.iterations), float(self.scale), float(self.bias),
                              (C.c_float * 3)(*u.fractal_color), (C.c_float * 3)(*u.background_color))


_F32_MAX = 3.4028234663852886e38


@dataclass
class FoldSystem:  # KifsFoldSystem: the fold system of kifs_render_folded_async; the defaults fold nothing (iterations 0)
    stages: object = 0                      # a mask of KifsFoldStage bits, or names: "abs", "sort", "tetra", "rotate", "mirror_z"
    iterations: int = 0                     # rounds of fold, rotate and scale, 0..KIFS_MAX_FOLD_ITERATIONS
    scale: float = 2.0                      # 1..16
    offset: tuple = (1.0, 1.0, 1.0)         # the fixed point of the scaling
    rotation: tuple = (1.0, 0.0, 0.0, 0.0, 1.0, 0.0, 0.0, 0.0, 1.0)  # row-major 3 x 3, used as given; read only with "rotate"

    def stage_bits(self) -> int:
        if isinstance(self.stages, str):
            names = [n for n in self.stages.replace("|", ",").replace("+", ",").split(",") if n.strip()]
        elif isinstance(self.stages, (list, tuple, set, frozenset)):
            names = list(self.stages)
        else:
            if int(self.stages) != self.stages or not 0 <= int(self.stages) <= 31:
                raise ValueError("FoldSystem: stages is a mask 0..31 or stage names")
            return int(self.stages)
        bits = 0
        for n in names:
            key = str(n).strip().lower()
            if key not in _lib.FOLD_STAGES:
                raise ValueError(f"FoldSystem: unknown stage {n!r}; one of {sorted(_lib.FOLD_STAGES)}")
            bits |= _lib.FOLD_STAGES[key]
        return bits

    def into_buffer_data(self) -> KifsFoldSystemC:
        """The record the library takes; refuses here what it would refuse."""
        bits = self.stage_bits()
        if int(self.iterations) != self.iterations or not 0 <= int(self.iterations) <= _lib.MAX_FOLD_ITERATIONS:
            raise ValueError(f"FoldSystem: 0..{_lib.MAX_FOLD_ITERATIONS} iterations")
        if not 1.0 <= float(np.float32(self.scale)) <= 16.0:  # (false for a NaN)
            raise ValueError("FoldSystem: scale is in [1, 16]")
        offset = [float(v) for v in self.offset]
        if len(offset) != 3 or not all(abs(v) <= _F32_MAX for v in offset):  # (false for a NaN)
            raise ValueError("FoldSystem: offset is three numbers finite in float32")
        rotation = [float(v) for v in np.asarray(self.rotation, dtype=np.float64).reshape(-1)]
        if len(rotation) != 9:
            raise ValueError("FoldSystem: rotation is a row-major 3 x 3 matrix")
        if (bits & _lib.FOLD_STAGES["rotate"]) and not all(abs(v) <= _F32_MAX for v in rotation):
            raise ValueError("FoldSystem: rotation is finite in float32")
        return KifsFoldSystemC(bits, int(self.iterations), float(self.scale), (C.c_float * 3)(*offset), (C.c_float * 9)(*rotation))


def uniform_bytes(u) -> bytes:
    """`bytemuck::bytes_of` of a uniform struct."""
    return bytes(memoryview(u).cast("B"))


class DevicePointers:
    """The destinations of a batch, prepared once: a C array of device pointers (and the tensors, kept alive).
    render_batch_async / render_shard_async take it in place of the list of tensors -- a step of a few hundred
    views otherwise spends as long collecting pointers on the host as the GPU spends rendering."""

    def __init__(self, outs):
        self.tensors = list(outs)
        self.array = (C.c_void_p * len(self.tensors))(*[_device_pointer(o) for o in self.tensors])

    def __len__(self):
        return len(self.tensors)

    def __getitem__(self, i):
        return self.tensors[i]


def camera_array(cameras):
    """A C array of CameraUniform images from CameraData objects / uniform images (prepared once per
    sequence of poses; the render calls take it in place of the list)."""
    if isinstance(cameras, C.Array):
        return cameras
    return (CameraUniform * len(cameras))(*[c.into_buffer_data() if hasattr(c, "into_buffer_data") else c
                                            for c in cameras])


def options_array(options):
    """A C array of OptionsUniform images from GuiData objects / uniform images (render_animation takes it in place of
    the list)."""
    if isinstance(options, C.Array):
        return options
    return (OptionsUniform * len(options))(*[o.into_buffer_data() if hasattr(o, "into_buffer_data") else o
                                             for o in options])


def _device_pointer(obj):
    if hasattr(obj, "data_ptr"):  # torch.Tensor
        return int(obj.data_ptr())
    return int(obj)


def _producer_stream(dest):
    """hipStream_t of torch's CURRENT stream on the device of `dest` (0 = the legacy default stream) when `dest` is
    a torch CUDA tensor -- the stream whatever produced the tensor (torch.zeros' fill kernel, a consumer's last read)
    was enqueued on, as far as this wrapper can know; None for raw pointers and host arrays."""
    if not getattr(dest, "is_cuda", False):
        return None
    import torch
    return int(torch.cuda.current_stream(dest.device).cuda_stream)


# ---- what the wrappers of the calls that carry a scene per view share (render_animation, render_accumulate*); `name`
# is the calling method's, for the message
def _accumulated_views(name, cameras, samples, per="per frame"):
    """The camera array of an accumulated call, its views and its output frames."""
    cams = camera_array(cameras)
    views = len(cams)
    if not 1 <= samples <= MAX_ACCUMULATE or not 1 <= views <= MAX_BATCH or views % samples:
        raise ValueError(f"{name}: 1..{MAX_ACCUMULATE} samples {per}, count * samples cameras, at most {MAX_BATCH} of them")
    return cams, views, views // samples


def _one_per_view(name, what, items, views):
    if items is not None and len(items) != views:
        raise ValueError(f"{name}: {len(items)} {what} for {views} cameras")
    return items


def _frame_outs(name, outs, n, rows, w, device):
    """`outs` (None: a new tensor) as the uint8 (n, rows, w, 4) destination, and the array of its frames' pointers."""
    import torch
    if outs is None:
        outs = torch.empty((n, rows, w, 4), dtype=torch.uint8, device=torch.device("cuda", device))
    if tuple(outs.shape) != (n, rows, w, 4) or outs.dtype != torch.uint8 or not outs.is_contiguous():
        raise ValueError(f"{name}: outs uint8 ({n}, {rows}, {w}, 4), contiguous")
    base, frame_bytes = _device_pointer(outs), rows * w * 4
    return outs, (C.c_void_p * n)(*[base + i * frame_bytes for i in range(n)])


def _jitter_cells(name, jitter, views, samples, centre=True):
    """(grid, cells) as the C calls take them.  `centre`: the rule of the resume and converge calls for cells None,
    which C takes only for the whole grid in order -- a grid of 1 then gets the pixel centre for every view."""
    grid, cells = (1, None) if jitter is None else jitter
    if cells is not None and not isinstance(cells, C.Array):
        cells = (KifsSubpixel * len(cells))(*[KifsSubpixel(int(i), int(j)) for i, j in cells])
    _one_per_view(name, "cells", cells, views)
    if centre and cells is None and samples != int(grid) * int(grid):
        if int(grid) != 1:
            raise ValueError(f"{name}: cells None needs samples == grid * grid")
        cells = (KifsSubpixel * views)()  # cell (0, 0) of the one-cell grid
    return int(grid), cells


class GraphicState:
    """render/graphics.rs:25-37.  Owns one library context bound to one HIP device."""

    def __init__(self, device: int = 0, screen_data: ScreenData = None,
                 camera_data: CameraData = None, gui_data: GuiData = None):
        st = C.c_int(0)
        self._ctx = lib.kifs_create(device, C.byref(st))
        if not self._ctx:
            raise KifsError(st.value, f"kifs_create(device={device})")
        self.device = device
        self.screen_data = ScreenData()
        self.camera_data = camera_data or CameraData()   # graphics.rs:194 CameraData::default
        self.gui_data = gui_data or GuiData()            # graphics.rs:200 GuiData::default
        self.camera_rotatable = False                    # graphics.rs:229
        self.iters = (100, 10, 10)
        self._upload_camera()
        self.update_options(self.gui_data)
        if screen_data is not None:
            self.update_screen_data(screen_data)

    # -- lifetime -------------------------------------------------------------------
    def close(self):
        if getattr(self, "_ctx", None):
            lib.kifs_destroy(self._ctx)
            self._ctx = None

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    # -- uniform updates (graphics.rs:262-308) ---------------------------------------
    def update_screen_data(self, new_screen_data: ScreenData):
        u = new_screen_data.into_buffer_data()
        check(lib.kifs_set_screen(self._ctx, C.byref(u)), "update_screen_data")
        self.screen_data = new_screen_data

    def _upload_camera(self):
        u = self.camera_data.into_buffer_data()
        check(lib.kifs_set_camera(self._ctx, C.byref(u)), "camera")

    def zoom_camera(self, distance: float):  # graphics.rs:268-278
        c = self.camera_data._c()
        check(lib.kifs_host_zoom(C.byref(c), distance))
        self.camera_data._take(c)
        self._upload_camera()

    def rotate_camera(self, delta_phi: float, delta_theta: float):  # graphics.rs:280-302
        if not self.camera_rotatable:
            return
        c = self.camera_data._c()
        check(lib.kifs_host_rotate(C.byref(c), delta_phi, delta_theta))
        self.camera_data._take(c)
        self._upload_camera()

    def mouse_motion(self, dx: float, dy: float):  # render.rs:255-270
        if not self.camera_rotatable:
            return
        c = self.camera_data._c()
        check(lib.kifs_host_mouse_motion(C.byref(c), dx, dy))
        self.camera_data._take(c)
        self._upload_camera()

    def enable_camera_rotation(self):
        self.camera_rotatable = True

    def disable_camera_rotation(self):
        self.camera_rotatable = False

    def is_camera_rotatable(self):
        return self.camera_rotatable

    def set_camera(self, camera_data: CameraData):
        self.camera_data = camera_data
        self._upload_camera()

    def update_options(self, new_options):
        """Accepts GuiData (converted like render.rs:320-321) or a packed OptionsUniform."""
        if isinstance(new_options, GuiData):
            self.gui_data = new_options
            u = new_options.into_buffer_data()
        else:
            u = new_options
        check(lib.kifs_set_options(self._ctx, C.byref(u)), "update_options")
        self._options_uniform = u

    def set_raw_uniforms(self, screen: ScreenUniform = None, camera: CameraUniform = None,
                         options: OptionsUniform = None):
        """Upload pre-packed byte images (what a Rust host would pass)."""
        if screen is not None:
            check(lib.kifs_set_screen(self._ctx, C.byref(screen)), "set_screen")
            self.screen_data = ScreenData(int(screen.width), int(screen.height))
        if camera is not None:
            check(lib.kifs_set_camera(self._ctx, C.byref(camera)), "set_camera")
        if options is not None:
            check(lib.kifs_set_options(self._ctx, C.byref(options)), "set_options")

    def set_iters(self, sdf_iters=100, normal_iters=10, fold_iters=10):
        check(lib.kifs_set_iters(self._ctx, sdf_iters, normal_iters, fold_iters), "set_iters")
        self.iters = (sdf_iters, normal_iters, fold_iters)

    def set_extensions(self, soft_shadow=False, shadow_steps=64, shadow_k=8.0, shadow_t0=0.02,
                       shadow_max_t=10.0):
        """Opt-in soft shadows (an extension; absent from the reference).  Off = reference shading."""
        e = ExtensionsC(1 if soft_shadow else 0, shadow_steps, shadow_k, shadow_t0, shadow_max_t)
        check(lib.kifs_set_extensions(self._ctx, C.byref(e)), "set_extensions")

    def set_supersampling(self, k: int = 1):
        """k x k supersampled anti-aliasing (an extension; the reference takes one sample per pixel): every render of
        this context averages k^2 samples per pixel in linear colour before the encode.  1 <= k <= 4; 1 = off."""
        check(lib.kifs_set_supersampling(self._ctx, int(k)), "set_supersampling")

    # -- render (graphics.rs:310-325) -----------------------------------------------------
    def _order_after_producer(self, dest, launch_stream):
        """The wrapper's stream rule for torch destinations: the library launches on non-blocking streams, which
        nothing orders after torch's current stream -- where the destination's fill, or its previous reader, sits.
        Every render entry point below therefore makes its launch stream (None = the context's) wait for an event
        recorded on torch's current stream of the destination's device (kifs_order_after: two HIP calls, nothing
        blocks the host; the same stream on both sides is a no-op).  A C caller does the same with kifs_order_after
        or orders its streams itself (include/kifs_hip.h); the reference has one queue (util/uniform.rs:23-35)."""
        producer = _producer_stream(dest)
        if producer is None or (launch_stream and producer == launch_stream):
            return
        check(lib.kifs_order_after(self._ctx, launch_stream, producer or None), "order_after")

    def order_after(self, stream, producer):
        """kifs_order_after on raw hipStream_t handles: the context's next work on `stream` (None: its own stream) runs
        after everything `producer` (a caller's stream) holds now.  Nothing blocks the host."""
        check(lib.kifs_order_after(self._ctx, stream or None, producer), "order_after")

    def render(self, out=None, y0: int = 0, y1: int = None, encode: int = ENCODE_SRGB,
               pitch_bytes: int = None):
        """Synchronous frame.  `out` None -> returns a (rows, W, 4) uint8 ndarray; an
        ndarray -> filled in place; a torch CUDA tensor (uint8, rows*W*4) -> written on
        the device."""
        w, h = self.screen_data.width, self.screen_data.height
        y1 = h if y1 is None else y1
        rows = max(y1 - y0, 0)
        if out is None:
            out = np.empty((rows, w, 4), dtype=np.uint8)
        pitch = pitch_bytes if pitch_bytes is not None else w * 4
        if isinstance(out, np.ndarray):
            _check_host_destination(out, rows, w, pitch)
            ptr = out.ctypes.data
        else:
            ptr = _device_pointer(out)
            self._order_after_producer(out, None)
        check(lib.kifs_render(self._ctx, ptr, pitch, y0, y1, encode), "render")
        return out

    def render_async(self, out, stream=None, y0: int = 0, y1: int = None,
                     encode: int = ENCODE_SRGB, pitch_bytes: int = None):
        """Enqueue on `stream` (int hipStream_t / torch stream / None = context stream)."""
        w, h = self.screen_data.width, self.screen_data.height
        y1 = h if y1 is None else y1
        pitch = pitch_bytes if pitch_bytes is not None else w * 4
        if stream is not None and hasattr(stream, "cuda_stream"):
            stream = stream.cuda_stream
            if not stream:
                # the C ABI reads a null hipStream_t as "the context's own stream"; the legacy
                # default stream has handle 0 and would silently end up there
                raise ValueError("render_async: pass a non-default torch.cuda.Stream "
                                 "(the null stream handle selects the context's stream)")
        self._order_after_producer(out, stream)
        check(lib.kifs_render_async(self._ctx, stream, _device_pointer(out), pitch, y0, y1,
                                    encode), "render_async")

    def render_batch_async(self, outs, cameras, stream=None, y0: int = 0, y1: int = None,
                           encode: int = ENCODE_SRGB, pitch_bytes: int = None):
        """One launch for len(outs) <= MAX_BATCH frames: frame i uses cameras[i] (CameraData or a
        CameraUniform image) and goes to the device tensor outs[i]; screen, options, iteration
        counts and extensions are the context's.  Enqueued on `stream` like render_async."""
        if len(outs) != len(cameras) or not (1 <= len(outs) <= MAX_BATCH):
            raise ValueError(f"render_batch_async: 1..{MAX_BATCH} frames, one camera each")
        w, h = self.screen_data.width, self.screen_data.height
        y1 = h if y1 is None else y1
        pitch = pitch_bytes if pitch_bytes is not None else w * 4
        if stream is not None and hasattr(stream, "cuda_stream"):
            stream = stream.cuda_stream
            if not stream:
                raise ValueError("render_batch_async: pass a non-default torch.cuda.Stream")
        n = len(outs)
        cams = camera_array(cameras)
        ptrs = outs.array if isinstance(outs, DevicePointers) else (C.c_void_p * n)(*[_device_pointer(o) for o in outs])
        self._order_after_producer(outs[0], stream)
        check(lib.kifs_render_batch_async(self._ctx, stream, n, cams, ptrs, pitch, y0, y1, encode),
              "render_batch_async")

    # ---- geometry output (kifs_render_geometry_async): colour plus (n.x, n.y, n.z, t) per pixel
    def render_geometry_batch(self, cameras=None, stream=None, y0: int = 0, y1: int = None, encode: int = ENCODE_SRGB,
                              colour=None, geometry=None):
        """One launch for len(cameras) <= MAX_BATCH frames (cameras None: one frame with the context's camera) that
        writes the frames AND their geometry planes.  Returns (colour, geometry): a uint8 (count, rows, W, 4) and a
        float32 (count, rows, W, 4) torch tensor on this context's device -- texel (n.x, n.y, n.z, t) on a hit,
        (0, 0, 0, +inf) on a miss.  `colour` / `geometry`: contiguous destination tensors of those shapes to reuse.
        Enqueued on `stream` like render_async; the caller synchronises before reading."""
        import torch
        w, h = self.screen_data.width, self.screen_data.height
        y1 = h if y1 is None else y1
        rows = max(y1 - y0, 0)
        n = 1 if cameras is None else len(cameras)
        if not 1 <= n <= MAX_BATCH:
            raise ValueError(f"render_geometry_batch: 1..{MAX_BATCH} frames")
        dev = torch.device("cuda", self.device)
        if colour is None:
            colour = torch.empty((n, rows, w, 4), dtype=torch.uint8, device=dev)
        if geometry is None:
            geometry = torch.empty((n, rows, w, 4), dtype=torch.float32, device=dev)
        if (tuple(colour.shape) != (n, rows, w, 4) or colour.dtype != torch.uint8 or not colour.is_contiguous()
                or tuple(geometry.shape) != (n, rows, w, 4) or geometry.dtype != torch.float32
                or not geometry.is_contiguous()):
            raise ValueError(f"render_geometry_batch: colour uint8 and geometry float32, both ({n}, {rows}, {w}, 4), contiguous")
        stream = self._stream_handle(stream, "render_geometry_batch")
        cams = None if cameras is None else camera_array(cameras)
        ptrs = (C.c_void_p * n)(*[_device_pointer(colour[i]) for i in range(n)])
        self._order_after_producer(colour, stream)
        self._order_after_producer(geometry, stream)
        check(lib.kifs_render_geometry_async(self._ctx, stream, n, cams, ptrs, w * 4, _device_pointer(geometry), w * 16,
                                             rows * w * 16, y0, y1, encode), "render_geometry")
        return colour, geometry

    def render_geometry(self, y0: int = 0, y1: int = None, encode: int = ENCODE_SRGB, stream=None):
        """The context's frame and its geometry plane, synchronously: (colour uint8 rows x W x 4, geometry float32
        rows x W x 4) torch tensors on this context's device; geometry[..., :3] is the normal, geometry[..., 3] is t
        (+inf on a miss)."""
        import torch
        colour, geometry = self.render_geometry_batch(None, stream=stream, y0=y0, y1=y1, encode=encode)
        if stream is None:
            self.synchronize()
        else:
            torch.cuda.synchronize(colour.device)
        return colour[0], geometry[0]

    # ---- ambient occlusion (kifs_render_occlusion_async): every hit attenuated, optionally the factors as a plane
    def render_occlusion_batch(self, cameras=None, ao: AmbientOcclusion = None, occlusion: bool = False, stream=None,
                               y0: int = 0, y1: int = None, encode: int = ENCODE_SRGB, colour=None, plane=None):
        """The frames of len(cameras) cameras (cameras None: one frame with the context's camera) with ambient
        occlusion `ao` (None: AmbientOcclusion()), the context's supersampling factor honoured.  Returns
        (colour, plane): a uint8 (count, rows, W, 4) torch tensor on this context's device and, with `occlusion`, a
        float32 (count, rows, W) one -- the factor of every hit, 1.0 on a miss (one sample per pixel only) -- else None.
        `colour` / `plane`: contiguous destination tensors of those shapes to reuse.  The library takes
        MAX_OCCLUSION_BATCH cameras per launch; more are fed to it that many at a time.  Enqueued on `stream` like
        render_async; the caller synchronises before reading."""
        import torch
        w, h = self.screen_data.width, self.screen_data.height
        y1 = h if y1 is None else y1
        rows = max(y1 - y0, 0)
        n = 1 if cameras is None else len(cameras)
        if n < 1:
            raise ValueError("render_occlusion_batch: at least one frame")
        dev = torch.device("cuda", self.device)
        if colour is None:
            colour = torch.empty((n, rows, w, 4), dtype=torch.uint8, device=dev)
        if tuple(colour.shape) != (n, rows, w, 4) or colour.dtype != torch.uint8 or not colour.is_contiguous():
            raise ValueError(f"render_occlusion_batch: colour uint8 ({n}, {rows}, {w}, 4), contiguous")
        if occlusion or plane is not None:
            if plane is None:
                plane = torch.empty((n, rows, w), dtype=torch.float32, device=dev)
            if tuple(plane.shape) != (n, rows, w) or plane.dtype != torch.float32 or not plane.is_contiguous():
                raise ValueError(f"render_occlusion_batch: plane float32 ({n}, {rows}, {w}), contiguous")
        term = (AmbientOcclusion() if ao is None else ao).into_buffer_data()
        stream = self._stream_handle(stream, "render_occlusion_batch")
        cams = None if cameras is None else camera_array(cameras)
        self._order_after_producer(colour, stream)
        if plane is not None:
            self._order_after_producer(plane, stream)
        step = _lib.MAX_OCCLUSION_BATCH
        base, frame_bytes = _device_pointer(colour), rows * w * 4  # (a plane of one f32 per pixel is as many bytes)
        planes = None if plane is None else _device_pointer(plane)
        for first in range(0, n, step):
            m = min(step, n - first)
            ptrs = (C.c_void_p * m)(*[base + (first + i) * frame_bytes for i in range(m)])
            part = None if cams is None else C.cast(C.byref(cams, first * C.sizeof(CameraUniform)), C.POINTER(CameraUniform))
            check(lib.kifs_render_occlusion_async(self._ctx, stream, m, part, ptrs, w * 4, C.byref(term),
                                                  None if planes is None else planes + first * frame_bytes, w * 4,
                                                  frame_bytes, y0, y1, encode), "render_occlusion")
        return colour, plane

    def render_occlusion(self, ao: AmbientOcclusion = None, occlusion: bool = False, y0: int = 0, y1: int = None,
                         encode: int = ENCODE_SRGB, stream=None):
        """The context's frame with ambient occlusion, synchronously: (colour uint8 rows x W x 4, plane float32
        rows x W or None) torch tensors on this context's device."""
        import torch
        colour, plane = self.render_occlusion_batch(None, ao=ao, occlusion=occlusion, stream=stream, y0=y0, y1=y1, encode=encode)
        if stream is None:
            self.synchronize()
        else:
            torch.cuda.synchronize(colour.device)
        return colour[0], None if plane is None else plane[0]

    # ---- a configurable light (kifs_render_lit_async): every hit shaded by `light`, optionally occluded
    def render_lit_batch(self, cameras, light: Light, ao: AmbientOcclusion = None, stream=None, y0: int = 0, y1: int = None,
                         encode: int = ENCODE_SRGB, colour=None):
        """The frames of len(cameras) cameras (cameras None: one frame with the context's camera) under `light`, with
        the ambient-occlusion term `ao` on top when one is given (None: none), the context's supersampling factor and
        soft-shadow extension honoured.  Returns a uint8 (count, rows, W, 4) torch tensor on this context's device;
        `colour`: a contiguous destination tensor of that shape to reuse.  The library takes MAX_LIGHT_BATCH cameras per
        launch; more are fed to it that many at a time.  Enqueued on `stream` like render_async; the caller synchronises
        before reading."""
        import torch
        w, h = self.screen_data.width, self.screen_data.height
        y1 = h if y1 is None else y1
        rows = max(y1 - y0, 0)
        n = 1 if cameras is None else len(cameras)
        if n < 1:
            raise ValueError("render_lit_batch: at least one frame")
        if colour is None:
            colour = torch.empty((n, rows, w, 4), dtype=torch.uint8, device=torch.device("cuda", self.device))
        if tuple(colour.shape) != (n, rows, w, 4) or colour.dtype != torch.uint8 or not colour.is_contiguous():
            raise ValueError(f"render_lit_batch: colour uint8 ({n}, {rows}, {w}, 4), contiguous")
        lit = light.into_buffer_data()
        term = None if ao is None else ao.into_buffer_data()
        stream = self._stream_handle(stream, "render_lit_batch")
        cams = None if cameras is None else camera_array(cameras)
        self._order_after_producer(colour, stream)
        step = _lib.MAX_LIGHT_BATCH
        base, frame_bytes = _device_pointer(colour), rows * w * 4
        for first in range(0, n, step):
            m = min(step, n - first)
            ptrs = (C.c_void_p * m)(*[base + (first + i) * frame_bytes for i in range(m)])
            part = None if cams is None else C.cast(C.byref(cams, first * C.sizeof(CameraUniform)), C.POINTER(CameraUniform))
            check(lib.kifs_render_lit_async(self._ctx, stream, m, part, ptrs, w * 4, C.byref(lit),
                                            None if term is None else C.byref(term), y0, y1, encode), "render_lit")
        return colour

    def render_lit(self, light: Light, ao: AmbientOcclusion = None, y0: int = 0, y1: int = None, encode: int = ENCODE_SRGB,
                   stream=None):
        """The context's frame under `light` (and `ao`), synchronously: a uint8 rows x W x 4 torch tensor on this
        context's device."""
        import torch
        colour = self.render_lit_batch(None, light, ao=ao, stream=stream, y0=y0, y1=y1, encode=encode)
        if stream is None:
            self.synchronize()
        else:
            torch.cuda.synchronize(colour.device)
        return colour[0]

    # ---- orbit-trap surface colouring (kifs_render_trapped_async): every hit coloured by `trap`, lit and optionally occluded
    def render_trapped_batch(self, cameras, trap: OrbitTrap, light: Light = None, ao: AmbientOcclusion = None, stream=None,
                             y0: int = 0, y1: int = None, encode: int = ENCODE_SRGB, colour=None):
        """The frames of len(cameras) cameras (cameras None: one frame with the context's camera) with every hit coloured
        by the orbit trap `trap`, under `light` (None: the reference's light) and with the ambient-occlusion term `ao` on
        top when one is given, the context's supersampling factor and soft-shadow extension honoured.  Returns a uint8
        (count, rows, W, 4) torch tensor on this context's device; `colour`: a contiguous destination tensor of that shape
        to reuse.  The library takes MAX_TRAP_BATCH cameras per launch; more are fed to it that many at a time.  Enqueued
        on `stream` like render_async; the caller synchronises before reading."""
        import torch
        w, h = self.screen_data.width, self.screen_data.height
        y1 = h if y1 is None else y1
        rows = max(y1 - y0, 0)
        n = 1 if cameras is None else len(cameras)
        if n < 1:
            raise ValueError("render_trapped_batch: at least one frame")
        if colour is None:
            colour = torch.empty((n, rows, w, 4), dtype=torch.uint8, device=torch.device("cuda", self.device))
        if tuple(colour.shape) != (n, rows, w, 4) or colour.dtype != torch.uint8 or not colour.is_contiguous():
            raise ValueError(f"render_trapped_batch: colour uint8 ({n}, {rows}, {w}, 4), contiguous")
        record = trap.into_buffer_data() if hasattr(trap, "into_buffer_data") else trap  # (or a KifsOrbitTrapC, linear colours)
        lit = None if light is None else light.into_buffer_data()
        term = None if ao is None else ao.into_buffer_data()
        stream = self._stream_handle(stream, "render_trapped_batch")
        cams = None if cameras is None else camera_array(cameras)
        self._order_after_producer(colour, stream)
        step = _lib.MAX_TRAP_BATCH
        base, frame_bytes = _device_pointer(colour), rows * w * 4
        for first in range(0, n, step):
            m = min(step, n - first)
            ptrs = (C.c_void_p * m)(*[base + (first + i) * frame_bytes for i in range(m)])
            part = None if cams is None else C.cast(C.byref(cams, first * C.sizeof(CameraUniform)), C.POINTER(CameraUniform))
            check(lib.kifs_render_trapped_async(self._ctx, stream, m, part, ptrs, w * 4, C.byref(record),
                                                None if lit is None else C.byref(lit),
                                                None if term is None else C.byref(term), y0, y1, encode), "render_trapped")
        return colour

    def render_trapped(self, trap: OrbitTrap, light: Light = None, ao: AmbientOcclusion = None, y0: int = 0, y1: int = None,
                       encode: int = ENCODE_SRGB, stream=None):
        """The context's frame coloured by `trap` (under `light`, with `ao`), synchronously: a uint8 rows x W x 4 torch
        tensor on this context's device."""
        import torch
        colour = self.render_trapped_batch(None, trap, light=light, ao=ao, stream=stream, y0=y0, y1=y1, encode=encode)
        if stream is None:
            self.synchronize()
        else:
            torch.cuda.synchronize(colour.device)
        return colour[0]

    def eval_trap(self, trap: OrbitTrap, points):
        """u -- the least distance of the orbit to the trap -- of (n, 3) positions with the context's options: (n,) float32.
        Only the trap's centre, axes and iterations are read: for parity tests and for choosing a range
        (configs.trap_range) from the positions a frame hits."""
        pts = np.ascontiguousarray(points, dtype=np.float32).reshape(-1, 3)
        n = pts.shape[0]
        u = np.empty(n, dtype=np.float32)
        record = trap.into_buffer_data() if hasattr(trap, "into_buffer_data") else trap
        fp = lambda a: a.ctypes.data_as(C.POINTER(C.c_float))
        check(lib.kifs_eval_trap(self._ctx, C.byref(record), fp(pts), n, fp(u)), "eval_trap")
        return u

    # ---- kaleidoscopic IFS scenes (kifs_render_folded_async): the base primitive seen through `fold`, lit and optionally occluded
    def render_folded_batch(self, cameras, fold: FoldSystem, light: Light = None, ao: AmbientOcclusion = None, stream=None,
                            y0: int = 0, y1: int = None, encode: int = ENCODE_SRGB, colour=None):
        """The frames of len(cameras) cameras (cameras None: one frame with the context's camera) of the context's KIFS
        primitive seen through the fold system `fold`, under `light` (None: the reference's light) and with the
        ambient-occlusion term `ao` on top when one is given, the context's supersampling factor and soft-shadow extension
        honoured.  Returns a uint8 (count, rows, W, 4) torch tensor on this context's device; `colour`: a contiguous
        destination tensor of that shape to reuse.  The library takes MAX_FOLD_BATCH cameras per launch; more are fed to
        it that many at a time.  Enqueued on `stream` like render_async; the caller synchronises before reading."""
        import torch
        w, h = self.screen_data.width, self.screen_data.height
        y1 = h if y1 is None else y1
        rows = max(y1 - y0, 0)
        n = 1 if cameras is None else len(cameras)
        if n < 1:
            raise ValueError("render_folded_batch: at least one frame")
        if colour is None:
            colour = torch.empty((n, rows, w, 4), dtype=torch.uint8, device=torch.device("cuda", self.device))
        if tuple(colour.shape) != (n, rows, w, 4) or colour.dtype != torch.uint8 or not colour.is_contiguous():
            raise ValueError(f"render_folded_batch: colour uint8 ({n}, {rows}, {w}, 4), contiguous")
        record = fold.into_buffer_data() if hasattr(fold, "into_buffer_data") else fold  # (or a KifsFoldSystemC)
        lit = None if light is None else light.into_buffer_data()
        term = None if ao is None else ao.into_buffer_data()
        stream = self._stream_handle(stream, "render_folded_batch")
        cams = None if cameras is None else camera_array(cameras)
        self._order_after_producer(colour, stream)
        step = _lib.MAX_FOLD_BATCH
        base, frame_bytes = _device_pointer(colour), rows * w * 4
        for first in range(0, n, step):
            m = min(step, n - first)
            ptrs = (C.c_void_p * m)(*[base + (first + i) * frame_bytes for i in range(m)])
            part = None if cams is None else C.cast(C.byref(cams, first * C.sizeof(CameraUniform)), C.POINTER(CameraUniform))
            check(lib.kifs_render_folded_async(self._ctx, stream, m, part, ptrs, w * 4, C.byref(record),
                                               None if lit is None else C.byref(lit),
                                               None if term is None else C.byref(term), y0, y1, encode), "render_folded")
        return colour

    def render_folded(self, fold: FoldSystem, light: Light = None, ao: AmbientOcclusion = None, y0: int = 0, y1: int = None,
                      encode: int = ENCODE_SRGB, stream=None):
        """The context's frame seen through `fold` (under `light`, with `ao`), synchronously: a uint8 rows x W x 4 torch
        tensor on this context's device."""
        import torch
        colour = self.render_folded_batch(None, fold, light=light, ao=ao, stream=stream, y0=y0, y1=y1, encode=encode)
        if stream is None:
            self.synchronize()
        else:
            torch.cuda.synchronize(colour.device)
        return colour[0]

    def eval_fold(self, fold: FoldSystem, points, sdf: bool = True, normal: bool = True):
        """(sdf, normal) -- the folded estimate, (n,) float32, and its normal, (n, 3) float32 -- of (n, 3) positions with
        the context's options; None for the one not asked for."""
        pts = np.ascontiguousarray(points, dtype=np.float32).reshape(-1, 3)
        n = pts.shape[0]
        d = np.empty(n, dtype=np.float32) if sdf else None
        nr = np.empty((n, 3), dtype=np.float32) if normal else None
        record = fold.into_buffer_data() if hasattr(fold, "into_buffer_data") else fold
        fp = lambda a: None if a is None else a.ctypes.data_as(C.POINTER(C.c_float))
        check(lib.kifs_eval_fold(self._ctx, C.byref(record), fp(pts), n, fp(d), fp(nr)), "eval_fold")
        return d, nr

    # ---- orbit-trap colouring of folded scenes (kifs_render_folded_trapped_async): the two above composed
    def render_folded_trapped_batch(self, cameras, fold: FoldSystem, trap: OrbitTrap, light: Light = None,
                                    ao: AmbientOcclusion = None, u_plane=False, stream=None, y0: int = 0, y1: int = None,
                                    encode: int = ENCODE_SRGB, colour=None):
        """The frames of len(cameras) cameras (cameras None: one frame with the context's camera) of the context's KIFS
        primitive seen through the fold system `fold`, every hit coloured by the orbit trap `trap` over the fold's own
        orbit, under `light` (None: the reference's light) and with the ambient-occlusion term `ao` on top when one is
        given, the context's supersampling factor and soft-shadow extension honoured.  `u_plane`: True, or a contiguous
        float32 (count, rows, W) torch tensor to reuse -- the trap distance u of every hit, +inf on a miss (one sample
        per pixel only).  Returns a uint8 (count, rows, W, 4) torch tensor on this context's device, or with a plane the
        pair (colour, plane); `colour`: a contiguous destination tensor of that shape to reuse.  The library takes
        MAX_FOLD_TRAP_BATCH cameras per launch; more are fed to it that many at a time.  Enqueued on `stream` like
        render_async; the caller synchronises before reading."""
        import torch
        w, h = self.screen_data.width, self.screen_data.height
        y1 = h if y1 is None else y1
        rows = max(y1 - y0, 0)
        n = 1 if cameras is None else len(cameras)
        if n < 1:
            raise ValueError("render_folded_trapped_batch: at least one frame")
        dev = torch.device("cuda", self.device)
        if colour is None:
            colour = torch.empty((n, rows, w, 4), dtype=torch.uint8, device=dev)
        if tuple(colour.shape) != (n, rows, w, 4) or colour.dtype != torch.uint8 or not colour.is_contiguous():
            raise ValueError(f"render_folded_trapped_batch: colour uint8 ({n}, {rows}, {w}, 4), contiguous")
        plane = None
        if u_plane is not None and u_plane is not False:
            plane = torch.empty((n, rows, w), dtype=torch.float32, device=dev) if u_plane is True else u_plane
            if tuple(plane.shape) != (n, rows, w) or plane.dtype != torch.float32 or not plane.is_contiguous():
                raise ValueError(f"render_folded_trapped_batch: u_plane float32 ({n}, {rows}, {w}), contiguous")
        system = fold.into_buffer_data() if hasattr(fold, "into_buffer_data") else fold  # (or a KifsFoldSystemC)
        record = trap.into_buffer_data() if hasattr(trap, "into_buffer_data") else trap  # (or a KifsOrbitTrapC, linear colours)
        lit = None if light is None else light.into_buffer_data()
        term = None if ao is None else ao.into_buffer_data()
        stream = self._stream_handle(stream, "render_folded_trapped_batch")
        cams = None if cameras is None else camera_array(cameras)
        self._order_after_producer(colour, stream)
        if plane is not None:
            self._order_after_producer(plane, stream)
        step = _lib.MAX_FOLD_TRAP_BATCH
        base, frame_bytes = _device_pointer(colour), rows * w * 4  # (a plane of one f32 per pixel is as many bytes)
        planes = None if plane is None else _device_pointer(plane)
        for first in range(0, n, step):
            m = min(step, n - first)
            ptrs = (C.c_void_p * m)(*[base + (first + i) * frame_bytes for i in range(m)])
            part = None if cams is None else C.cast(C.byref(cams, first * C.sizeof(CameraUniform)), C.POINTER(CameraUniform))
            check(lib.kifs_render_folded_trapped_async(self._ctx, stream, m, part, ptrs, w * 4, C.byref(system), C.byref(record),
                                                       None if lit is None else C.byref(lit),
                                                       None if term is None else C.byref(term),
                                                       None if planes is None else planes + first * frame_bytes, w * 4,
                                                       frame_bytes, y0, y1, encode), "render_folded_trapped")
        return colour if plane is None else (colour, plane)

    def render_folded_trapped(self, fold: FoldSystem, trap: OrbitTrap, light: Light = None, ao: AmbientOcclusion = None,
                              u_plane=False, y0: int = 0, y1: int = None, encode: int = ENCODE_SRGB, stream=None):
        """The context's frame seen through `fold` and coloured by `trap` (under `light`, with `ao`), synchronously: a
        uint8 rows x W x 4 torch tensor on this context's device, or with `u_plane` the pair (colour, float32 rows x W)."""
        import torch
        r = self.render_folded_trapped_batch(None, fold, trap, light=light, ao=ao, u_plane=u_plane, stream=stream, y0=y0, y1=y1,
                                             encode=encode)
        colour, plane = r if isinstance(r, tuple) else (r, None)
        if stream is None:
            self.synchronize()
        else:
            torch.cuda.synchronize(colour.device)
        return colour[0] if plane is None else (colour[0], plane[0])

    def eval_fold_trap(self, fold: FoldSystem, trap: OrbitTrap, points):
        """u -- the least distance to the trap of the fold's orbit, continued by the base primitive's -- of (n, 3)
        positions with the context's options: (n,) float32.  Of the trap only centre, axes and iterations are read."""
        pts = np.ascontiguousarray(points, dtype=np.float32).reshape(-1, 3)
        n = pts.shape[0]
        u = np.empty(n, dtype=np.float32)
        system = fold.into_buffer_data() if hasattr(fold, "into_buffer_data") else fold
        record = trap.into_buffer_data() if hasattr(trap, "into_buffer_data") else trap
        fp = lambda a: a.ctypes.data_as(C.POINTER(C.c_float))
        check(lib.kifs_eval_fold_trap(self._ctx, C.byref(system), C.byref(record), fp(pts), n, fp(u)), "eval_fold_trap")
        return u

    # ---- ray queries (kifs_trace_rays_async): caller-supplied rays to hit, normal and colour
    def trace_rays(self, rays, colours: bool = True, geometry: bool = True, encode: int = ENCODE_SRGB, stream=None):
        """Trace n rays of the caller's own through the context's scene (options, iteration counts, extensions; the
        screen, the camera and the supersampling factor are not read).  `rays`: an (n, 8) float32 torch tensor on this
        context's device in KifsRay layout -- (origin.xyz, -, direction.xyz, -), the two reserved words are not read -- or
        a pair (origins, directions) of (n, 3) arrays or tensors, which is packed here.  A direction is used as given,
        not normalised: t is in units of its length.  Returns (geometry, rgba): an (n, 4) float32 tensor of texels
        (n.x, n.y, n.z, t), (0, 0, 0, +inf) on a miss, and an (n, 4) uint8 tensor of the pixels the rays would have
        produced in a frame; None for the one not asked for.  Enqueued on `stream` like render_async (the launch is
        ordered after torch's current stream, where the rays were produced); the caller synchronises before reading."""
        import torch
        if not colours and not geometry:
            raise ValueError("trace_rays: colours, geometry or both")
        dev = torch.device("cuda", self.device)
        if isinstance(rays, (tuple, list)):
            if len(rays) != 2:
                raise ValueError("trace_rays: a packed (n, 8) tensor or an (origins, directions) pair")
            o, d = (torch.as_tensor(np.asarray(v, dtype=np.float32) if not torch.is_tensor(v) else v).to(dev, torch.float32)
                    for v in rays)
            if o.dim() != 2 or o.shape[1] != 3 or tuple(d.shape) != tuple(o.shape):
                raise ValueError("trace_rays: origins and directions are both (n, 3)")
            packed = torch.zeros((o.shape[0], 8), dtype=torch.float32, device=dev)
            packed[:, 0:3] = o
            packed[:, 4:7] = d
            rays = packed
        if (not getattr(rays, "is_cuda", False) or rays.device != dev or rays.dtype != torch.float32 or rays.dim() != 2
                or rays.shape[1] != 8 or not rays.is_contiguous()):
            raise ValueError(f"trace_rays: rays is a contiguous (n, 8) float32 tensor on {dev}")
        n = int(rays.shape[0])
        if n > _lib.MAX_RAYS:
            raise ValueError(f"trace_rays: at most {_lib.MAX_RAYS} rays per call")
        geom = torch.empty((n, 4), dtype=torch.float32, device=dev) if geometry else None
        rgba = torch.empty((n, 4), dtype=torch.uint8, device=dev) if colours else None
        if n == 0:
            return geom, rgba
        stream = self._stream_handle(stream, "trace_rays")
        self._order_after_producer(rays, stream)
        check(lib.kifs_trace_rays_async(self._ctx, stream, _device_pointer(rays), n,
                                        _device_pointer(geom) if geometry else None,
                                        _device_pointer(rgba) if colours else None, encode), "trace_rays")
        return geom, rgba

    # ---- adaptive anti-aliasing (kifs_render_adaptive_async): the k x k resolve for the edge pixels only
    def render_adaptive_batch(self, cameras=None, k: int = 2, normal_cos: float = 0.9, depth_rel: float = 0.05, stream=None,
                              encode: int = ENCODE_SRGB, colour=None, edge_counts=None):
        """len(cameras) <= MAX_BATCH whole frames (cameras None: one frame with the context's camera), each rendered
        once with its geometry; the pixels whose hit / miss, normal (dot product below `normal_cos`) or depth (relative
        difference above `depth_rel`) differs from a 4-neighbour's get the k x k supersampled resolve, every other pixel
        stays the plain frame's.  Returns (colour, edge_counts): a uint8 (count, H, W, 4) and an int32
        (count,) torch tensor on this context's device -- the number of pixels supersampled per frame.  `colour`, `edge_counts`:
        contiguous destination tensors of those shapes to reuse.  Enqueued on `stream` like render_async; the caller
        synchronises before reading.  A tensor this method allocates is written on the launch stream, which torch's
        allocator does not know of: keep the returned tensors alive until the launch has run (or pass your own), as with
        render_geometry_batch's planes."""
        import torch
        w, h = self.screen_data.width, self.screen_data.height
        n = 1 if cameras is None else len(cameras)
        if not 1 <= n <= MAX_BATCH:
            raise ValueError(f"render_adaptive_batch: 1..{MAX_BATCH} frames")
        dev = torch.device("cuda", self.device)
        if colour is None:
            colour = torch.empty((n, h, w, 4), dtype=torch.uint8, device=dev)
        if tuple(colour.shape) != (n, h, w, 4) or colour.dtype != torch.uint8 or not colour.is_contiguous():
            raise ValueError(f"render_adaptive_batch: colour uint8 ({n}, {h}, {w}, 4), contiguous")
        counts = torch.empty((n,), dtype=torch.int32, device=dev) if edge_counts is None else edge_counts
        if tuple(counts.shape) != (n,) or counts.dtype != torch.int32 or not counts.is_contiguous():
            raise ValueError(f"render_adaptive_batch: edge_counts int32 ({n},), contiguous")
        stream = self._stream_handle(stream, "render_adaptive_batch")
        cams = None if cameras is None else camera_array(cameras)
        base, frame_bytes = _device_pointer(colour), h * w * 4
        ptrs = (C.c_void_p * n)(*[base + i * frame_bytes for i in range(n)])
        aa = AdaptiveAAC(int(k), float(normal_cos), float(depth_rel))
        self._order_after_producer(colour, stream)
        check(lib.kifs_render_adaptive_async(self._ctx, stream, n, cams, ptrs, w * 4, C.byref(aa), _device_pointer(counts),
                                             encode), "render_adaptive")
        return colour, counts

    def render_adaptive(self, k: int = 2, normal_cos: float = 0.9, depth_rel: float = 0.05, encode: int = ENCODE_SRGB,
                        stream=None):
        """The context's frame with adaptive anti-aliasing, synchronously: (colour uint8 H x W x 4 torch tensor on this
        context's device, number of pixels supersampled)."""
        import torch
        colour, counts = self.render_adaptive_batch(None, k=k, normal_cos=normal_cos, depth_rel=depth_rel, stream=stream,
                                                    encode=encode)
        if stream is None:
            self.synchronize()
        else:
            torch.cuda.synchronize(colour.device)
        return colour[0], int(counts[0].item())

    # ---- animated batches (kifs_render_animation_async): per-frame constant, power and colours in one launch
    def render_animation(self, options, cameras=None, outs=None, y0: int = 0, y1: int = None, encode: int = ENCODE_SRGB,
                         stream=None):
        """One launch for len(options) <= MAX_BATCH frames of a morph: frame i is rendered with options[i] (GuiData or
        an OptionsUniform image; an options_array is taken as it is) and cameras[i] (cameras None: the context's camera
        for every frame).  constant, power, fractal_color and background_color may differ between the frames;
        everything else of the options must be frame 0's (KifsError BAD_ARG otherwise).  The context's own options are
        neither used nor changed.  Returns the frames as one uint8 (count, rows, W, 4) torch tensor on this context's
        device; `outs`: a contiguous destination tensor of that shape to reuse.  Enqueued on `stream` like render_async
        and ordered after torch's current stream; the caller synchronises before reading, and keeps a tensor this
        method allocated alive until the launch has run (as with render_geometry_batch's planes)."""
        w, h = self.screen_data.width, self.screen_data.height
        y1 = h if y1 is None else y1
        rows = max(y1 - y0, 0)
        opts = options_array(options)
        n = len(opts)
        if not 1 <= n <= MAX_BATCH:
            raise ValueError(f"render_animation: 1..{MAX_BATCH} frames")
        if cameras is not None:
            _one_per_view("render_animation", "option images", opts, len(cameras))
        outs, ptrs = _frame_outs("render_animation", outs, n, rows, w, self.device)
        stream = self._stream_handle(stream, "render_animation")
        cams = None if cameras is None else camera_array(cameras)
        self._order_after_producer(outs, stream)
        check(lib.kifs_render_animation_async(self._ctx, stream, n, cams, opts, ptrs, w * 4, y0, y1, encode),
              "render_animation")
        return outs

    # ---- accumulated frames (kifs_render_accumulate_async): every frame the linear-colour mean of its sub-frames
    def render_accumulate(self, cameras, samples, options=None, outs=None, y0: int = 0, y1: int = None,
                          encode: int = ENCODE_SRGB, stream=None, jitter=None):
        """One launch for len(cameras) / samples output frames, each the mean of `samples` sub-frames taken in linear
        colour before the encode: motion blur (configs.shutter_cameras), depth of field (configs.lens_cameras), a morph
        without temporal aliasing (per-sub-frame options).  Sub-frame s of frame i is cameras[i * samples + s] (CameraData
        or CameraUniform images; a camera_array is taken as it is) with options[i * samples + s] (GuiData or
        OptionsUniform images, as render_animation takes them; None: the context's options for all of them).
        1 <= samples <= MAX_ACCUMULATE and len(cameras) <= MAX_BATCH.  Returns the frames as one uint8
        (count, rows, W, 4) torch tensor on this context's device; `outs`: a contiguous destination tensor of that shape
        to reuse.  Enqueued on `stream` like render_async and ordered after torch's current stream; the caller
        synchronises before reading, and keeps a tensor this method allocated alive until the launch has run.
        `jitter` = (grid, cells) sends sub-frame v through cell cells[v] = (i, j) of the grid x grid cells of its pixel
        instead of the centre (kifs_render_accumulate_jittered_async: the blur's rays anti-alias too); cells: a sequence
        of len(cameras) pairs (configs.jitter_cells), a ready KifsSubpixel array, or None with samples == grid * grid for
        the supersampling order (configs.grid_cells).  None: today's call and bytes."""
        w, h = self.screen_data.width, self.screen_data.height
        y1 = h if y1 is None else y1
        rows = max(y1 - y0, 0)
        samples = int(samples)
        cams, views, n = _accumulated_views("render_accumulate", cameras, samples)
        opts = _one_per_view("render_accumulate", "option images", None if options is None else options_array(options), views)
        outs, ptrs = _frame_outs("render_accumulate", outs, n, rows, w, self.device)
        stream = self._stream_handle(stream, "render_accumulate")
        self._order_after_producer(outs, stream)
        if jitter is None:
            check(lib.kifs_render_accumulate_async(self._ctx, stream, n, samples, cams, opts, ptrs, w * 4, y0, y1, encode),
                  "render_accumulate")
            return outs
        grid, cells = _jitter_cells("render_accumulate", jitter, views, samples, centre=False)
        check(lib.kifs_render_accumulate_jittered_async(self._ctx, stream, n, samples, cams, opts, grid, cells, ptrs, w * 4,
                                                        y0, y1, encode), "render_accumulate")
        return outs

    # ---- progressive accumulation (kifs_render_accumulate_resume_async): a frame's linear sums carried across launches
    def render_accumulate_resume(self, sums, prior, cameras, samples, options=None, outs=None, picture: bool = True,
                                 y0: int = 0, y1: int = None, encode: int = ENCODE_SRGB, stream=None, jitter=None):
        """One PASS of a progressive frame: render_accumulate's launch for these cameras, options and jitter, whose
        resolve starts from `sums` -- a contiguous float32 (count, rows, W, 4) tensor on this context's device holding
        (sum.r, sum.g, sum.b, float(total)) per pixel after `prior` sub-frames; prior == 0: not read, whatever it holds --
        adds the pass's sub-frames in the contract's order and writes the sums back with total = prior + samples.  With
        `picture` the frames encode(sum / total) are returned as render_accumulate returns them (`outs` to reuse); without,
        the pass only advances the plane and returns None.  Passes whose views concatenate to one render_accumulate
        call's give that call's bytes, for any split; the library keeps no state, `sums` and `prior` are all of it
        (Accumulator below keeps them together).  jitter None: the pixel centre.  Ordered after the producers of both
        `sums` and `outs` -- torch's current stream -- and after nothing else: two passes of one plane on different
        streams are the caller's to order (contract (c) of the header); Accumulator.add does it."""
        import torch
        w, h = self.screen_data.width, self.screen_data.height
        y1 = h if y1 is None else y1
        rows = max(y1 - y0, 0)
        samples, prior = int(samples), int(prior)
        cams, views, n = _accumulated_views("render_accumulate_resume", cameras, samples, "per frame and pass")
        if not 0 <= prior <= _lib.MAX_PROGRESSIVE_SAMPLES - samples:
            raise ValueError(f"render_accumulate_resume: prior + samples within 0..{_lib.MAX_PROGRESSIVE_SAMPLES}")
        opts = _one_per_view("render_accumulate_resume", "option images", None if options is None else options_array(options), views)
        if (not isinstance(sums, torch.Tensor) or tuple(sums.shape) != (n, rows, w, 4) or sums.dtype != torch.float32
                or not sums.is_contiguous() or not sums.is_cuda):
            raise ValueError(f"render_accumulate_resume: sums float32 ({n}, {rows}, {w}, 4), contiguous, on the device")
        ptrs = None
        if picture:
            outs, ptrs = _frame_outs("render_accumulate_resume", outs, n, rows, w, self.device)
        grid, cells = _jitter_cells("render_accumulate_resume", jitter, views, samples)
        stream = self._stream_handle(stream, "render_accumulate_resume")
        self._order_after_producer(sums, stream)
        if picture:
            self._order_after_producer(outs, stream)
        check(lib.kifs_render_accumulate_resume_async(self._ctx, stream, n, samples, cams, opts, grid, cells,
                                                      _device_pointer(sums), w * 16, rows * w * 16, prior, ptrs, w * 4, y0, y1,
                                                      encode), "render_accumulate_resume")
        return outs if picture else None

    def render_accumulate_converge(self, sums, moments, cameras, samples, rule, restart: bool = False, counts=None,
                                   options=None, outs=None, picture: bool = True, y0: int = 0, y1: int = None,
                                   encode: int = ENCODE_SRGB, stream=None, jitter=None):
        """One CONVERGING pass of a progressive frame (kifs_render_accumulate_converge_async): render_accumulate_resume's
        pass for the pixels whose mean has not settled under rule = (tolerance, min_samples).  `sums` is that call's plane
        with w the PIXEL'S OWN count; `moments` a contiguous float32 (count, rows, W) tensor, the sum of the squared
        luminances of every pixel's sub-frames; restart=True reads neither (the first pass).  A settled pixel is neither
        marched nor written; with `picture` every pixel is encoded from its state after the pass.  `counts`, an int32 or
        uint32 (count,) tensor on the device, receives per frame the pixels still active after the pass (0: done).  The
        library keeps no state.  Ordered after the producers of all four tensors -- torch's current stream -- and after
        nothing else, as render_accumulate_resume."""
        import torch
        w, h = self.screen_data.width, self.screen_data.height
        y1 = h if y1 is None else y1
        rows = max(y1 - y0, 0)
        samples = int(samples)
        cams, views, n = _accumulated_views("render_accumulate_converge", cameras, samples, "per frame and pass")
        tolerance, min_samples = float(rule[0]), int(rule[1])
        if not tolerance >= 0.0 or not 2 <= min_samples <= _lib.MAX_PROGRESSIVE_SAMPLES:
            raise ValueError(f"render_accumulate_converge: tolerance >= 0, min_samples within 2..{_lib.MAX_PROGRESSIVE_SAMPLES}")
        opts = _one_per_view("render_accumulate_converge", "option images", None if options is None else options_array(options), views)
        for name, plane, shape in (("sums", sums, (n, rows, w, 4)), ("moments", moments, (n, rows, w))):
            if (not isinstance(plane, torch.Tensor) or tuple(plane.shape) != shape or plane.dtype != torch.float32
                    or not plane.is_contiguous() or not plane.is_cuda):
                raise ValueError(f"render_accumulate_converge: {name} float32 {shape}, contiguous, on the device")
        if counts is not None and (not isinstance(counts, torch.Tensor) or tuple(counts.shape) != (n,) or not counts.is_cuda
                                   or counts.dtype not in (torch.int32, torch.uint32) or not counts.is_contiguous()):
            raise ValueError(f"render_accumulate_converge: counts int32 ({n},), contiguous, on the device")
        ptrs = None
        if picture:
            outs, ptrs = _frame_outs("render_accumulate_converge", outs, n, rows, w, self.device)
        grid, cells = _jitter_cells("render_accumulate_converge", jitter, views, samples)
        stream = self._stream_handle(stream, "render_accumulate_converge")
        for tensor in (sums, moments, counts, outs if picture else None):
            if tensor is not None:
                self._order_after_producer(tensor, stream)
        c_rule = _lib.KifsConvergence(tolerance, min_samples)
        check(lib.kifs_render_accumulate_converge_async(
            self._ctx, stream, n, samples, cams, opts, grid, cells, _device_pointer(sums), w * 16, rows * w * 16,
            _device_pointer(moments), w * 4, rows * w * 4, int(bool(restart)), C.byref(c_rule),
            None if counts is None else _device_pointer(counts), ptrs, w * 4, y0, y1, encode), "render_accumulate_converge")
        return outs if picture else None

    def render_shard_async(self, outs, cameras, stripes, in_place: bool = False, stream=None,
                           encode: int = ENCODE_SRGB, pitch_bytes: int = None):
        """render_batch_async for a row shard (kifs_render_shard_async): `stripes` is the list of
        8-row stripe indices (shard_stripes); outs[i] is a packed (rows, W, 4) device tensor, or
        with in_place a whole (H, W, 4) frame whose shard rows are written where they belong."""
        if len(outs) != len(cameras) or not (1 <= len(outs) <= MAX_BATCH):
            raise ValueError(f"render_shard_async: 1..{MAX_BATCH} frames, one camera each")
        w = self.screen_data.width
        pitch = pitch_bytes if pitch_bytes is not None else w * 4
        if stream is not None and hasattr(stream, "cuda_stream"):
            stream = stream.cuda_stream
            if not stream:
                raise ValueError("render_shard_async: pass a non-default torch.cuda.Stream")
        n = len(outs)
        cams = camera_array(cameras)
        # The library knows nothing about the size of the destinations: a packed shard needs rows * pitch bytes, a
        # shard rendered in place a whole frame.  (A DevicePointers remembers what it has been checked against: a
        # step of a few hundred views must not pay for the check every time.)
        h = self.screen_data.height
        if any(s < 0 or s * STRIPE_ROWS >= h for s in stripes):
            raise ValueError("render_shard_async: stripe outside the frame")
        need_rows = h if in_place else sum(min(STRIPE_ROWS, h - s * STRIPE_ROWS) for s in stripes)
        need = ((need_rows - 1) * pitch + w * 4) if need_rows else 0
        checked = getattr(outs, "checked_bytes", None)
        if checked is None or checked < need:
            for o in (outs.tensors if isinstance(outs, DevicePointers) else outs):
                if hasattr(o, "element_size"):
                    if not o.is_contiguous() or o.element_size() != 1 or o.numel() < need:
                        raise ValueError(f"render_shard_async: every destination must be a contiguous uint8 tensor of at "
                                         f"least {need} bytes ({need_rows} rows of pitch {pitch}"
                                         f"{', a whole frame: in_place' if in_place else ''}); got {tuple(o.shape)}")
            if isinstance(outs, DevicePointers):
                outs.checked_bytes = need
        ptrs = outs.array if isinstance(outs, DevicePointers) else (C.c_void_p * n)(*[_device_pointer(o) for o in outs])
        st = _stripe_array(stripes)
        self._order_after_producer(outs[0], stream)
        check(lib.kifs_render_shard_async(self._ctx, stream, n, cams, ptrs, pitch, st, len(st),
                                          1 if in_place else 0, encode), "render_shard_async")

    def unpack_shard_async(self, frames, shards, stripes, stream=None):
        """Root side of the gather (kifs_unpack_shard_async): `shards` (count, rows, W, 4) packed,
        `frames` (count, H, W, 4); stripe k of every shard goes to frame rows 8 * stripes[k]...
        Both are contiguous device tensors."""
        w, h = self.screen_data.width, self.screen_data.height
        if frames.dim() != 4 or shards.dim() != 4 or not (frames.is_contiguous() and shards.is_contiguous()):
            raise ValueError("unpack_shard_async: frames (count, H, W, 4) and shards (count, rows, W, 4), contiguous")
        count = int(frames.shape[0])
        rows = int(shards.shape[1])
        want_rows = sum(min(STRIPE_ROWS, h - s * STRIPE_ROWS) for s in stripes)
        if (tuple(frames.shape[1:]) != (h, w, 4) or tuple(shards.shape) != (count, rows, w, 4) or rows != want_rows
                or frames.element_size() != 1 or shards.element_size() != 1):
            raise ValueError(f"unpack_shard_async: shapes {tuple(frames.shape)} / {tuple(shards.shape)} do not match "
                             f"{count} frames of {h}x{w} and a shard of {want_rows} rows")
        if stream is not None and hasattr(stream, "cuda_stream"):
            stream = stream.cuda_stream
            if not stream:
                raise ValueError("unpack_shard_async: pass a non-default torch.cuda.Stream")
        st = _stripe_array(stripes)
        self._order_after_producer(frames, stream)
        check(lib.kifs_unpack_shard_async(self._ctx, stream, count, _device_pointer(frames), w * 4, h * w * 4,
                                          _device_pointer(shards), w * 4, rows * w * 4, st, len(st)),
              "unpack_shard_async")

    # ---- sparse shards (kifs_pack_sparse_async / kifs_unpack_sparse_async / kifs_fill_shard_async)
    def _stream_handle(self, stream, what):
        if stream is not None and hasattr(stream, "cuda_stream"):
            stream = stream.cuda_stream
            if not stream:
                raise ValueError(f"{what}: pass a non-default torch.cuda.Stream")
        return stream

    def sparse_capacity(self, count: int, stripes) -> int:
        """Records a payload must have room for: every tile of `count` shards of these stripes."""
        return count * len(stripes) * ((self.screen_data.width + 31) // 32)

    def pack_sparse_async(self, shards, stripes, records, n_records, host_n_records=None, stream=None,
                          encode: int = ENCODE_SRGB):
        """Peer side: `shards` (count, rows, W, 4) packed -> `records` (capacity, 1040) uint8 device tensor,
        their number in `n_records` (int32 device tensor of one element) and, asynchronously, in the pinned
        host tensor `host_n_records` (valid once the stream has passed this point)."""
        w, h = self.screen_data.width, self.screen_data.height
        if shards.dim() != 4 or not shards.is_contiguous() or shards.element_size() != 1:
            raise ValueError("pack_sparse_async: shards (count, rows, W, 4) uint8, contiguous")
        count, rows = int(shards.shape[0]), int(shards.shape[1])
        want_rows = sum(min(STRIPE_ROWS, h - s * STRIPE_ROWS) for s in stripes)
        if tuple(shards.shape) != (count, rows, w, 4) or rows != want_rows:
            raise ValueError(f"pack_sparse_async: shape {tuple(shards.shape)} is not {count} shards of {want_rows} x {w}")
        if (records.dim() != 2 or int(records.shape[1]) != SPARSE_RECORD_BYTES or records.element_size() != 1
                or not records.is_contiguous() or int(records.shape[0]) < self.sparse_capacity(count, stripes)):
            raise ValueError(f"pack_sparse_async: records must be (>= {self.sparse_capacity(count, stripes)}, "
                             f"{SPARSE_RECORD_BYTES}) uint8, contiguous")
        if n_records.numel() != 1 or n_records.element_size() != 4:
            raise ValueError("pack_sparse_async: n_records is one 32-bit integer on the device")
        if host_n_records is not None and (host_n_records.numel() != 1 or host_n_records.element_size() != 4
                                           or not host_n_records.is_pinned()):
            raise ValueError("pack_sparse_async: host_n_records is one 32-bit integer in pinned host memory")
        st = _stripe_array(stripes)
        stream = self._stream_handle(stream, "pack_sparse_async")
        self._order_after_producer(records, stream)
        check(lib.kifs_pack_sparse_async(self._ctx, stream, count,
                                         _device_pointer(shards), w * 4, rows * w * 4, st, len(st), encode,
                                         _device_pointer(records), int(records.shape[0]), _device_pointer(n_records),
                                         _device_pointer(host_n_records) if host_n_records is not None else None),
              "pack_sparse_async")

    def erase_sparse_async(self, frames, records, n_records: int, stripes, stream=None, encode: int = ENCODE_SRGB):
        """The background over the tiles of the first `n_records` records (kifs_erase_sparse_async)."""
        self.unpack_sparse_async(frames, records, n_records, stripes, stream=stream, _erase_encode=encode)

    def unpack_sparse_async(self, frames, records, n_records: int, stripes, stream=None, _erase_encode=None):
        """Root side: the first `n_records` records of `records` -> their rows of `frames` (count, H, W, 4)."""
        w, h = self.screen_data.width, self.screen_data.height
        if frames.dim() != 4 or tuple(frames.shape[1:]) != (h, w, 4) or not frames.is_contiguous() or frames.element_size() != 1:
            raise ValueError(f"unpack_sparse_async: frames (count, {h}, {w}, 4) uint8, contiguous")
        count = int(frames.shape[0])
        if n_records < 0 or n_records > self.sparse_capacity(count, stripes) or (n_records and (
                records.dim() != 2 or int(records.shape[1]) != SPARSE_RECORD_BYTES or int(records.shape[0]) < n_records
                or not records.is_contiguous() or records.element_size() != 1)):
            raise ValueError("unpack_sparse_async: n_records records of 1040 bytes, at most one per tile of the shards")
        st = _stripe_array(stripes)
        stream = self._stream_handle(stream, "erase_sparse_async" if _erase_encode is not None else "unpack_sparse_async")
        self._order_after_producer(frames, stream)
        if _erase_encode is not None:
            check(lib.kifs_erase_sparse_async(self._ctx, stream, count,
                                              _device_pointer(frames), w * 4, h * w * 4,
                                              _device_pointer(records) if n_records else None, n_records, st, len(st),
                                              _erase_encode), "erase_sparse_async")
            return
        check(lib.kifs_unpack_sparse_async(self._ctx, stream, count,
                                           _device_pointer(frames), w * 4, h * w * 4,
                                           _device_pointer(records) if n_records else None, n_records, st, len(st)),
              "unpack_sparse_async")

    def fill_shard_async(self, frames, stripes, stream=None, encode: int = ENCODE_SRGB):
        """The background over the rows of `stripes` of `frames` (count, H, W, 4)."""
        w, h = self.screen_data.width, self.screen_data.height
        if frames.dim() != 4 or tuple(frames.shape[1:]) != (h, w, 4) or not frames.is_contiguous() or frames.element_size() != 1:
            raise ValueError(f"fill_shard_async: frames (count, {h}, {w}, 4) uint8, contiguous")
        st = _stripe_array(stripes)
        stream = self._stream_handle(stream, "fill_shard_async")
        self._order_after_producer(frames, stream)
        check(lib.kifs_fill_shard_async(self._ctx, stream, int(frames.shape[0]),
                                        _device_pointer(frames), w * 4, h * w * 4, st, len(st), encode),
              "fill_shard_async")

    def debug_last_round_steps(self) -> int:
        """Round length of the ray re-queuing in the latest launch (0: one wave per block)."""
        return int(lib.kifs_debug_last_round_steps(self._ctx))

    def debug_last_group_tiles(self) -> int:
        """Latest launch: 0 = one wave per tile (render_wave_kernel), 1 / 2 = tiles per 256-thread
        workgroup (render_group_kernel), -1 = no ray re-queuing."""
        return int(lib.kifs_debug_last_group_tiles(self._ctx))

    KERNEL_NAMES = ("render_kernel", "render_group_kernel", "render_wave_kernel", "render_bunny_quad_kernel",
                    "render_bunny_coop_kernel", "render_ssaa_kernel", "render_geometry_kernel", "render_adaptive_kernel",
                    "render_animation_kernel", "render_accumulate_kernel")

    def debug_last_kernel(self) -> str:
        """Name of the render kernel the latest launch used ("" before the first)."""
        k = int(lib.kifs_debug_last_kernel(self._ctx))
        return self.KERNEL_NAMES[k] if 0 <= k < len(self.KERNEL_NAMES) else ""

    def debug_last_bunny_form(self) -> int:
        """The bunny's throughput form in the latest launch: 0 four lanes per ray (weights in VGPRs), 1 four waves per
        64 rays, 2 four lanes per ray with layer 2 in LDS; -1 = not a re-queued bunny launch."""
        return int(lib.kifs_debug_last_bunny_form(self._ctx))

    def set_frames_in_flight(self, n: int):
        """Scheduling hint: the caller keeps n frames in flight on this device (one context and
        stream each).  n > 1 trades the lone-frame residency cap for throughput."""
        check(lib.kifs_set_frames_in_flight(self._ctx, int(n)), "set_frames_in_flight")

    def set_profiling(self, every: int = 1):
        """every = 0: off; 1: time every launch; n: every n-th launch."""
        check(lib.kifs_set_profiling(self._ctx, int(every)), "set_profiling")

    def profile_read(self):
        """(launches, mean_ms, min_ms, max_ms) of the render kernel since the last read."""
        n, mean, lo, hi = C.c_int(), C.c_double(), C.c_double(), C.c_double()
        check(lib.kifs_profile_read(self._ctx, C.byref(n), C.byref(mean), C.byref(lo), C.byref(hi)),
              "profile_read")
        return n.value, mean.value, lo.value, hi.value

    def last_kernel_ms(self) -> float:
        return float(lib.kifs_last_kernel_ms(self._ctx))

    def synchronize(self):
        check(lib.kifs_synchronize(self._ctx), "synchronize")

    # -- point evaluation (parity tooling) -------------------------------------------------
    def eval_points(self, points, want_normals=True):
        pts = np.ascontiguousarray(points, dtype=np.float32).reshape(-1, 3)
        n = pts.shape[0]
        sdf = np.empty(n, dtype=np.float32)
        nrm = np.empty((n, 3), dtype=np.float32) if want_normals else None
        fp = lambda a: a.ctypes.data_as(C.POINTER(C.c_float)) if a is not None else None
        check(lib.kifs_eval_points(self._ctx, fp(pts), n, fp(sdf), fp(nrm)), "eval_points")
        return sdf, nrm

    def debug_counters(self, enable: bool = True):
        """Switch per-wave diagnostics on/off (and reset them); returns the sums of the records
        written since the last call (see kifs_debug_wave_records)."""
        try:
            rec = self.debug_wave_records()
        except KifsError:
            rec = np.zeros((0, 4), dtype=np.uint64)
        out = (C.c_uint64 * 8)()
        check(lib.kifs_debug_counters(self._ctx, 1 if enable else 0, out), "debug_counters")
        rec = rec[rec[:, 0] > 0]
        return dict(fast_steps=int((rec[:, 2] & np.uint64(0xffffffff)).sum()),
                    fast_entries=int((rec[:, 2] >> np.uint64(32)).sum()),
                    general_steps=int(rec[:, 3].sum()), waves=len(rec),
                    fast_ticks=int(rec[:, 1].sum()), wave_ticks=int(rec[:, 0].sum()))

    def debug_get_tile_order(self):
        buf = np.zeros(1 << 22, dtype=np.uint32)
        n = C.c_size_t(0)
        check(lib.kifs_debug_get_tile_order(self._ctx, buf.ctypes.data_as(C.POINTER(C.c_uint32)),
                                            buf.size, C.byref(n)), "get_tile_order")
        return buf[:n.value].copy()

    def debug_get_tile_costs(self):
        """(cost, seen, shift) of the full frame's tile table (kifs_debug_get_tile_costs): what the latest recording launch
        wrote, the memory of a batch's sorts (cost << 8 | age) and the sort's shift for the costs."""
        tiles = ((self.screen_data.width + 31) // 32) * ((self.screen_data.height + 7) // 8)
        cost, seen = np.zeros(tiles, dtype=np.uint32), np.zeros(tiles, dtype=np.uint32)
        n, shift = C.c_size_t(0), C.c_uint32(0)
        up = lambda a: a.ctypes.data_as(C.POINTER(C.c_uint32))
        check(lib.kifs_debug_get_tile_costs(self._ctx, up(cost), up(seen), cost.size, C.byref(n), C.byref(shift)), "get_tile_costs")
        return cost[:n.value].copy(), seen[:n.value].copy(), int(shift.value)

    def debug_set_tile_order(self, order):
        o = np.ascontiguousarray(order, dtype=np.uint32)
        check(lib.kifs_debug_set_tile_order(self._ctx, o.ctypes.data_as(C.POINTER(C.c_uint32)),
                                            o.size), "set_tile_order")

    def debug_sort_tiles(self, cost, tiles_x: int, shift: int = 0):
        """The tile-order sort on chosen costs (kifs_debug_sort_tiles): (order, cost table afterwards), both uint32
        arrays of cost.size words.  The context's own tile tables are not touched."""
        cs = np.ascontiguousarray(cost, dtype=np.uint32).ravel()
        order, after = np.empty_like(cs), np.empty_like(cs)
        up = lambda a: a.ctypes.data_as(C.POINTER(C.c_uint32))
        check(lib.kifs_debug_sort_tiles(self._ctx, up(cs), cs.size, tiles_x, shift, up(order), up(after)), "debug_sort_tiles")
        return order, after

    def debug_wave_records(self, max_waves: int = 1 << 20):
        """(n_waves, 4) uint64: total ticks, long-ray-loop ticks, long-ray steps, general steps."""
        buf = np.zeros((max_waves, 4), dtype=np.uint64)
        n = C.c_size_t(0)
        check(lib.kifs_debug_wave_records(self._ctx, buf.ctypes.data_as(C.POINTER(C.c_uint64)),
                                          max_waves, C.byref(n)), "debug_wave_records")
        return buf[:n.value]

    def eval_math(self, fn: int, x, param: float = 0.0):
        xs = np.ascontiguousarray(x, dtype=np.float32).ravel()
        out = np.empty_like(xs)
        fp = lambda a: a.ctypes.data_as(C.POINTER(C.c_float))
        check(lib.kifs_eval_math(self._ctx, fn, fp(xs), param, fp(out), xs.size), "eval_math")
        return out


_NO_PASS = object()  # Accumulator._last_stream before the first pass (None is the context's own stream)


class Accumulator:
    """The state of a progressive frame (GraphicState.render_accumulate_resume): the plane of linear sums and the number
    of sub-frames in it, for `count` frames of rows [y0, y1) of `state`'s screen.  add() is one pass; passes of any sizes
    give the bytes of one render_accumulate call over all their views.  Passes may run on different streams: add() orders
    a pass after the previous one when its stream differs (render_accumulate_resume leaves that to its caller) -- with
    kifs_order_after when the previous pass ran on a caller's stream, and with state.synchronize(), A HOST WAIT, when it
    ran on the context's own stream, for which the header has no handle to name as a producer."""

    def __init__(self, state, count: int = 1, y0: int = 0, y1: int = None):
        import torch
        self.state, self.count, self.y0 = state, int(count), int(y0)
        self.y1 = state.screen_data.height if y1 is None else int(y1)
        rows = max(self.y1 - self.y0, 0)
        self.sums = torch.zeros((self.count, rows, state.screen_data.width, 4), dtype=torch.float32,
                                device=torch.device("cuda", state.device))
        self.reset()

    def add(self, cameras, samples, options=None, outs=None, picture: bool = True, encode: int = ENCODE_SRGB, stream=None,
            jitter=None):
        """One pass of `samples` sub-frames per frame (len(cameras) == count * samples): the frames after it, or None
        with picture=False.  `stream` as render_async takes it; a pass on another stream than the previous pass's is
        ordered after that pass first -- without blocking the host when it ran on a caller's stream, and by waiting on
        the host for the context's own stream (state.synchronize()) when it ran there."""
        if len(camera_array(cameras)) != self.count * int(samples):
            raise ValueError(f"Accumulator.add: {self.count} x {samples} cameras")
        handle = getattr(stream, "cuda_stream", stream) or None  # None: the context's own stream
        if self._last_stream is not _NO_PASS and handle != self._last_stream:
            if self._last_stream is None:
                self.state.synchronize()
            else:
                self.state.order_after(handle, self._last_stream)
        frames = self.state.render_accumulate_resume(self.sums, self.total, cameras, samples, options=options, outs=outs,
                                                     picture=picture, y0=self.y0, y1=self.y1, encode=encode, stream=stream,
                                                     jitter=jitter)
        self.total += int(samples)
        self._last_stream = handle
        return frames

    def reset(self):
        """Start over: the next pass does not read the plane, and is ordered after no earlier pass."""
        self.total = 0
        self._last_stream = _NO_PASS

    def linear_mean(self):
        """The linear HDR mean of every pixel, float32 (count, rows, W, 3): sums / total, as the plane describes itself.
        The caller synchronises first."""
        return self.sums[..., :3] / self.sums[..., 3:]


class ConvergingAccumulator(Accumulator):
    """An Accumulator with a stopping rule (GraphicState.render_accumulate_converge): beside the plane of sums it owns a
    plane of second moments and a tensor of counts, add() marches only the pixels whose mean luminance has not settled to
    a standard error of `tolerance` (never before `min_samples` sub-frames), and active() tells how many are left.  The
    first pass after reset() restarts the planes.  `total` stays the number of sub-frames OFFERED to every pixel; what a
    pixel took is samples_per_pixel().  (A class of its own: Accumulator's constructor and passes stay as they are.)"""

    def __init__(self, state, count: int = 1, y0: int = 0, y1: int = None, tolerance: float = 1.0 / 256.0, min_samples: int = 16):
        import torch
        super().__init__(state, count, y0, y1)
        self.tolerance, self.min_samples = float(tolerance), int(min_samples)
        self.moments = torch.zeros(tuple(self.sums.shape[:3]), dtype=torch.float32, device=self.sums.device)
        self.counts = torch.zeros((self.count,), dtype=torch.int32, device=self.sums.device)

    def add(self, cameras, samples, options=None, outs=None, picture: bool = True, encode: int = ENCODE_SRGB, stream=None,
            jitter=None):
        """Accumulator.add with the rule: one converging pass, ordered after the previous one as there."""
        if len(camera_array(cameras)) != self.count * int(samples):
            raise ValueError(f"ConvergingAccumulator.add: {self.count} x {samples} cameras")
        handle = getattr(stream, "cuda_stream", stream) or None  # None: the context's own stream
        if self._last_stream is not _NO_PASS and handle != self._last_stream:
            if self._last_stream is None:
                self.state.synchronize()
            else:
                self.state.order_after(handle, self._last_stream)
        frames = self.state.render_accumulate_converge(self.sums, self.moments, cameras, samples, (self.tolerance, self.min_samples),
                                                       restart=self.total == 0, counts=self.counts, options=options, outs=outs,
                                                       picture=picture, y0=self.y0, y1=self.y1, encode=encode, stream=stream,
                                                       jitter=jitter)
        self.total += int(samples)
        self._last_stream = handle
        return frames

    def active(self):
        """Per frame the pixels still active after the last pass, as a list of ints (0: the frame is done).  Waits for
        the context's launches and the device first."""
        import torch
        self.state.synchronize()
        torch.cuda.synchronize(self.sums.device)
        return [int(v) for v in self.counts.cpu().tolist()]

    def samples_per_pixel(self):
        """float32 (count, rows, W): the sub-frames every pixel holds, the plane's w.  The caller synchronises first."""
        return self.sums[..., 3]


class MultiGraphicState:
    """Single-process multi-GPU renderer over kifs_multi_* -- what the reference's one-process host would hold
    in place of its GraphicState (graphics.rs:25-37) on a node with several GPUs: one context per device, 8-row
    stripes dealt to the devices, shards collected on the first device.  render(): one frame, dense, synchronous.
    render_batch_async() / wait(): steps of up to 512 frames, sparse records over RCCL grouped send/recv inside
    the library, two steps in flight."""

    def __init__(self, devices, screen_data: ScreenData, camera_data: CameraData = None,
                 gui_data: GuiData = None, iters=(100, 10, 10)):
        arr = (C.c_int * len(devices))(*devices)
        st = C.c_int(0)
        self._m = lib.kifs_multi_create(arr, len(devices), C.byref(st))
        if not self._m:
            raise KifsError(st.value, f"kifs_multi_create({list(devices)})")
        self.devices = list(devices)
        self.screen_data = screen_data
        u = screen_data.into_buffer_data()
        check(lib.kifs_multi_set_screen(self._m, C.byref(u)), "multi set_screen")
        self.set_camera(camera_data or CameraData())
        self.update_options(gui_data or GuiData())
        check(lib.kifs_multi_set_iters(self._m, *iters), "multi set_iters")

    def set_camera(self, camera_data: CameraData):
        u = camera_data.into_buffer_data()
        check(lib.kifs_multi_set_camera(self._m, C.byref(u)), "multi set_camera")

    def update_options(self, gui_data: GuiData):
        u = gui_data.into_buffer_data()
        check(lib.kifs_multi_set_options(self._m, C.byref(u)), "multi set_options")

    def render(self, out=None, encode: int = ENCODE_SRGB, pitch_bytes: int = None):
        w, h = self.screen_data.width, self.screen_data.height
        if out is None:
            out = np.empty((h, w, 4), dtype=np.uint8)
        if isinstance(out, np.ndarray):
            _check_host_destination(out, h, w, pitch_bytes or w * 4)
        ptr = out.ctypes.data if isinstance(out, np.ndarray) else _device_pointer(out)
        self._order_after_producer(out)
        check(lib.kifs_multi_render(self._m, ptr, pitch_bytes or w * 4, encode), "multi render")
        return out

    def _order_after_producer(self, dest):
        """GraphicState._order_after_producer for the root device's streams (kifs_multi_order_after): what this object
        enqueues on the root from now on follows torch's current stream there."""
        producer = _producer_stream(dest)
        if producer is not None:
            check(lib.kifs_multi_order_after(self._m, producer or None), "multi order_after")

    # ---- batches of frames, gathered on the first device (kifs_multi_render_batch_async) ----------------
    def set_extensions(self, soft_shadow=False, shadow_steps=0, shadow_k=0.0, shadow_t0=0.0, shadow_max_t=0.0):
        e = ExtensionsC(1 if soft_shadow else 0, int(shadow_steps), float(shadow_k), float(shadow_t0), float(shadow_max_t))
        check(lib.kifs_multi_set_extensions(self._m, C.byref(e)), "multi set_extensions")

    def set_supersampling(self, k: int = 1):
        """GraphicState.set_supersampling on every device: the gathered frames equal one device's."""
        check(lib.kifs_multi_set_supersampling(self._m, int(k)), "multi set_supersampling")

    def set_gather(self, gather: str = "sparse", transport: str = "auto"):
        """gather: 'sparse' (the other devices send only the tiles that hold something) or 'dense';
        transport: 'auto', 'rccl' (grouped ncclSend / ncclRecv inside the library) or 'copy' (peer copies)."""
        g = {"sparse": _lib.GATHER_SPARSE, "dense": _lib.GATHER_DENSE}[gather]
        t = {"auto": _lib.TRANSPORT_AUTO, "rccl": _lib.TRANSPORT_RCCL, "copy": _lib.TRANSPORT_COPY}[transport]
        check(lib.kifs_multi_set_gather(self._m, g, t), f"multi set_gather({gather}, {transport})")

    def _frames_args(self, frames, cameras):
        w, h = self.screen_data.width, self.screen_data.height
        if (frames.dim() != 4 or tuple(frames.shape[1:]) != (h, w, 4) or frames.element_size() != 1
                or not frames.is_contiguous()):
            raise ValueError(f"render_batch: frames (count, {h}, {w}, 4) uint8, contiguous, on the first listed device")
        cams = camera_array(cameras)
        if len(cams) != int(frames.shape[0]) or not 1 <= len(cams) <= MAX_BATCH:
            raise ValueError(f"render_batch: {int(frames.shape[0])} frames for {len(cams)} cameras (1..{MAX_BATCH})")
        if frames.is_cuda and frames.device.index not in (None, self.devices[0]):
            raise ValueError("render_batch: frames must live on the first listed device (the root of the gather)")
        return len(cams), cams, _device_pointer(frames), w * 4, h * w * 4

    def render_batch_async(self, frames, cameras, encode: int = ENCODE_SRGB, untouched: bool = False) -> int:
        """Submits one step: frames[i] (a (count, H, W, 4) uint8 tensor on the first listed device) <- cameras[i].
        Returns the step number for wait() / stream_wait().  untouched=True: `frames` is the buffer passed two
        steps ago and nothing else wrote to it since (KIFS_MULTI_FRAMES_UNTOUCHED)."""
        n, cams, ptr, pitch, stride = self._frames_args(frames, cameras)
        self._order_after_producer(frames)
        step = C.c_uint64(0)
        check(lib.kifs_multi_render_batch_async(self._m, n, cams, ptr, pitch, stride, encode,
                                                _lib.MULTI_FRAMES_UNTOUCHED if untouched else 0, C.byref(step)),
              "multi render_batch_async")
        return int(step.value)

    def render_batch(self, frames, cameras, encode: int = ENCODE_SRGB):
        n, cams, ptr, pitch, stride = self._frames_args(frames, cameras)
        self._order_after_producer(frames)
        check(lib.kifs_multi_render_batch(self._m, n, cams, ptr, pitch, stride, encode), "multi render_batch")
        return frames

    def wait(self, step: int):
        check(lib.kifs_multi_wait(self._m, int(step)), f"multi wait({step})")

    def wait_all(self):
        check(lib.kifs_multi_wait_all(self._m), "multi wait_all")

    def stream_wait(self, step: int, stream):
        handle = stream.cuda_stream if hasattr(stream, "cuda_stream") else stream
        if not handle:
            raise ValueError("stream_wait: pass a non-default torch.cuda.Stream")
        check(lib.kifs_multi_stream_wait(self._m, int(step), handle), f"multi stream_wait({step})")

    def stats(self, reset: bool = False) -> dict:
        st = _lib.MultiStatsC()
        check(lib.kifs_multi_stats(self._m, C.byref(st), 1 if reset else 0), "multi stats")
        return {"steps": int(st.steps), "records_received": int(st.records_received), "tiles_covered": int(st.tiles_covered),
                "bytes_received": int(st.bytes_received),
                "transport": {0: "auto", 1: "rccl", 2: "copy"}[int(st.transport)],
                "gather": {0: "sparse", 1: "dense"}[int(st.gather)],
                "rccl_version": int(st.rccl_version), "comm_ranks": int(st.comm_ranks)}

    def comm_selftest(self, nbytes: int = 1 << 20):
        check(lib.kifs_multi_comm_selftest(self._m, int(nbytes)), "multi comm_selftest")

    def set_weights(self, weights=None):
        """Shares of the devices (one integer each, None = equal)."""
        arr = None if weights is None else (C.c_int * len(self.devices))(*[int(w) for w in weights])
        check(lib.kifs_multi_set_weights(self._m, arr), "multi set_weights")

    def shards(self):
        """[(device, n_stripes, rows, kernel ms of the last render)] per listed device."""
        res = []
        for i in range(len(self.devices)):
            d, n, rows = C.c_int(), C.c_int(), C.c_int()
            check(lib.kifs_multi_shard(self._m, i, C.byref(d), C.byref(n), C.byref(rows)))
            res.append((d.value, n.value, rows.value, float(lib.kifs_multi_shard_ms(self._m, i))))
        return res

    def close(self):
        if getattr(self, "_m", None):
            lib.kifs_multi_destroy(self._m)
            self._m = None

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def _check_host_destination(out: np.ndarray, rows: int, width: int, pitch: int):
    """A host destination must hold rows of `pitch` bytes: the library copies (rows-1)*pitch + 4*width
    bytes into it and knows nothing about the array's size."""
    if out.dtype != np.uint8 or not out.flags.c_contiguous:
        raise ValueError("render: host destination must be a C-contiguous uint8 array")
    if pitch < width * 4 or pitch % 4:
        raise ValueError("render: pitch_bytes must be a multiple of 4 and at least 4 * width")
    if rows > 0 and out.nbytes < (rows - 1) * pitch + width * 4:
        raise ValueError(f"render: host destination of {out.nbytes} bytes is too small for {rows} rows "
                         f"of pitch {pitch}")


def _stripe_array(stripes):
    return (C.c_int * len(stripes))(*[int(s) for s in stripes])


def shard_stripes(height: int, rank: int, world: int, weights=None):
    """kifs_shard_stripes: (stripe indices of `rank`, total rows) when the frame's 8-row stripes
    are dealt to `world` ranks (weights None: equal shares = stripes rank, rank + world, ...)."""
    cap = (height + STRIPE_ROWS - 1) // STRIPE_ROWS
    buf = (C.c_int * max(cap, 1))()
    n, rows = C.c_int(), C.c_int()
    wts = None if weights is None else (C.c_int * world)(*[int(x) for x in weights])
    check(lib.kifs_shard_stripes(height, world, wts, rank, buf, cap, C.byref(n), C.byref(rows)), "shard_stripes")
    return list(buf[:n.value]), rows.value


def band_range(height: int, rank: int, world: int):
    y0, y1 = C.c_int(), C.c_int()
    check(lib.kifs_band_range(height, rank, world, C.byref(y0), C.byref(y1)), "band_range")
    return y0.value, y1.value
