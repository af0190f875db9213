"""kifs_raymarching_amd -- MI355X-native raymarching hot path of kifs-raymarching.

(The repository brief names the package `kifs-raymarching_amd`; Python cannot import a
hyphenated name, so the directory uses an underscore.)

Importing this package loads libkifs_hip.so and fails loudly if it is missing: there is
no CPU or PyTorch fallback for the render path.
"""
from . import _lib  # noqa: F401  (raises ImportError when the HIP library is absent)
from ._lib import ENCODE_SRGB, ENCODE_UNORM, MAX_FOLD_TRAP_BATCH, KifsError
from .graphics import (MAX_ACCUMULATE, MAX_BATCH, MAX_JITTER_GRID, Accumulator, AmbientOcclusion, Light, OrbitTrap, FoldSystem, ConvergingAccumulator, CameraData, DevicePointers, camera_array, FractalGroup, GraphicState, GuiData, MultiGraphicState,
                       PrimitiveShape, ScreenData, band_range, options_array, shard_stripes, uniform_bytes)

__all__ = ["GraphicState", "MultiGraphicState", "ScreenData", "CameraData", "GuiData", "FractalGroup",
           "PrimitiveShape", "KifsError", "ENCODE_SRGB", "ENCODE_UNORM", "band_range",
           "uniform_bytes", "MAX_BATCH", "shard_stripes", "DevicePointers", "camera_array",
           "options_array", "MAX_ACCUMULATE", "MAX_JITTER_GRID", "Accumulator", "ConvergingAccumulator", "AmbientOcclusion", "Light", "OrbitTrap", "FoldSystem", "MAX_FOLD_TRAP_BATCH"]
