"""The scenes the accumulated-frame tests share between the CPU (tests/test_accumulate_reference.py: the model and these
scenes against the oracle) and the GPU (tests/test_gpu_accumulate.py: the kernel against the model): the pipelines of
geometry_cases at 74 x 45 -- ten columns past a 32-pixel tile edge, five rows past an 8-row one -- with motion-blur
cameras from configs.shutter_cameras and per-sub-frame option images."""
import math

import numpy as np

from geometry_cases import PIPELINES, Raw, cases  # noqa: F401  (re-exported)

W, H = 74, 45
TURN = 24  # frames per turn of the test orbit: 15 degrees from frame to frame


def scene(K, name, width=W, height=H):
    """(screen, camera, gui, iters) of a pipeline."""
    return cases(K, width, height)[name]


def image(K, gui):
    """A fresh 80-byte options image of `gui` (GuiData, Raw or an image)."""
    from kifs_raymarching_amd._lib import OptionsUniform
    src = gui.into_buffer_data() if hasattr(gui, "into_buffer_data") else gui
    return OptionsUniform.from_buffer_copy(K.uniform_bytes(src))


def blur_cameras(K, cam, count, samples, shutter=1.0):
    """count * samples cameras: the sub-frames of `count` consecutive frames of an orbit of TURN frames per turn through
    the pipeline's camera (its distance and elevation, the frame nearest its azimuth first).  With the shutter open for
    the whole interval, neighbouring sub-frames are 15 / samples degrees apart: far enough to differ."""
    from kifs_raymarching_amd.configs import shutter_cameras
    first = int(round(cam.phi / (2.0 * math.pi / TURN)))
    out = []
    for f in range(count):
        out.extend(shutter_cameras((cam, TURN), first + f, samples, shutter))
    return out


def turned_away(K, cam):
    """The camera's image with its forward axis reversed: it looks away from the scene and every ray misses."""
    u = cam.into_buffer_data()
    for k in range(3):
        u.matrix[0][k] = -u.matrix[0][k]
    return u


def varied(K, gui, cam, count, samples, seed=0):
    """(options, cameras), count * samples of each: images of `gui`'s pipeline whose constant, power and both colours
    differ per sub-frame (padding words too: the contract ignores them), on cameras far enough out (distance 6) that
    whole tiles of the frame miss in every sub-frame; sub-frame 1 of every frame is turned away and misses everywhere."""
    options, cams = [], []
    for v in range(count * samples):
        u, k = image(K, gui), v + seed
        u.constant[0] += np.float32(0.03 * k)
        u.constant[1] -= np.float32(0.02 * k)
        u.constant[3] += np.float32(0.015 * k)
        u.power = np.float32(u.power + 0.25 * k)
        for ch in range(3):
            u.fractal_color[ch] = np.float32(0.15 + 0.2 * ((k + ch) % 4))
            u.background_color[ch] = np.float32(0.02 + 0.11 * ((k + 2 * ch) % 5))
        u._padding1, u._padding2, u._padding3 = 0xdead0000 + v, 17 * v, 0xffffffff
        options.append(u)
        c = K.CameraData(origin_distance=6.0 + 0.1 * (v % samples), phi=cam.phi + 0.05 * v, theta=cam.theta - 0.02 * v)
        cams.append(turned_away(K, c) if v % samples == 1 else c.into_buffer_data())
    return options, cams
