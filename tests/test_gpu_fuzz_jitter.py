"""A seeded handful of random jittered accumulated launches (kifs_render_accumulate_jittered_async) against
tests/jitter_reference.py, every byte: random pipeline, grid, samples, cells (given, or NULL where samples == grid^2), band,
encode and per-sub-frame options, on frames of at most 48 x 24 with sentinel-filled destinations."""
import ctypes as C

import numpy as np
import pytest

import accumulate_cases as AC
import jitter_reference as JR
from geometry_cases import PIPELINES, Raw

pytestmark = pytest.mark.gpu

SENT = 0x5A
CASES = 12


def _case(K, seed):
    rng = np.random.default_rng(20261019 + seed)
    name = PIPELINES[int(rng.integers(0, len(PIPELINES)))] if seed >= len(PIPELINES) else PIPELINES[seed]
    w, h = int(rng.integers(9, 49)), int(rng.integers(3, 25))
    g = int(rng.integers(1, K.MAX_JITTER_GRID + 1))
    null_cells = bool(rng.integers(0, 3) == 0)
    samples = g * g if null_cells else int(rng.integers(1, 10))
    count = int(rng.integers(1, 4)) if samples <= 16 else 1
    views = count * samples
    cells = None if null_cells else [(int(rng.integers(0, g)), int(rng.integers(0, g))) for _ in range(views)]
    y0 = int(rng.integers(0, h))
    y1 = int(rng.integers(y0 + 1, h + 1))
    if rng.integers(0, 2):
        y0, y1 = 0, h
    return dict(name=name, w=w, h=h, g=g, samples=samples, count=count, cells=cells, y0=y0, y1=y1, encode=int(rng.integers(0, 2)),
                varied=bool(rng.integers(0, 2)) and name != "unknown_id" and views <= 8, pad=4 * int(rng.integers(0, 5)), seed=seed)


@pytest.fixture(scope="module")
def ags(kifs):
    g = kifs.GraphicState(0)
    yield g
    g.close()


@pytest.mark.parametrize("seed", range(CASES))
def test_random_jittered_launch(seed, ags, kifs, oracle):
    import torch
    from kifs_raymarching_amd._lib import KifsSubpixel, OptionsUniform, lib
    p = _case(kifs, seed)
    screen, cam, gui, iters = AC.scene(kifs, p["name"], p["w"], p["h"])
    ags.update_screen_data(screen)
    ags.set_camera(cam)
    ags.update_options(gui.u if isinstance(gui, Raw) else gui)
    ags.set_iters(*iters)
    ags.set_extensions(soft_shadow=False)
    ags.set_supersampling(1)
    count, samples, g = p["count"], p["samples"], p["g"]
    if p["varied"]:
        options, cams = AC.varied(kifs, gui, cam, count, samples, seed=seed)
        for v in range(len(cams)):  # nearer than `varied` puts them, so that rays hit
            if v % samples != 1:
                cams[v] = kifs.CameraData(origin_distance=cam.origin_distance + 0.02 * v, phi=cam.phi + 0.03 * v, theta=cam.theta).into_buffer_data()
    else:
        options, cams = None, AC.blur_cameras(kifs, cam, count, samples)
    rows, pitch = p["y1"] - p["y0"], 4 * p["w"] + p["pad"]
    dest = torch.full((count, rows, pitch), SENT, dtype=torch.uint8, device="cuda:0")
    torch.cuda.synchronize()
    ptrs = (C.c_void_p * count)(*[dest[i].data_ptr() for i in range(count)])
    arr = None if options is None else (OptionsUniform * len(options))(*options)
    cells = None if p["cells"] is None else (KifsSubpixel * len(p["cells"]))(*[KifsSubpixel(i, j) for i, j in p["cells"]])
    st = lib.kifs_render_accumulate_jittered_async(ags._ctx, None, count, samples, kifs.camera_array(cams), arr, g, cells, ptrs, pitch,
                                                   p["y0"], p["y1"], p["encode"])
    assert st == 0, p
    assert lib.kifs_synchronize(ags._ctx) == 0
    host = dest.cpu().numpy()
    got = host[:, :, :4 * p["w"]].reshape(count, rows, p["w"], 4)
    assert (host[:, :, 4 * p["w"]:] == SENT).all(), p
    want = JR.jittered_frames(oracle, kifs, screen, cams, options if options is not None else gui, iters, samples, g, p["cells"],
                              p["encode"], y0=p["y0"], y1=p["y1"])
    bad = (got != want).any(-1)
    assert not bad.any(), (p, int(bad.sum()), np.argwhere(bad)[:3].tolist(), got[bad][:2].tolist(), want[bad][:2].tolist())
