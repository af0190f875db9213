"""The consumers of ray queries on a GPU: GraphicState.trace_rays with a packed tensor and with an origin / direction
pair, on the context's stream and on a side stream, and the two branches of tools/render.py built on it -- --panorama
(the equirectangular picture, byte for byte the CPU reference's over configs.panorama_rays) and --focus-at (the focus
distance of --dof from the traced pixel; a pixel that misses ends the run with status 1)."""
import subprocess
import sys
from pathlib import Path

import numpy as np
import pytest

import ray_cases
import ray_reference as RR
from geometry_cases import cases

pytestmark = pytest.mark.gpu

ROOT = Path(__file__).resolve().parent.parent
CHILD_TIMEOUT = 120  # seconds: a child that renders 64 x 64 takes a few, most of it the interpreter and the imports
WORKLOAD, SCALE = "cfg1_julia_256", 0.25  # 64 x 64


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def test_trace_rays_takes_a_packed_tensor_or_a_pair_on_either_stream(kifs, oracle):
    import torch
    _, _, gui, iters = cases(kifs, 64, 48)["sierpinski"]
    rays, _ = ray_cases.rays(2)
    rays = rays[:777]
    want_geom, want_rgba, _ = RR.trace_scene(oracle, kifs, gui, iters, rays)
    with kifs.GraphicState(0, gui_data=gui) as g:
        g.set_iters(*iters)
        packed = torch.from_numpy(rays).to("cuda:0")
        side = torch.cuda.Stream(device="cuda:0")
        for stream in (None, side):
            for arg in (packed, (rays[:, 0:3], rays[:, 4:7]), (packed[:, 0:3], packed[:, 4:7])):
                geom, rgba = g.trace_rays(arg, stream=stream)
                if stream is None:
                    g.synchronize()
                else:
                    stream.synchronize()
                assert tuple(geom.shape) == (777, 4) and geom.dtype == torch.float32
                assert tuple(rgba.shape) == (777, 4) and rgba.dtype == torch.uint8
                assert (_bits(geom.cpu().numpy()) == _bits(want_geom)).all()
                assert (rgba.cpu().numpy() == want_rgba).all()
        geom, none = g.trace_rays(packed, colours=False)
        g.synchronize()
        assert none is None and (_bits(geom.cpu().numpy()) == _bits(want_geom)).all()
        none, rgba = g.trace_rays(packed, geometry=False, encode=kifs.ENCODE_UNORM)
        g.synchronize()
        assert none is None and (rgba.cpu().numpy() == RR.trace_scene(oracle, kifs, gui, iters, rays, encode=0)[1]).all()
        empty = g.trace_rays(packed[:0])
        assert tuple(empty[0].shape) == (0, 4) and tuple(empty[1].shape) == (0, 4)
        with pytest.raises(ValueError):
            g.trace_rays(packed, colours=False, geometry=False)
        with pytest.raises(ValueError):
            g.trace_rays(packed[:, :7])
        with pytest.raises(ValueError):
            g.trace_rays((rays[:, 0:3], rays[:5, 4:7]))


_CHILD_DIED = []  # a child that timed out or died on a signal: nothing else is started


def _render_tool(*args):
    """tools/render.py as a fresh child process with a time limit of its own; one at a time.  (status, stdout)."""
    assert not _CHILD_DIED, f"an earlier child of this module did not end in order: {_CHILD_DIED}"
    cmd = [sys.executable, str(ROOT / "tools" / "render.py"), *args]
    try:
        p = subprocess.run(cmd, capture_output=True, text=True, timeout=CHILD_TIMEOUT)
    except subprocess.TimeoutExpired as e:
        _CHILD_DIED.append(("timeout", args))
        pytest.fail(f"tools/render.py {args}: no end after {CHILD_TIMEOUT} s\n{e.stdout}\n{e.stderr}")
    if p.returncode < 0:
        _CHILD_DIED.append((p.returncode, args))
        pytest.fail(f"tools/render.py {args}: ended by signal {-p.returncode}\n{p.stdout}\n{p.stderr}")
    return p.returncode, p.stdout + p.stderr


def test_render_tool_panorama(kifs, oracle, tmp_path):
    from kifs_raymarching_amd.configs import WORKLOADS, panorama_rays
    from kifs_raymarching_amd.image import write_png
    w = WORKLOADS[WORKLOAD]
    origin = (0.5, -1.0, 0.25)
    rays = panorama_rays(origin, 64, 32)
    geom, rgba, _ = RR.trace_scene(oracle, kifs, w.gui, w.iters, rays)
    hit = RR.hits(geom)
    assert 100 < hit.sum() < hit.size - 100  # from the reference alone: the picture shows the set and the background
    out = tmp_path / "pano.png"
    status, text = _render_tool(WORKLOAD, str(out), "--scale", str(SCALE), "--panorama", ",".join(str(v) for v in origin))
    assert status == 0, text
    assert "64x32 equirectangular" in text and f"{int(hit.sum())} rays hit" in text, text
    write_png(str(tmp_path / "model.png"), rgba.reshape(32, 64, 4))
    assert out.read_bytes() == (tmp_path / "model.png").read_bytes()


def _pixel_reference(kifs, oracle, x, y):
    """(ray, t, focus distance in f32) of pixel (x, y) of the tool's frame, from the CPU reference."""
    from kifs_raymarching_amd.configs import WORKLOADS, pixel_rays
    w = WORKLOADS[WORKLOAD]
    screen = kifs.ScreenData(int(w.screen.width * SCALE), int(w.screen.height * SCALE))
    ray = pixel_rays(screen, w.camera)[y * screen.width + x]
    geom, _, _ = RR.trace_scene(oracle, kifs, w.gui, w.iters, ray[None])
    m0 = np.array(w.camera.into_buffer_data().matrix[0][:3], dtype=np.float32)
    d = ray[4:7]
    return w, screen, geom[0, 3], geom[0, 3] * ((d[0] * -m0[0] + d[1] * -m0[1]) + d[2] * -m0[2])


def test_render_tool_focus_at_a_pixel_that_hits(kifs, oracle, tmp_path):
    from kifs_raymarching_amd.configs import lens_cameras
    from kifs_raymarching_amd.image import write_png
    w, screen, t, focus = _pixel_reference(kifs, oracle, 32, 30)
    assert np.isfinite(t) and 3.0 < focus < 5.0  # from the reference alone: the centre of the frame shows the set
    out = tmp_path / "focus.png"
    status, text = _render_tool(WORKLOAD, str(out), "--scale", str(SCALE), "--dof", "0.05", "--focus-at", "32,30", "--samples", "4")
    assert status == 0, text
    assert f"hit at t = {float(t):.6g}, focus distance {float(focus):.6g}" in text, text
    assert f"focus at {float(focus)}" in text, text
    # the picture is the accumulated call's for that distance
    with kifs.GraphicState(0, screen_data=screen, camera_data=w.camera, gui_data=w.gui) as g:
        g.set_iters(*w.iters)
        frames = g.render_accumulate(lens_cameras(w.camera, 0.05, float(focus), 4), 4)
        g.synchronize()
        write_png(str(tmp_path / "model.png"), frames.cpu().numpy()[0])
    assert out.read_bytes() == (tmp_path / "model.png").read_bytes()


def test_render_tool_focus_at_a_pixel_that_misses(kifs, oracle, tmp_path):
    _, _, t, _ = _pixel_reference(kifs, oracle, 1, 1)
    assert np.isinf(t)  # from the reference alone: the corner shows the background
    out = tmp_path / "focus.png"
    status, text = _render_tool(WORKLOAD, str(out), "--scale", str(SCALE), "--dof", "0.05", "--focus-at", "1,1", "--samples", "4")
    assert status == 1, (status, text)
    assert "misses the scene" in text and not out.exists()
