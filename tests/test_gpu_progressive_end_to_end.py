"""The consumers of progressive accumulation on a GPU: what hands out cameras, options and cells pass by pass -- the
viewer's refinement (ViewerSession(refine=), kifs_raymarching_amd/viewer.py), the --spp branch of tools/render.py and
graphics.Accumulator across streams -- held byte for byte to tests/progressive_reference.py (the unmodified oracle's
linear sub-frames carried through a plane in np.float32) and to ONE render_accumulate call over the concatenated views.
tests/test_progressive_viewer.py checks the same hand-out with fakes; here the pixels are checked.  74 x 45 (ten columns
past a tile edge, five rows past one) and the tool's 96 x 54; the scene is accumulate_cases' julia_24.

Accumulator across streams: two passes of one Accumulator on different streams are ordered by the wrapper
(Accumulator.add: kifs_order_after after a caller's stream, a host wait after the context's own).  The first pass is held
back by work enqueued on ITS stream, so that with nothing ordering them the second pass would run first and the first then
overwrite the plane with total 2: a wrong value, nothing that can fault, and not to be looped.  Run once with the wrapper's
ordering taken out, both cases passed all the same: accum::enqueue goes through anim::follow_stream_change, which orders a
launch after the previous launch on the same tile table when the stream changes (the feedback's buffer rotation needs it),
so on one context the passes of one band are in order by the scheduler's doing.  The contract does not promise that, the
wrapper no longer leans on it, and which calls the wrapper makes is pinned on the CPU
(tests/test_progressive_api.py::test_accumulator_orders_a_pass_after_the_previous_pass_on_another_stream); this test holds
the values whoever orders the passes.

Still not covered: passes handed from the context's own stream to a caller's WITHOUT a host wait (the header has no call
that names the context's stream as a producer), and prior near 2^24 anywhere but tests/test_gpu_progressive.py's refusals."""
import subprocess
import sys
from pathlib import Path

import numpy as np
import pytest

import accumulate_cases as AC
import jitter_reference as JR
import progressive_reference as PR
from helpers import oracle_uniforms

pytestmark = pytest.mark.gpu

ROOT = Path(__file__).resolve().parent.parent
W, H = AC.W, AC.H
CHILD_TIMEOUT = 120  # seconds: a child that renders 96 x 54 takes a few, most of it the interpreter and the imports
HOLD_PASSES = 384    # as tests/test_gpu_context_lifecycle.py::_hold_back: about 28 ms of GPU time


class Sink:
    def __init__(self):
        self.frames = []

    def present(self, frame, index):
        assert index == len(self.frames)
        self.frames.append(np.array(frame))

    def close(self):
        pass


def _same(got, want, what):
    assert got.shape == want.shape, (what, got.shape, want.shape)
    bad = (got != want).any(-1)
    assert not bad.any(), (what, int(bad.sum()), np.argwhere(bad)[:3].tolist(), got[bad][:2].tolist(), want[bad][:2].tolist())


def _same_plane(texels, want, total, what):
    """Every f32 bit pattern: the sums, and w == float(total)."""
    assert texels.shape == want.shape, (what, texels.shape, want.shape)
    bad = (texels.view(np.uint32) != want.view(np.uint32)).any(-1)
    assert not bad.any(), (what, int(bad.sum()), np.argwhere(bad)[:3].tolist(), texels[bad][:2].tolist(), want[bad][:2].tolist())
    assert (texels[..., 3] == np.float32(total)).all(), what


def _plain(oracle, kifs, screen, cam, gui, iters):
    s, c, o = oracle_uniforms(oracle, kifs, (screen, cam, gui))
    return oracle.render(s, c, o, oracle.iters(*iters))


def test_viewer_refinement_is_the_jittered_frame(kifs, oracle):
    """ViewerSession(GraphicState, [sink], refine=(3, 4, 2)): the plain frame, two refinements, nothing after the limit;
    then input, the plain frame of the moved camera and a refinement that starts over."""
    import copy
    from kifs_raymarching_amd.configs import jitter_cells
    from kifs_raymarching_amd.viewer import ViewerSession
    screen, cam, gui, iters = AC.scene(kifs, "julia_24")
    cells = jitter_cells(3, 4, 0) + jitter_cells(3, 4, 4)
    lin = JR.linear_views(oracle, kifs, screen, [cam] * 8, gui, iters, 3, cells, 8)  # every reference before the first launch
    _, _, after = PR.progressive_frames(oracle, kifs, screen, [cam] * 8, gui, iters, 8, 3, (4, 4), cells, lin=lin)
    plain = _plain(oracle, kifs, screen, cam, gui, iters)
    assert (after[0][0] != plain).any() and (after[1][0] != after[0][0]).any()  # from the references alone: refinement shows
    with kifs.GraphicState(0, screen_data=screen, camera_data=copy.deepcopy(cam), gui_data=gui) as g:
        g.set_iters(*iters)
        sink = Sink()
        s = ViewerSession(g, [sink], refine=(3, 4, 2))
        assert s.redraw() and len(sink.frames) == 1
        _same(sink.frames[0], plain, "the first frame")
        assert s.redraw() and s.redraw() and len(sink.frames) == 3 and s.passes_added == 2
        _same(sink.frames[1], after[0][0], "idle redraw 1 against the model")
        _same(sink.frames[2], after[1][0], "idle redraw 2 against the model")
        assert not s.redraw() and len(sink.frames) == 3 and s.frames_presented == 3  # the limit: nothing is presented
        plane = s.accumulator.sums.cpu().numpy()
        assert s.accumulator.total == 8 and (plane[..., 3] == np.float32(8.0)).all()
        for n in (4, 8):  # and against one call over the concatenated views
            whole = g.render_accumulate([cam] * n, n, jitter=(3, cells[:n]))
            g.synchronize()
            _same(sink.frames[n // 4], whole.cpu().numpy()[0], f"one call of {n} views")
        s.mouse_wheel(lines=1.0)
        moved = copy.deepcopy(g.camera_data)
        assert moved.origin_distance != cam.origin_distance
        assert s.redraw() and len(sink.frames) == 4 and s.passes_added == 0 and s.accumulator.total == 0
        _same(sink.frames[3], _plain(oracle, kifs, screen, moved, gui, iters), "the plain frame of the moved camera")
        assert s.redraw() and len(sink.frames) == 5 and s.accumulator.total == 4
        whole = g.render_accumulate([moved] * 4, 4, jitter=(3, cells[:4]))
        g.synchronize()
        _same(sink.frames[4], whole.cpu().numpy()[0], "refinement after the reset: one jittered call with the moved camera")
        want, want_plane, _ = PR.progressive_frames(oracle, kifs, screen, [moved] * 4, gui, iters, 4, 3, (4,), cells[:4])
        _same(sink.frames[4], want[0], "refinement after the reset: the model")
        _same_plane(s.accumulator.sums.cpu().numpy(), want_plane, 4, "the plane after the reset holds nothing of the old one")
        assert (sink.frames[4] != sink.frames[1]).any()
        s.close()


_CHILD_DIED = []  # a child that timed out or died on a signal: nothing else is started


def _render_tool(*args):
    """tools/render.py as a fresh child process with a time limit of its own; one at a time."""
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
    assert p.returncode == 0, (p.returncode, p.stdout, p.stderr)
    return p.stdout


SCALE = 0.05  # cfg2_julia_1080p at 96 x 54


def _tool_state(kifs):
    """A GraphicState configured as tools/render.py configures its own."""
    from kifs_raymarching_amd.configs import WORKLOADS
    w = WORKLOADS["cfg2_julia_1080p"]
    screen = kifs.ScreenData(max(1, int(w.screen.width * SCALE)), max(1, int(w.screen.height * SCALE)))
    assert (screen.width, screen.height) == (96, 54) and not w.extensions
    g = kifs.GraphicState(0, screen_data=screen, camera_data=w.camera, gui_data=w.gui)
    g.set_iters(*w.iters)
    return w, screen, g


def test_render_tool_spp_lens(kifs, oracle, tmp_path):
    """--dof 0.05,3.2 --spp 12 --jitter 2: three passes of 4 whose cells walk through the grid, against one call of the same
    12 lens cameras and the concatenated cells (the PNG files byte for byte: same writer, same pixels) and the model."""
    from kifs_raymarching_amd.configs import jitter_cells, lens_cameras, pass_splits
    from kifs_raymarching_amd.image import write_png
    w, screen, g = _tool_state(kifs)
    with g:
        cams = lens_cameras(w.camera, 0.05, 3.2, 12)
        cells = [c for d in (0, 4, 8) for c in jitter_cells(2, 4, d)]
        assert pass_splits(12, 4) == [4, 4, 4] and len(set(cells)) == 4
        lin = JR.linear_views(oracle, kifs, screen, cams, w.gui, w.iters, 2, cells, 12)
        want, _, after = PR.progressive_frames(oracle, kifs, screen, cams, w.gui, w.iters, 12, 2, (4, 4, 4), cells, lin=lin)
        assert (after[0] != want).any()  # the later passes show
        out = tmp_path / "tool.png"
        text = _render_tool("cfg2_julia_1080p", str(out), "--scale", str(SCALE), "--dof", "0.05,3.2", "--spp", "12", "--jitter", "2")
        assert "12 sub-frames in 3 passes" in text, text
        whole = g.render_accumulate(cams, 12, jitter=(2, cells))
        g.synchronize()
        frame = whole.cpu().numpy()[0]
        _same(frame, want[0], "one call against the model")
        write_png(str(tmp_path / "one_call.png"), frame)
        assert out.read_bytes() == (tmp_path / "one_call.png").read_bytes()
        write_png(str(tmp_path / "model.png"), want[0])
        assert out.read_bytes() == (tmp_path / "model.png").read_bytes()


def test_render_tool_spp_two_frames_in_one_accumulator(kifs, oracle, tmp_path):
    """--frames 0 1 --motion-blur 6 --spp 6 --jitter 2: two output frames in one Accumulator, passes of 4 + 2, frame k's
    cells starting at k."""
    from kifs_raymarching_amd.configs import jitter_cells, pass_splits, shutter_cameras
    from kifs_raymarching_amd.image import write_png
    w, screen, g = _tool_state(kifs)
    with g:
        assert pass_splits(6, 4) == [4, 2]
        cams = [c for k in (0, 1) for c in shutter_cameras(w, k, 6, 0.5)]
        cells = [c for k in (0, 1) for c in jitter_cells(2, 4, k) + jitter_cells(2, 2, k + 4)]
        lin = JR.linear_views(oracle, kifs, screen, cams, w.gui, w.iters, 2, cells, 6)
        want, _, _ = PR.progressive_frames(oracle, kifs, screen, cams, w.gui, w.iters, 6, 2, (4, 2), cells, lin=lin)
        assert (want[0] != want[1]).any()
        out = tmp_path / "orbit_%03d.png"
        _render_tool("cfg2_julia_1080p", str(out), "--scale", str(SCALE), "--frames", "0", "1", "--motion-blur", "6", "--spp", "6",
                     "--jitter", "2")
        whole = g.render_accumulate(cams, 6, jitter=(2, cells))
        g.synchronize()
        frames = whole.cpu().numpy()
        _same(frames, want, "one call against the model")
        for k in (0, 1):
            write_png(str(tmp_path / f"one_call_{k}.png"), frames[k])
            assert (tmp_path / ("orbit_%03d.png" % k)).read_bytes() == (tmp_path / f"one_call_{k}.png").read_bytes(), k


@pytest.mark.parametrize("first_on", ["caller", "own"])
def test_accumulator_orders_passes_across_streams(first_on, kifs, oracle):
    """acc.add(first, 2, picture=False, stream=s1) behind work that holds s1 back, then acc.add(rest, 2, stream=s2): picture
    and plane are the model's for 2 + 2.  "own": the first pass on the context's own stream (stream=None), which the
    wrapper orders after torch's current stream -- a side stream held back while that call is made; the second pass is
    then made with torch's current stream idle again."""
    import torch
    screen, cam, gui, iters = AC.scene(kifs, "julia_24")
    cams = AC.blur_cameras(kifs, cam, 2, 4)
    first, rest = [cams[0], cams[1], cams[4], cams[5]], [cams[2], cams[3], cams[6], cams[7]]
    cells_first, cells_rest = [(0, 1), (1, 0), (1, 1), (0, 0)], [(1, 1), (0, 0), (0, 1), (1, 0)]
    call_cells = cells_first[:2] + cells_rest[:2] + cells_first[2:] + cells_rest[2:]
    lin = JR.linear_views(oracle, kifs, screen, cams, gui, iters, 2, call_cells, 4)
    want, want_plane, _ = PR.progressive_frames(oracle, kifs, screen, cams, gui, iters, 4, 2, (2, 2), call_cells, lin=lin)
    with kifs.GraphicState(0, screen_data=screen, camera_data=cam, gui_data=gui) as g:
        g.set_iters(*iters)
        acc = kifs.Accumulator(g, count=2)
        warm = kifs.Accumulator(g, count=2)  # (the scene tables and the tile table exist before anything is held back)
        warm.add(first, 2, jitter=(2, cells_first))
        g.synchronize()
        out = torch.full((2, H, W, 4), 0xA5, dtype=torch.uint8, device="cuda:0")
        torch.cuda.synchronize()
        s1, s2 = torch.cuda.Stream(device=0), torch.cuda.Stream(device=0)
        with torch.cuda.stream(s1):  # torch's current stream outside this block stays idle
            held = torch.zeros(1 << 26, dtype=torch.float32, device="cuda:0")
            for _ in range(HOLD_PASSES):
                held.add_(1.0)
            if first_on == "own":
                assert acc.add(first, 2, picture=False, jitter=(2, cells_first)) is None
        if first_on == "caller":
            assert acc.add(first, 2, picture=False, stream=s1, jitter=(2, cells_first)) is None
        got = acc.add(rest, 2, outs=out, stream=s2, jitter=(2, cells_rest))
        s1.synchronize()
        s2.synchronize()
        g.synchronize()
        assert got is out and acc.total == 4
        plane = acc.sums.cpu().numpy()
        print("w words of the plane:", np.unique(plane[..., 3]).tolist())
        assert (plane[..., 3] == np.float32(4.0)).all(), np.unique(plane[..., 3]).tolist()
        _same_plane(plane, want_plane, 4, first_on)
        _same(out.cpu().numpy(), want, first_on)
        del held
