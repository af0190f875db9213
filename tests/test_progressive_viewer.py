"""ViewerSession's progressive refinement (kifs_raymarching_amd/viewer.py, refine = (grid, samples per pass, passes)) with
a fake renderer and a fake accumulator, no GPU: idle redraws add jittered passes up to the limit and then stop presenting,
every pass takes the cells configs.jitter_cells gives it and the renderer's camera, any input starts over, and a session
without `refine` is the session tests/test_viewer.py describes."""
import numpy as np
import pytest

from test_viewer import HostRenderer


class FakeAccumulator:
    """Records every add(); the frame it returns carries the number of sub-frames in it."""

    def __init__(self):
        self.total = 0
        self.adds = []
        self.resets = 0

    def add(self, cameras, samples, jitter=None, **kw):
        assert len(cameras) == samples and not kw
        self.total += samples
        self.adds.append((list(cameras), samples, jitter, self.total))
        f = np.zeros((1, 8, 16, 4), dtype=np.uint8)
        f[..., 0] = self.total
        f[..., 3] = 255
        return f

    def reset(self):
        self.resets += 1
        self.total = 0


class Sink:
    def __init__(self):
        self.frames = []

    def present(self, frame, index):
        assert index == len(self.frames)
        self.frames.append(np.array(frame))

    def close(self):
        pass


def test_idle_redraws_refine_up_to_the_limit(kifs):
    from kifs_raymarching_amd.configs import jitter_cells
    from kifs_raymarching_amd.viewer import ViewerSession
    r, acc, sink = HostRenderer(kifs), FakeAccumulator(), Sink()
    s = ViewerSession(r, [sink], refine=(4, 5, 3), accumulator=acc)
    assert s.redraw() and r.renders == 1 and not acc.adds      # the first redraw is the plain frame
    assert sink.frames[0].shape == (8, 16, 4) and sink.frames[0][0, 0, 2] == 1
    for p in range(3):                                         # nothing moves: one pass per redraw
        assert s.redraw()
        cams, samples, jitter, total = acc.adds[p]
        assert samples == 5 and total == 5 * (p + 1) and all(c is r.camera_data for c in cams)
        assert jitter == (4, jitter_cells(4, 5, frame=5 * p))
        assert sink.frames[1 + p].shape == (8, 16, 4) and sink.frames[1 + p][0, 0, 0] == 5 * (p + 1)
    assert jitter_cells(4, 5, 0) != jitter_cells(4, 5, 5) != jitter_cells(4, 5, 10)  # every pass its own cells
    assert not s.redraw() and not s.redraw()                   # the limit: nothing more is presented
    assert s.frames_presented == 4 == len(sink.frames) and r.renders == 1 and len(acc.adds) == 3 and s.passes_added == 3


def test_input_resets_the_accumulator(kifs):
    from kifs_raymarching_amd.configs import jitter_cells
    from kifs_raymarching_amd.viewer import ViewerSession
    r, acc, sink = HostRenderer(kifs), FakeAccumulator(), Sink()
    s = ViewerSession(r, [sink], refine=(3, 9, 8), accumulator=acc)
    assert s.redraw() and s.redraw() and s.redraw()            # the frame and two passes
    assert acc.total == 18 and s.passes_added == 2
    resets = acc.resets
    s.mouse_wheel(lines=1.0)                                   # input: the next redraw is the plain frame again
    moved = r.camera_data.origin_distance
    assert s.redraw() and r.renders == 2 and acc.resets == resets + 1 and acc.total == 0 and s.passes_added == 0
    assert sink.frames[-1][0, 0, 2] == 2 and len(acc.adds) == 2
    assert s.redraw()                                          # and refinement starts over, with the new camera
    cams, samples, jitter, total = acc.adds[-1]
    assert total == 9 and jitter == (3, jitter_cells(3, 9, frame=0)) and cams[0].origin_distance == moved
    s.mouse_button(True)
    s.mouse_motion(10.0, 0.0)
    s.request_redraw()
    assert s.redraw() and r.renders == 3 and acc.total == 0
    s.close()


def test_without_refine_the_session_is_as_before(kifs):
    from kifs_raymarching_amd.viewer import ViewerSession
    r, sink = HostRenderer(kifs), Sink()
    s = ViewerSession(r, [sink])
    assert s.refine is None and s.accumulator is None
    assert s.redraw() and not s.redraw() and not s.redraw()
    s.mouse_wheel(lines=1.0)
    assert s.redraw() and not s.redraw()
    assert s.frames_presented == 2 and r.renders == 2 and s.accumulator is None
    zero = ViewerSession(HostRenderer(kifs), [], refine=(2, 4, 0), accumulator=FakeAccumulator())  # no passes allowed
    assert zero.redraw() and not zero.redraw() and not zero.accumulator.adds
    for bad in ((0, 1, 1), (2, 5, 1), (2, 0, 1), (2, 4, -1)):
        with pytest.raises(ValueError):
            ViewerSession(r, [], refine=bad)
