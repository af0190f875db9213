"""The consumers of converging accumulation on a GPU -- graphics.ConvergingAccumulator, the --spp --tolerance branch of
tools/render.py, the viewer's refinement with a tolerance (ViewerSession(refine=, tolerance=)) -- and its passes
interleaved with other launches on one long-lived context, held byte for byte and bit for bit to
tests/converge_reference.py (the unmodified oracle's linear sub-frames carried through both planes in np.float32 under
the header's rule).  74 x 45 and the tool's 96 x 54; the scenes are converge_cases' julia_24 and cfg2_julia_1080p."""
import subprocess
import sys
from pathlib import Path

import numpy as np
import pytest

import accumulate_cases as AC
import converge_cases as CC
import converge_reference as CR
import jitter_reference as JR
import progressive_reference as PR

pytestmark = pytest.mark.gpu

ROOT = Path(__file__).resolve().parent.parent
W, H = CC.W, CC.H
CHILD_TIMEOUT = 120  # seconds: a child that renders 96 x 54 takes a few, most of it the interpreter and the imports
SCALE = 0.05         # cfg2_julia_1080p at 96 x 54
TOOL = dict(tolerance=1 / 8, min_samples=4, spp=24, grid=2, per_pass=4)
VIEW = dict(tolerance=1 / 8, min_samples=4, refine=(3, 4, 6))


def _same(got, want, what):
    assert got.shape == want.shape, (what, got.shape, want.shape)
    bad = (got != want).any(-1)
    assert not bad.any(), (what, int(bad.sum()), np.argwhere(bad)[:3].tolist(), got[bad][:2].tolist(), want[bad][:2].tolist())


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def _until_done(model):
    """The passes a consumer runs: up to and including the first after which no pixel is active."""
    for p, m in enumerate(model):
        if not m["counts"].any():
            return p + 1
    return len(model)


def tool_model(oracle, kifs):
    """What tools/render.py --dof 0.05,3.2 --spp 24 --jitter 2 --tolerance 1/8 --min-samples 4 hands out, and the model's
    passes over it."""
    from kifs_raymarching_amd.configs import WORKLOADS, jitter_cells, lens_cameras, pass_splits
    w = WORKLOADS["cfg2_julia_1080p"]
    screen = kifs.ScreenData(max(1, int(w.screen.width * SCALE)), max(1, int(w.screen.height * SCALE)))
    splits = pass_splits(TOOL["spp"], TOOL["per_pass"])
    cams = lens_cameras(w.camera, 0.05, 3.2, TOOL["spp"])
    cells = [c for p in range(len(splits)) for c in jitter_cells(TOOL["grid"], TOOL["per_pass"], p * TOOL["per_pass"])]
    lin = JR.linear_views(oracle, kifs, screen, cams, w.gui, w.iters, TOOL["grid"], cells, TOOL["spp"])
    model = CR.converged(oracle, PR.split_views(lin, 1, TOOL["spp"], splits), [(TOOL["tolerance"], TOOL["min_samples"])] * len(splits))
    return w, screen, splits, model


def viewer_model(oracle, kifs):
    from kifs_raymarching_amd.configs import jitter_cells
    screen, cam, gui, iters = AC.scene(kifs, "julia_24")
    g, s, passes = VIEW["refine"]
    cells = [c for p in range(passes) for c in jitter_cells(g, s, p * s)]
    lin = JR.linear_views(oracle, kifs, screen, [cam] * (s * passes), gui, iters, g, cells, s * passes)
    model = CR.converged(oracle, PR.split_views(lin, 1, s * passes, (s,) * passes), [(VIEW["tolerance"], VIEW["min_samples"])] * passes)
    return screen, cam, gui, iters, model


def test_converging_accumulator(kifs, oracle):
    screen, cam, gui, iters, cams, cells = CC.views(kifs, "julia_24", 2)
    lin = JR.linear_views(oracle, kifs, screen, cams, gui, iters, CC.GRID, cells, CC.SAMPLES)
    rule = (CC.tolerance("julia_24"), CC.MIN_SAMPLES)
    model = CR.converged(oracle, PR.split_views(lin, 2, CC.SAMPLES, CC.SPLITS), [rule] * 3)
    cam_p, cell_p = PR.pass_views(cams, 2, CC.SAMPLES, CC.SPLITS), PR.pass_views(cells, 2, CC.SAMPLES, CC.SPLITS)
    with kifs.GraphicState(0, screen_data=screen, camera_data=cam, gui_data=gui) as g:
        g.set_iters(*iters)
        acc = kifs.ConvergingAccumulator(g, count=2, tolerance=rule[0], min_samples=rule[1])
        for p in range(3):
            out = acc.add(cam_p[p], CC.PER_PASS, picture=p != 1, jitter=(CC.GRID, cell_p[p]))
            assert acc.active() == [int(c) for c in model[p]["counts"]] and acc.total == 4 * (p + 1)
            assert (out is None) == (p == 1)
            if out is not None:
                _same(out.cpu().numpy(), model[p]["frames"], ("picture", p))
            assert (_bits(acc.sums.cpu().numpy()) == _bits(model[p]["sums"])).all(), p
            assert (_bits(acc.moments.cpu().numpy()) == _bits(model[p]["moments"])).all(), p
            assert (acc.samples_per_pixel().cpu().numpy() == model[p]["sums"][..., 3]).all()
        assert 0 < model[2]["counts"].min() and not model[2]["mask"].all()
        acc.reset()  # the next pass restarts: the planes are not read
        acc.sums.fill_(float("nan"))
        acc.moments.fill_(float("nan"))
        out = acc.add(cam_p[0], CC.PER_PASS, jitter=(CC.GRID, cell_p[0]))
        assert acc.active() == [int(c) for c in model[0]["counts"]] and acc.total == 4
        _same(out.cpu().numpy(), model[0]["frames"], "after reset")
        assert (_bits(acc.sums.cpu().numpy()) == _bits(model[0]["sums"])).all()


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


def test_render_tool_stops_early(kifs, oracle, tmp_path):
    """--dof 0.05,3.2 --spp 24 --jitter 2 --tolerance 0.125 --min-samples 4: passes of 4 until no pixel is active -- fewer
    than the six the cap allows -- and the PNG of the last pass run, byte for byte the model's."""
    from kifs_raymarching_amd.image import write_png
    w, screen, splits, model = tool_model(oracle, kifs)
    run = _until_done(model)
    assert len(splits) == 6 and 1 < run < 6, [m["counts"].tolist() for m in model]  # from the oracle alone: it stops early
    out = tmp_path / "tool.png"
    text = _render_tool("cfg2_julia_1080p", str(out), "--scale", str(SCALE), "--dof", "0.05,3.2", "--spp", str(TOOL["spp"]), "--jitter",
                        str(TOOL["grid"]), "--tolerance", str(TOOL["tolerance"]), "--min-samples", str(TOOL["min_samples"]))
    assert f"{run} of 6 passes run (stopped early)" in text, text
    rays = float(model[run - 1]["sums"][..., 3].mean())
    assert f"{rays:.2f} rays per pixel" in text, (text, rays)
    write_png(str(tmp_path / "model.png"), model[run - 1]["frames"][0])
    assert out.read_bytes() == (tmp_path / "model.png").read_bytes()
    assert (model[run - 1]["frames"][0] != model[0]["frames"][0]).any()


class Sink:
    def __init__(self):
        self.frames = []

    def present(self, frame, index):
        assert index == len(self.frames)
        self.frames.append(np.array(frame))

    def close(self):
        pass


def test_viewer_refinement_stops_when_nothing_is_active(kifs, oracle):
    """ViewerSession(refine=(3, 4, 6), tolerance=1/8, min_samples=4): the plain frame, then idle redraws until no pixel is
    active -- before the six passes are used up -- and none after; input starts over."""
    import copy
    from kifs_raymarching_amd.viewer import ViewerSession
    screen, cam, gui, iters, model = viewer_model(oracle, kifs)
    run = _until_done(model)
    assert 1 < run < 6, [m["counts"].tolist() for m in model]
    with kifs.GraphicState(0, screen_data=screen, camera_data=copy.deepcopy(cam), gui_data=gui) as g:
        g.set_iters(*iters)
        sink = Sink()
        s = ViewerSession(g, [sink], refine=VIEW["refine"], tolerance=VIEW["tolerance"], min_samples=VIEW["min_samples"])
        assert s.redraw() and len(sink.frames) == 1 and not s.converged
        for p in range(run):
            assert s.redraw(), p
            _same(sink.frames[1 + p], model[p]["frames"][0], ("idle redraw", p))
        assert s.converged and s.passes_added == run and s.accumulator.active() == [0]
        assert not s.redraw() and not s.redraw() and len(sink.frames) == 1 + run
        assert (_bits(s.accumulator.sums.cpu().numpy()) == _bits(model[run - 1]["sums"])).all()
        s.mouse_wheel(lines=1.0)
        assert s.redraw() and s.passes_added == 0 and not s.converged and s.accumulator.total == 0
        assert s.redraw() and s.passes_added == 1 and s.accumulator.total == 4
        s.close()


def test_passes_interleaved_with_other_launches_on_one_context(kifs, oracle):
    """One long-lived context: converging passes with an animated launch, an accumulated launch and a resume pass of
    other views between them -- the scene-table ring is shared -- leave the model's planes, pictures and counts, and the
    launches in between leave the bytes they leave on their own."""
    import torch
    screen, cam, gui, iters, cams, cells = CC.views(kifs, "julia_24")
    lin = JR.linear_views(oracle, kifs, screen, cams, gui, iters, CC.GRID, cells, CC.SAMPLES)
    rule = (1 / 16, 4)
    model = CR.converged(oracle, PR.split_views(lin, 1, CC.SAMPLES, CC.SPLITS), [rule] * 3)
    options, other = AC.varied(kifs, gui, cam, 2, 4)
    with kifs.GraphicState(0, screen_data=screen, camera_data=cam, gui_data=gui) as g:
        g.set_iters(*iters)

        def between():
            a = g.render_animation(options[:4], cameras=other[:4])
            b = g.render_accumulate(other, 4, options=options)
            plane = torch.zeros((2, H, W, 4), dtype=torch.float32, device="cuda:0")
            c = g.render_accumulate_resume(plane, 0, other, 4, options=options)
            g.synchronize()
            return [t.cpu().numpy() for t in (a, b, c, plane)]

        alone = between()
        assert (alone[1] == alone[2]).all()  # a first resume pass is the accumulated call
        acc = kifs.ConvergingAccumulator(g, count=1, tolerance=rule[0], min_samples=rule[1])
        for p in range(3):
            out = acc.add(cams[4 * p:4 * p + 4], 4, jitter=(CC.GRID, cells[4 * p:4 * p + 4]))
            assert acc.active() == [int(model[p]["counts"][0])]
            _same(out.cpu().numpy(), model[p]["frames"], ("picture", p))
            assert (_bits(acc.sums.cpu().numpy()) == _bits(model[p]["sums"])).all(), p
            assert (_bits(acc.moments.cpu().numpy()) == _bits(model[p]["moments"])).all(), p
            again = between()
            for x, y in zip(alone, again):
                assert x.shape == y.shape and (x.view(np.uint8) == y.view(np.uint8)).all(), p
        assert g.debug_last_kernel() == "render_accumulate_kernel"
        plain = g.render()
        assert g.debug_last_kernel() != "render_accumulate_kernel" and tuple(plain.shape) == (H, W, 4)
