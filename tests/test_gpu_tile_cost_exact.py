"""The cost tables of the throughput kernels against a model built from the CPU oracle's per-ray step traces
(kor_march_trace), word for word.  The traces know nothing of the kernels' culls, so the scenes here switch them off the
way the library itself does (max_distance at 2e15: fill_params' `sane`): every pixel's ray is live and stops after exactly
the oracle's number of steps, and what is left to model is the counting -- rounds, chunks, the queue's order, the hit
chunks' term, the maximum over a batch's views -- in tests/tile_cost_model.py.  Frames with ragged right and bottom tiles:
Julia 2040 x 516 (64 x 65 tiles; Julia feedback from 2048) as a lone frame, 2 and 4 views, which the shape rules take to
render_group_kernel with one tile, with two tiles and to render_wave_kernel; Sierpinski 4090 x 1028 (128 x 129 tiles; KIFS
feedback from 16 384) with 1 and 2 views; and batches of 2 and 3 views of both FORCED onto each of the three forms in child
processes (tests/tile_cost_exact.py holds the check itself).  The model is evaluated on a sample of tiles -- the frame's corners and ragged
edges, its centre, a seeded draw -- because a trace is one oracle call per pixel.  Then the sort: the order equals the
stable model's, entry for entry; and a batch that looks away from the fractal records nothing and gets the identity."""
import os
import subprocess
import sys
from pathlib import Path

import numpy as np
import pytest

import kernel_forms as F
import tile_cost_exact as X

gpu = pytest.mark.gpu
ROOT = Path(__file__).resolve().parent.parent


@gpu
@pytest.mark.parametrize("scene,count,form", [("julia", 1, "group1"), ("julia", 2, "group2"), ("julia", 4, "wave"),
                                              ("sierpinski", 1, "group2"), ("sierpinski", 2, "wave")])
def test_recorded_work_equals_the_model_from_the_oracles_traces(scene, count, form, kifs, oracle):
    """The forms the shape rules choose by themselves, in this process."""
    assert X.check_exact(kifs, oracle, scene, count, X.FORM[form]) >= 8


@gpu
@pytest.mark.parametrize("form", ["group1", "group2", "wave"])
def test_batches_of_two_and_three_views_forced_onto_every_form(form):
    """Batches of 2 and 3 views forced onto render_group_kernel with one tile, with two tiles and onto render_wave_kernel
    (KIFS_TUNING=1 KIFS_GROUP_TILES=n, read once per process: a child, as tests/kernel_forms.py runs its forms)."""
    run = subprocess.run([sys.executable, str(ROOT / "tests" / "tile_cost_exact.py"), form], capture_output=True, text=True,
                         timeout=240, env=F.child_env(os.environ, form))
    assert run.returncode == 0, (run.stdout[-1500:], run.stderr[-3000:])
    assert f"tile_cost_exact: {form}: 3 cases" in run.stdout, run.stdout[-1500:]
    print(run.stdout.strip().splitlines()[-1])


@gpu
def test_a_batch_that_looks_away_records_nothing_and_gets_the_identity(kifs):
    import torch
    from kifs_raymarching_amd.configs import WORKLOADS, orbit_camera
    w = WORKLOADS["cfg2_julia_1080p"]
    g = kifs.GraphicState(0, screen_data=w.screen, camera_data=w.camera, gui_data=w.gui)
    g.set_iters(*w.iters)
    images = []
    for i in range(3):
        u = orbit_camera(w, 7 * i).into_buffer_data()
        for r in range(3):
            for a in range(3):
                u.matrix[r][a] = -u.matrix[r][a]  # every ray's direction reversed: all of them leave the scene behind
        images.append(u)
    frames = torch.zeros((3, 1080, 1920, 4), dtype=torch.uint8, device="cuda:0")
    stream = torch.cuda.Stream()
    for _ in range(2):  # record, then sort
        g.render_batch_async([frames[i] for i in range(3)], kifs.camera_array(images), stream=stream)
        stream.synchronize()
        cost, seen, _ = g.debug_get_tile_costs()
        assert not cost.any() and not seen.any()
    assert (frames == frames[0, 0, 0]).all()
    ids = np.arange(60 * 135)
    assert (g.debug_get_tile_order() == ((ids % 60) | ((ids // 60) << 16))).all()
    g.close()
