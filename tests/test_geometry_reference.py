"""tests/geometry_reference.c IS the oracle's march: for one scene per pipeline, every pixel's loop counter equals
kor_render_stats' and the colour rebuilt from the normal it hands out equals kor_shade_pixel bit for bit (no heatmap, no
shadows).  That is what makes the GPU comparison of tests/test_gpu_geometry.py mean something.  CPU only."""
import numpy as np
import pytest

import aa_reference as AA
import geometry_reference as GR
from geometry_cases import PIPELINES, cases
from helpers import oracle_uniforms

W, H = 75, 46


@pytest.mark.parametrize("name", PIPELINES)
def test_the_restatement_is_the_oracles_march(name, kifs, oracle):
    screen, cam, gui, iters = cases(kifs, W, H)[name]
    s, c, o = oracle_uniforms(oracle, kifs, (screen, cam, gui))
    it = oracle.iters(*iters)
    geom, hit, steps = GR.march(oracle, s, c, o, it)
    _, want_steps, stats = oracle.render_stats(s, c, o, it)
    assert (steps == want_steps).all(), int((steps != want_steps).sum())
    assert int(hit.sum()) == int(stats.hits)
    want = AA.linear_frame(oracle, s, c, o, it)
    got = GR.colour_from_geometry(oracle, o, geom, hit)
    assert GR.same_bits(got, want).all(), int((~GR.same_bits(got, want)).sum())
    # the texels themselves: misses are the miss texel, hits carry a finite t >= 0
    assert (geom[~hit].view(np.uint32) == GR.MISS).all()
    assert np.isfinite(geom[hit][:, 3]).all() and (geom[hit][:, 3] >= 0).all()
    if name != "unknown_id":  # (its SDF is the constant 1: nothing is ever hit)
        assert hit.any() and not hit.all()
    else:
        assert not hit.any()
