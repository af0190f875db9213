"""The model of jittered accumulated frames (tests/jitter_reference.py) held to the oracle on the CPU, so that
tests/test_gpu_accumulate_jitter.py cannot pass vacuously: a grid of 1 is the accumulated model's frame; the whole grid in
supersampling order with one camera is aa_reference.aa_frame byte for byte (g = 2, 3); a jittered frame differs from the
unjittered one on a silhouette; and configs.grid_cells / jitter_cells are distinct, cover the grid at g^2, follow the
stated formula and refuse more than g^2."""
import math

import numpy as np
import pytest

import aa_reference as AA
import accumulate_cases as AC
import accumulate_reference as AR
import jitter_reference as JR

W, H = 42, 21  # ten columns past a tile edge, five rows past two: small, the oracle runs on the CPU


def test_a_grid_of_one_is_the_accumulated_model(oracle, kifs):
    screen, cam, gui, iters = AC.scene(kifs, "julia_24", W, H)
    cams = AC.blur_cameras(kifs, cam, 2, 3)
    want = AR.accumulate_frames(oracle, kifs, screen, cams, gui, iters, 3)
    assert (JR.jittered_frames(oracle, kifs, screen, cams, gui, iters, 3, 1, cells=[(0, 0)] * 6) == want).all()
    one = AR.accumulate_frames(oracle, kifs, screen, cams[:2], gui, iters, 1)
    assert (JR.jittered_frames(oracle, kifs, screen, cams[:2], gui, iters, 1, 1) == one).all()  # cells None: 1 == 1^2


@pytest.mark.parametrize("g", [2, 3])
@pytest.mark.parametrize("name", ["julia_24", "sphere"])
def test_the_whole_grid_in_order_is_the_supersampled_frame(name, g, oracle, kifs):
    screen, cam, gui, iters = AC.scene(kifs, name, W, H)
    for encode in (1, 0):
        want = AA.aa_frame(oracle, kifs, screen, cam, gui, iters, g, encode)
        got = JR.jittered_frames(oracle, kifs, screen, [cam] * (g * g), gui, iters, g * g, g, None, encode)
        assert got.shape == (1, H, W, 4) and (got[0] == want).all(), (name, g, encode)
        from kifs_raymarching_amd.configs import grid_cells
        given = JR.jittered_frames(oracle, kifs, screen, [cam] * (g * g), gui, iters, g * g, g, grid_cells(g), encode)
        assert (given == got).all()


def test_a_jittered_frame_differs_on_the_silhouette_only(oracle, kifs):
    screen, cam, gui, iters = AC.scene(kifs, "sphere", W, H)
    cams = [cam] * 3
    cells = [(0, 0), (2, 2), (1, 0)]
    plain = AR.linear_views(oracle, kifs, screen, cams, gui, iters)
    lin = JR.linear_views(oracle, kifs, screen, cams, gui, iters, 3, cells, 3)
    bg = np.array(list(AC.image(kifs, gui).background_color), dtype=np.float32)
    hit = (plain[0] != bg).any(-1)
    edge = np.zeros_like(hit)
    for v in range(3):
        edge |= hit ^ (lin[v] != bg).any(-1)  # a pixel the centre's ray hits and a cell's misses, or the other way round
    assert 0 < edge.sum() < hit.sum()
    got = JR.jittered_frames(oracle, kifs, screen, cams, gui, iters, 3, 3, cells, lin=lin)[0]
    flat = AR.accumulate_frames(oracle, kifs, screen, cams, gui, iters, 3, lin=plain)[0]
    differs = (got != flat).any(-1)
    assert differs[edge].any() and not differs[~hit & ~edge].any()  # far outside every ray misses: the same background
    # the centre cell of an odd grid is the pixel centre itself: the unjittered sub-frame, bit for bit
    mid = JR.linear_views(oracle, kifs, screen, cams[:1], gui, iters, 3, [(1, 1)], 1)
    assert (mid[0].view(np.uint32) == plain[0].view(np.uint32)).all()


def test_grid_cells_and_jitter_cells(kifs):
    from kifs_raymarching_amd.configs import grid_cells, jitter_cells
    for g in range(1, kifs.MAX_JITTER_GRID + 1):
        n = g * g
        cells = grid_cells(g)
        assert cells == [(s % g, s // g) for s in range(n)] and len(set(cells)) == n
        a = next(a for a in range(math.ceil(0.618 * n), 10 * n + 2) if math.gcd(a, n) == 1)
        assert a >= 0.618 * n and math.gcd(a, n) == 1 and (a == math.ceil(0.618 * n) or math.gcd(a - 1, n) != 1)
        for frame in (0, 1, 7):
            full = jitter_cells(g, n, frame)
            assert sorted(full) == sorted(cells)  # every cell exactly once
            for s, (i, j) in enumerate(full):
                assert 0 <= i < g and 0 <= j < g and j * g + i == ((s + frame) * a) % n, (g, frame, s)
            for samples in (0, 1, min(3, n), n - 1):
                part = jitter_cells(g, samples, frame)
                assert part == full[:samples] and len(set(part)) == samples
        assert jitter_cells(g, n) == jitter_cells(g, n, 0)
        with pytest.raises(ValueError):
            jitter_cells(g, n + 1)
    assert jitter_cells(4, 16)[:4] == [(0, 0), (3, 2), (2, 1), (1, 0)]  # a = 11: 0, 11, 6, 1
    if True:  # the order is not the supersampling order: the cell is unrelated to the sub-frame's time
        assert jitter_cells(4, 16) != grid_cells(4) and jitter_cells(4, 16, 1)[0] == (3, 2)
    with pytest.raises(ValueError):
        grid_cells(0)
    with pytest.raises(ValueError):
        jitter_cells(0, 0)
