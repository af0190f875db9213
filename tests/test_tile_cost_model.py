"""The models of the tile order's feedback (tests/tile_cost_model.py) hold what the feedback promises, on the CPU: the sort
with a memory is a permutation, heaviest bin first, ties in index order; the memory keeps a tile's largest cost for `window`
sorts and then gives it up, and with a window of one it is the latest cost alone; the recorded work of a tile follows the
kernel's rounds and chunks; and work_cost_shift lands the top of every launch's range in the bins.  test_gpu_tile_cost.py
holds the kernels to the same models."""
import numpy as np
import pytest

import tile_cost_model as T


def costs(n, seed, live=0.05, top=1056):
    rng = np.random.default_rng(seed)
    c = np.zeros(n, dtype=np.uint32)
    m = rng.random(n) < live
    c[m] = rng.integers(1, top + 1, size=int(m.sum()), dtype=np.uint32)
    return c


@pytest.mark.parametrize("n,tiles_x", [(12, 3), (30, 5), (2048, 64), (8100, 60)])
@pytest.mark.parametrize("shift", [0, 1, 3])
def test_order_is_a_permutation_heaviest_first_ties_in_index_order(n, tiles_x, shift):
    for seed, live in ((1, 0.05), (2, 0.6), (3, 0.0), (4, 1.0)):
        c = costs(n, seed, live)
        order = T.stable_order(c, shift, tiles_x)
        index = (order & 0xffff).astype(np.int64) + (order >> 16).astype(np.int64) * tiles_x
        assert (np.sort(index) == np.arange(n)).all()
        b = T.bins_along(order, c, shift, tiles_x)
        assert (np.diff(b) >= 0).all()
        same = np.diff(b) == 0
        assert (np.diff(index)[same] > 0).all()
        if live == 0.0:
            assert (index == np.arange(n)).all()  # nothing recorded: the identity


def test_memory_keeps_the_largest_cost_for_a_window_of_sorts():
    n, window = 64, 5
    seen = np.zeros(n, dtype=np.uint32)
    history = []
    rng = np.random.default_rng(7)
    for s in range(40):
        c = rng.integers(0, 1000, size=n, dtype=np.uint32)
        if s % 9 == 0:
            c[3] = 5000  # a cost nothing else reaches
        history.append(c)
        seen = T.remember(seen, c, window)
        got = seen >> 8
        recent = np.max(history[-window:], axis=0)
        # never below the latest cost, never above the largest of the window; the outstanding cost is held exactly
        # `window` sorts
        assert (got >= c).all() and (got <= recent).all()
        assert (got[3] == 5000) == (s % 9 < window)
        assert ((seen & 0xff) < window).all()
    assert (T.remember(seen, history[-1], 1) >> 8 == history[-1]).all()  # a window of one: the latest costs alone


def test_memory_saturates_and_keeps_zero_tiles_last():
    seen = T.remember(np.zeros(4, dtype=np.uint32), np.array([0, 1, 0xffffffff, 1 << 20], dtype=np.uint32), 16)
    assert list(seen >> 8) == [0, 1, T.SEEN_COST_MAX, 1 << 20]
    order = T.stable_order(seen >> 8, 1, 2)
    assert list(order) == [0 | (1 << 16), 1 | (1 << 16), 0, 1]  # (cost 1 >> 1 is the empty bin too: index order)


def test_recorded_work_follows_the_rounds_and_chunks():
    # one chunk: marched to the end in one go -- the longest ray's steps
    assert T.wave_tile_work([5, 9, 200], 16, 256) == 200
    # 256 rays, all stopping at step 3: four chunks, one round
    assert T.wave_tile_work([3] * 256, 16, 256) == 12
    # 256 rays that never stop: four chunks x 256 steps, the top of the range; with four chunks of hits shaded
    assert T.wave_tile_work([256] * 256, 16, 256) == 1024
    assert T.cost_from_work(1024, 256) == 1024 + 4 * T.WORK_PER_SHADED_CHUNK
    # 65 long rays and 191 that stop at once: round one has four chunks (one of them runs 16 steps, the ones of short rays
    # one step), round two two chunks, and so on until 64 are left... here all 65 go on: two chunks per round to the end
    w = T.wave_tile_work([1] * 191 + [256] * 65, 16, 256)
    assert w == (1 + 1 + 16 + 16) + 2 * (256 - 16)
    assert T.cost_from_work(10 ** 9, 0) == T.COST_TOP
    # the group kernel: rounds of several chunks count in full, whatever their rays do; the last chunk as it ran
    assert T.group_work([3] * 256, 16, 256) == 4 * 16
    assert T.group_work([1] * 191 + [256] * 65, 16, 256) == 4 * 16 + 2 * (256 - 16)
    assert T.group_work([40] * 100 + [7], 16, 256) == 2 * 16 + 2 * 16 + 2 * 16  # (two chunks, three rounds: 40 > 32)
    assert T.group_work([200] * 512, 16, 256) <= 8 * 256
    assert T.group_work([20, 30], 16, 256) == 30 and T.group_work([20, 30], 16, 256, False) == 16 + 14


@pytest.mark.parametrize("max_iterations,group_tiles,want", [(256, 0, 1), (256, 1, 1), (256, 2, 2), (512, 0, 2), (100, 1, 0),
                                                             (119, 2, 0), (120, 2, 1), (10000, 2, 7)])
def test_shift_lands_the_top_of_the_range_in_the_bins(max_iterations, group_tiles, want):
    s = T.work_cost_shift(max_iterations, group_tiles)
    assert s == want
    top = 4 * max(group_tiles, 1) * (max_iterations + T.WORK_PER_SHADED_CHUNK)
    assert (top >> s) <= 1023 and (s == 0 or (top >> (s - 1)) > 1023)
    assert T.work_cost_shift(max_iterations, group_tiles, round_steps=0) == 0


def test_the_queue_model_on_tiles_traced_by_the_oracle(kifs, oracle):
    """The exact queue model (wave_queue_work: what test_gpu_tile_cost_exact.py holds the kernel to) on real rays: tiles of
    a 256 x 64 Julia frame, every pixel traced by the oracle (kor_march_trace).  Whatever the queue's order, the count lies
    between what the rays need -- the longest ray's steps, and a 64th of all steps -- and the group kernel's rule, which
    counts every chunk of a round in full; and a queue of one chunk costs its longest ray."""
    import tile_cost_exact as X
    screen = kifs.ScreenData(256, 64)
    gui = kifs.GuiData(fractal_group=kifs.FractalGroup.JuliaSet, max_iterations=64, max_distance=2.0e15, epsilon=1e-3)
    cam = kifs.CameraData(origin_distance=3.2, min_distance=1.0, phi=0.4, theta=0.25)
    seen_costs = set()
    for tile in (0, 3, 27, 28, 36, 63):
        x0, y0 = (tile % 8) * 32, (tile // 8) * 8
        pix = T.wave_arrival_order([[True] * 32] * 8)
        steps = X.ray_steps(oracle, kifs, screen, cam, gui, (8, 10, 10), [(x0 + lx, y0 + ly) for ly, lx in pix])
        assert len(steps) == 256 and min(steps) >= 1 and max(steps) <= 64
        for rounds in (4, 16):
            w = T.wave_queue_work(steps, rounds, 64)
            assert max(max(steps), -(-sum(steps) // 64)) <= w <= T.group_work(steps, rounds, 64) <= 4 * 64
            assert T.wave_queue_work(steps[:64], rounds, 64) == max(steps[:64])
            assert T.wave_queue_work(steps, rounds, 64) >= T.wave_queue_work(sorted(steps)[:200], rounds, 64)
            seen_costs.add(w)
    assert len(seen_costs) >= 3
