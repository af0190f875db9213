"""The tile order's feedback for batches on the GPU (kifs_render_common.hpp: cost_from_work; tile_order_kernel with its
memory; kifs_schedule.cpp: feedback_before / feedback_after), held to tests/tile_cost_model.py.  1080p Julia frames (60 x
135 tiles; Julia feedback starts at 2048 tiles), batches of 32 views on render_wave_kernel and of 4 and 8 views on
render_group_kernel, cameras moving along the orbit from launch to launch:
  * the cost table read back after a recording launch holds work -- within the range the shift was chosen for, zero for
    tiles no ray enters, positive wherever a view shows the fractal -- and is the same table on a second context;
  * after the sort the table is zero, the memory is the model's word for word (over two sorts, the second on top of the
    first), and the order is a permutation whose bins, taken from the memory, never decrease;
  * every checked frame of eight consecutive launches equals the frame a lone launch of another context renders, across a
    change of stream and a change of pipeline and back in the middle, and one of them equals the oracle's;
  * the memory's window runs out on the device as in the model (19 periods).
test_gpu_tile_cost_exact.py holds the recorded work to a model from the oracle's step traces, on ragged frames, Julia and
Sierpinski.  Frames below 2048 tiles have no feedback and are not here."""
import numpy as np
import pytest

import tile_cost_model as T
from helpers import oracle_frame

gpu = pytest.mark.gpu
TX, TY = 60, 135


@pytest.fixture(scope="module")
def work(kifs):
    import torch
    from kifs_raymarching_amd.configs import WORKLOADS, orbit_camera

    class Work:
        w = WORKLOADS["cfg2_julia_1080p"]
        frames = torch.zeros((32, 1080, 1920, 4), dtype=torch.uint8, device="cuda:0")
        lone_cache = {}

        def context(self):
            g = kifs.GraphicState(0, screen_data=self.w.screen, camera_data=self.w.camera, gui_data=self.w.gui)
            g.set_iters(*self.w.iters)
            return g

        def launch(self, g, first, count, stream):
            cams = [orbit_camera(self.w, first + i) for i in range(count)]
            g.render_batch_async([self.frames[i] for i in range(count)], cams, stream=stream)
            stream.synchronize()

        def lone(self, pose):
            if pose not in self.lone_cache:
                self.ref.set_camera(orbit_camera(self.w, pose))
                self.lone_cache[pose] = torch.from_numpy(self.ref.render()).to("cuda:0")
            return self.lone_cache[pose]

        def tiles_showing_the_fractal(self, count):
            f = self.frames[:count]
            hit = (f != f[0, 0, 0]).any(dim=-1).any(dim=0)  # (1080, 1920): some view's pixel is not the background
            return hit.reshape(TY, 8, TX, 32).any(dim=3).any(dim=1).reshape(-1).cpu().numpy()

    wk = Work()
    wk.ref = wk.context()
    yield wk
    wk.ref.close()


def check_recorded(wk, g, count, group_tiles):
    cost, seen, shift = g.debug_get_tile_costs()
    assert cost.shape == (TX * TY,) and shift == T.work_cost_shift(wk.w.gui.max_iterations, group_tiles)
    top = 4 * max(group_tiles, 1) * (wk.w.gui.max_iterations + T.WORK_PER_SHADED_CHUNK)
    assert 0 < cost.max() <= top and (cost.max() >> shift) <= 1023
    assert cost[0] == 0 and cost[TX - 1] == 0 and cost[-1] == 0  # the frame's corners: no ray enters the cull sphere
    shown = wk.tiles_showing_the_fractal(count)
    assert shown.sum() > 100 and (cost[shown] > 0).all()
    assert 100 < (cost > 0).sum() < TX * TY // 3
    return cost, seen, shift


def check_sorted(g, seen_before, cost, shift):
    cost_after, seen, _ = g.debug_get_tile_costs()
    assert not cost_after.any()
    assert (seen == T.remember(seen_before, cost, T.ORDER_WINDOW_BATCH)).all()
    order = g.debug_get_tile_order()
    index = (order & 0xffff).astype(np.int64) + (order >> 16).astype(np.int64) * TX
    assert (np.sort(index) == np.arange(TX * TY)).all()
    assert (np.diff(T.bins_along(order, seen >> 8, shift, TX)) >= 0).all()
    assert (order == T.stable_order(seen >> 8, shift, TX)).all()  # ties in tile-index order: the model's order, entry for entry
    return seen


@gpu
def test_wave_kernel_batches_record_work_remember_it_and_stay_exact(work, kifs, oracle):
    import torch
    from kifs_raymarching_amd.configs import WORKLOADS, orbit_camera
    wk, B = work, 32
    streams = [torch.cuda.Stream(), torch.cuda.Stream()]
    g = wk.context()
    wk.launch(g, 0, B, streams[0])  # launch 0 of the period: records
    assert g.debug_last_kernel() == "render_wave_kernel"
    cost0, seen0, shift = check_recorded(wk, g, B, 0)
    assert not seen0.any()
    g2 = wk.context()  # the same views on a second context: the same table
    wk.launch(g2, 0, B, streams[0])
    assert (g2.debug_get_tile_costs()[0] == cost0).all()
    g2.close()
    seen = seen0
    other = WORKLOADS["cfg3_sierpinski_1080p"]
    for j in range(1, 9):
        first = 17 * j
        if j == 6:  # another pipeline in between (no feedback for it at this size), and back
            g.update_options(other.gui)
            g.set_iters(*other.iters)
            wk.launch(g, first, B, streams[1])
            g.update_options(wk.w.gui)
            g.set_iters(*wk.w.iters)
        wk.launch(g, first, B, streams[0 if j < 4 else 1])  # (the caller changes streams before launch 4)
        assert g.debug_last_kernel() == "render_wave_kernel"
        for view in (0, 17, 31):
            assert torch.equal(wk.frames[view], wk.lone(first + view)), (j, view)
        if j == 1:
            seen = check_sorted(g, seen, cost0, shift)
        elif j == 3:
            cost3, seen3, _ = check_recorded(wk, g, B, 0)
            assert (seen3 == seen).all()  # only a sort writes the memory
        elif j == 4:
            seen = check_sorted(g, seen, cost3, shift)
            assert ((seen >> 8) >= np.maximum(cost0, cost3)).all()  # both sets of views are remembered
    want = oracle_frame(oracle, kifs, wk.w.screen, orbit_camera(wk.w, 17 * 8 + 17), wk.w.gui, wk.w.iters)
    assert (wk.frames[17].cpu().numpy() == want).all()
    g.close()


@gpu
@pytest.mark.parametrize("count", [4, 8])
def test_group_kernel_batches_record_work_remember_it_and_stay_exact(count, work, kifs):
    import torch
    wk = work
    stream = torch.cuda.Stream()
    g = wk.context()
    wk.launch(g, 40, count, stream)
    assert g.debug_last_kernel() == "render_group_kernel"
    tiles = g.debug_last_group_tiles()
    assert tiles in (1, 2)
    cost0, seen0, shift = check_recorded(wk, g, count, tiles)
    g2 = wk.context()
    wk.launch(g2, 40, count, stream)
    assert (g2.debug_get_tile_costs()[0] == cost0).all()
    g2.close()
    seen = seen0
    for j in range(1, 5):
        first = 40 + 9 * j
        wk.launch(g, first, count, stream)
        assert g.debug_last_kernel() == "render_group_kernel" and g.debug_last_group_tiles() == tiles
        for view in (0, count - 1):
            assert torch.equal(wk.frames[view], wk.lone(first + view)), (j, view)
        if j == 1:
            seen = check_sorted(g, seen, cost0, shift)
        elif j == 3:
            cost3, _, _ = check_recorded(wk, g, count, tiles)
        elif j == 4:
            seen = check_sorted(g, seen, cost3, shift)
    g.close()


@gpu
def test_the_memory_gives_a_cost_up_after_its_window_on_the_device(work):
    """One period on views A, then 18 periods on views B half an orbit away: after every sort the memory read back equals the
    model's, carried from sort to sort -- what A alone made long stays for ORDER_WINDOW_BATCH sorts and is gone afterwards --
    and the order is the stable model's."""
    import torch
    wk, count = work, 4
    stream = torch.cuda.Stream()
    g = wk.context()
    seen = np.zeros(TX * TY, dtype=np.uint32)
    first_sort = True
    only_a = None
    for period in range(19):
        first = 0 if period == 0 else 60
        wk.launch(g, first, count, stream)                      # k = 0: records
        cost, before, shift = g.debug_get_tile_costs()
        assert (before == seen).all()
        if period == 0:
            cost_a = cost
        elif period == 1:
            cost_b = cost
            only_a = cost_a > cost_b                            # tiles the first views made more work for
            assert only_a.sum() > 20
        wk.launch(g, first, count, stream)                      # k = 1: sorts
        seen = T.remember(seen, cost, 1 if first_sort else T.ORDER_WINDOW_BATCH)
        first_sort = False
        after, got, _ = g.debug_get_tile_costs()
        assert not after.any() and (got == seen).all(), period
        assert (g.debug_get_tile_order() == T.stable_order(seen >> 8, shift, TX)).all(), period
        if only_a is not None:
            want = cost_a if period < T.ORDER_WINDOW_BATCH else cost_b
            assert ((seen >> 8)[only_a] == want[only_a]).all(), period
        wk.launch(g, first, count, stream)                      # k = 2
    g.close()
