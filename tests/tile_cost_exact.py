"""What tests/test_gpu_tile_cost_exact.py checks for one scene, view count and kernel form: the cost table of a recording
launch against the model built from the oracle's step traces, word for word, then the sort.  In a module of its own because
the forms a batch's shape rules do not choose are forced by KIFS_GROUP_TILES under KIFS_TUNING=1, which the library reads
once per process: the test runs this file as a child with the environment of kernel_forms.child_env.
    python tests/tile_cost_exact.py FORM      (group1 | group2 | wave: every forced case of that form)"""
import ctypes as C
import sys
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parent.parent
for _p in (str(ROOT), str(ROOT / "tests")):
    if _p not in sys.path:
        sys.path.insert(0, _p)

import tile_cost_model as T  # noqa: E402
from helpers import oracle_frame, oracle_uniforms  # noqa: E402

# the cases forced in a child, per form: (scene, views)
FORCED = {"group1": (("julia", 2), ("julia", 3), ("sierpinski", 3)), "group2": (("julia", 2), ("julia", 3), ("sierpinski", 2)),
          "wave": (("julia", 2), ("julia", 3), ("sierpinski", 3))}
FORM = {"group1": ("render_group_kernel", 1), "group2": ("render_group_kernel", 2), "wave": ("render_wave_kernel", 0)}


def scenes(kifs):
    julia = kifs.GuiData(fractal_group=kifs.FractalGroup.JuliaSet, max_iterations=64, max_distance=2.0e15, epsilon=1e-3,
                         fractal_color=(250, 180, 90), background_color=(3, 5, 9))
    sierpinski = kifs.GuiData(fractal_group=kifs.FractalGroup.KaleidoscopicIFS, primitive_shape=kifs.PrimitiveShape.SierpinskiTetrahedron,
                              max_iterations=48, max_distance=2.0e15, epsilon=1e-3, fractal_color=(250, 180, 90), background_color=(3, 5, 9))
    return {"julia": (kifs.ScreenData(2040, 516), julia, (8, 10, 10)), "sierpinski": (kifs.ScreenData(4090, 1028), sierpinski, (100, 10, 6))}


def camera(kifs, i):
    return kifs.CameraData(origin_distance=3.2 + 0.3 * i, min_distance=1.0, phi=0.4 + 0.9 * i, theta=0.25 - 0.2 * i)


def ray_steps(oracle, kifs, screen, cam, gui, iters, pixels):
    f = oracle.lib().kor_march_trace
    f.restype = C.c_int
    s, c, o = oracle_uniforms(oracle, kifs, (screen, cam, gui))
    it = oracle.iters(*iters)
    scratch = (C.c_uint8 * 1)()
    args = (C.byref(s), C.byref(c), C.byref(o), C.byref(it))
    return [f(*args, C.c_int(x), C.c_int(y), scratch, C.c_int(0)) for x, y in pixels]


def sample_tiles(tx, ty, n, seed):
    rng = np.random.default_rng(seed)
    fixed = [0, tx - 1, (ty - 1) * tx, ty * tx - 1, (ty // 2) * tx + tx // 2, (ty // 2) * tx + tx // 2 - 1, (ty - 1) * tx + tx // 2,
             (ty // 2) * tx + tx - 1]
    return sorted(set(fixed) | set(int(i) for i in rng.integers(0, tx * ty, size=n)))


def check_exact(kifs, oracle, scene, count, want_form):
    """Renders `count` views of `scene`, demands the kernel form `want_form` = (kernel, tiles per workgroup) and holds the
    recorded costs, the memory and the order to the models.  Returns the number of workgroups compared."""
    import torch
    screen, gui, iters = scenes(kifs)[scene]
    Wd, Ht = screen.width, screen.height
    tx, ty = (Wd + 31) // 32, (Ht + 7) // 8
    cams = [camera(kifs, i) for i in range(count)]
    g = kifs.GraphicState(0, screen_data=screen, camera_data=cams[0], gui_data=gui)
    g.set_iters(*iters)
    frames = torch.zeros((count, Ht, Wd, 4), dtype=torch.uint8, device="cuda:0")
    stream = torch.cuda.Stream()
    g.render_batch_async([frames[i] for i in range(count)], cams, stream=stream)
    stream.synchronize()
    kernel, tiles, rounds = g.debug_last_kernel(), g.debug_last_group_tiles(), g.debug_last_round_steps()
    assert (kernel, tiles) == want_form and rounds > 0
    cost, seen, shift = g.debug_get_tile_costs()
    order = g.debug_get_tile_order()  # the order the recording launch ran in: which tiles shared a workgroup
    assert cost.shape == (tx * ty,) and shift == T.work_cost_shift(gui.max_iterations, tiles) and not seen.any()
    host = frames.cpu().numpy()
    bg = host[0, 0, 0].copy()
    for i in (0, count - 1):  # the frames are the oracle's
        assert (oracle_frame(oracle, kifs, screen, cams[i], gui, iters) == host[i]).all()
    index = (order & 0xffff).astype(np.int64) + (order >> 16).astype(np.int64) * tx
    group_of = {int(t): [int(u) for u in index[(k // max(tiles, 1)) * max(tiles, 1):(k // max(tiles, 1) + 1) * max(tiles, 1)]]
                for k, t in enumerate(index)}
    groups = {tuple(group_of[t]) for t in sample_tiles(tx, ty, 10 if scene == "julia" else 4, seed=count)}
    genjulia, checked = False, []
    for members in sorted(groups):
        per_view = []
        for v in range(count):
            steps, hits = [], 0
            for t in members:
                x0, y0 = (t % tx) * 32, (t // tx) * 8
                valid = [[x0 + lx < Wd and y0 + ly < Ht for lx in range(32)] for ly in range(8)]
                pix = T.wave_arrival_order(valid)
                steps += ray_steps(oracle, kifs, screen, cams[v], gui, iters, [(x0 + lx, y0 + ly) for ly, lx in pix])
                hits += int((host[v, y0:y0 + 8, x0:x0 + 32] != bg).any(axis=-1).sum())
            if kernel == "render_wave_kernel":
                march = T.wave_queue_work(steps, rounds, gui.max_iterations)
            else:
                march = T.group_work(steps, rounds, gui.max_iterations, not genjulia)
            per_view.append(T.cost_from_work(march, hits))
        for t in members:
            assert int(cost[t]) == max(per_view), (members, t, per_view)
        checked.append((members, max(per_view)))
    print(scene, count, kernel, tiles, 'tiles checked:', checked[:6], '...', len(checked), 'groups; distinct costs', len({c for _, c in checked}))
    assert len({c for _, c in checked}) >= 2  # (the sample is not one saturated value)
    # the same views again on a second context: the same table
    with kifs.GraphicState(0, screen_data=screen, camera_data=cams[0], gui_data=gui) as g2:
        g2.set_iters(*iters)
        g2.render_batch_async([frames[i] for i in range(count)], cams, stream=stream)
        stream.synchronize()
        assert (g2.debug_get_tile_costs()[0] == cost).all()
    if count > 1:  # the next launch sorts: the order is the stable model's, entry for entry
        g.render_batch_async([frames[i] for i in range(count)], cams, stream=stream)
        stream.synchronize()
        after, seen, _ = g.debug_get_tile_costs()
        assert not after.any() and (seen == T.remember(np.zeros_like(cost), cost, 1)).all()
        assert (g.debug_get_tile_order() == T.stable_order(seen >> 8, shift, tx)).all()
    g.close()
    return len(checked)


if __name__ == "__main__":
    import kifs_raymarching_amd as K
    import oracle as O
    O.build()
    form = sys.argv[1]
    total = 0
    for scene_, count_ in FORCED[form]:
        total += check_exact(K, O, scene_, count_, FORM[form])
    print(f"tile_cost_exact: {form}: {len(FORCED[form])} cases, {total} workgroups ok")
