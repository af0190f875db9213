"""Jittered accumulated frames on the GPU (kifs_render_accumulate_jittered_async, accum::jitter_render_kernel), bit for
bit: every byte of every output frame equals tests/jitter_reference.py -- the unmodified oracle's linear colour of every
sub-frame at its cell's pixel of the virtual screen, summed in np.float32 in the contract's order, divided and encoded with
the oracle's encoder.  No tolerance.  Two identities pin the call from both sides: a grid of 1 gives
kifs_render_accumulate_async's bytes, and the whole grid in supersampling order with one camera gives the bytes of
kifs_set_supersampling + a batch render.  Frames are 74 x 45 (ten columns past a tile edge, five rows past one) unless a
case says otherwise, and every destination is pre-filled with a sentinel so that a missing or a stray store shows.  The
scenes are tests/accumulate_cases.py's; tests/test_jitter_reference.py holds the model to the oracle on the CPU."""
import ctypes as C

import numpy as np
import pytest

import aa_reference as AA
import accumulate_cases as AC
import accumulate_reference as AR
import jitter_reference as JR
from geometry_cases import PIPELINES, Raw

pytestmark = pytest.mark.gpu

W, H = AC.W, AC.H
BAD_ARG, BAD_SIZE = 7, 3
SENT = 0xA5
HOOKS = (9, "render_accumulate_kernel", 0, -1, -1)
CELLS_2x3 = [(0, 0), (2, 2), (1, 0), (2, 0), (0, 2), (1, 1)]  # of a 3 x 3 grid: two frames of three sub-frames


@pytest.fixture(scope="module")
def ags(kifs):
    g = kifs.GraphicState(0)
    yield g
    g.close()


def _setup(g, screen, cam, gui, iters):
    g.update_screen_data(screen)
    g.set_camera(cam)
    g.update_options(gui.u if isinstance(gui, Raw) else gui)
    g.set_iters(*iters)
    g.set_extensions(soft_shadow=False)
    g.set_supersampling(1)


def _cells(cells):
    from kifs_raymarching_amd._lib import KifsSubpixel
    return None if cells is None else (KifsSubpixel * len(cells))(*[KifsSubpixel(i, j) for i, j in cells])


def _call(g, kifs, cams, samples, grid, cells, options=None, y0=0, y1=None, encode=1, pitch=None, sync=True, dest=None,
          unjittered=False):
    """The raw entry point on sentinel-filled destinations: (status, (count, rows, pitch) uint8 device tensor)."""
    import torch
    from kifs_raymarching_amd._lib import OptionsUniform, lib
    w, h = g.screen_data.width, g.screen_data.height
    y1 = h if y1 is None else y1
    rows = y1 - y0
    pitch = 4 * w if pitch is None else pitch
    count = len(cams) // samples
    if dest is None:
        dest = torch.full((count, max(rows, 1), pitch), SENT, dtype=torch.uint8, device="cuda:0")
        torch.cuda.synchronize()
    ptrs = (C.c_void_p * count)(*[dest[i].data_ptr() for i in range(count)])
    arr = None if options is None else (OptionsUniform * len(options))(*options)
    cam_arr = kifs.camera_array(cams)
    if unjittered:
        st = lib.kifs_render_accumulate_async(g._ctx, None, count, samples, cam_arr, arr, ptrs, pitch, y0, y1, encode)
    else:
        st = lib.kifs_render_accumulate_jittered_async(g._ctx, None, count, samples, cam_arr, arr, grid, _cells(cells), ptrs, pitch,
                                                       y0, y1, encode)
    if sync:
        assert lib.kifs_synchronize(g._ctx) == 0
    return st, dest


def _pixels(dest, w):
    host = dest.cpu().numpy()
    return host[:, :, :4 * w].reshape(host.shape[0], host.shape[1], w, 4), host[:, :, 4 * w:]


def _hooks(g):
    from kifs_raymarching_amd._lib import lib
    return (lib.kifs_debug_last_kernel(g._ctx), g.debug_last_kernel(), g.debug_last_round_steps(), g.debug_last_group_tiles(),
            g.debug_last_bunny_form())


_LINEAR = {}  # the oracle's linear sub-frames, computed once per scene and shared by the encodes and tests that use it


def _want(key, oracle, kifs, screen, cams, options, iters, samples, grid, cells, encode, ext=None, y0=0, y1=None):
    if key not in _LINEAR:
        _LINEAR[key] = JR.linear_views(oracle, kifs, screen, cams, options, iters, grid, cells, samples, ext)
    return JR.jittered_frames(oracle, kifs, screen, cams, options, iters, samples, grid, cells, encode, lin=_LINEAR[key], y0=y0, y1=y1)


def _same(got, want, what):
    bad = (got != want).any(-1)
    assert got.shape == want.shape and not bad.any(), (what, int(bad.sum()), np.argwhere(bad)[:3].tolist(),
                                                        got[bad][:2].tolist(), want[bad][:2].tolist())


@pytest.mark.parametrize("name", PIPELINES)
@pytest.mark.parametrize("encode", [1, 0])
def test_every_pipeline_bit_exact(name, encode, ags, kifs, oracle):
    screen, cam, gui, iters = AC.scene(kifs, name)
    _setup(ags, screen, cam, gui, iters)
    cams = AC.blur_cameras(kifs, cam, 2, 3)
    st, dest = _call(ags, kifs, cams, 3, 3, CELLS_2x3, encode=encode)  # options NULL: the context's
    assert st == 0 and _hooks(ags) == HOOKS
    want = _want(("pipeline", name), oracle, kifs, screen, cams, gui, iters, 3, 3, CELLS_2x3, encode)
    _same(_pixels(dest, W)[0], want, name)


@pytest.mark.parametrize("g", [2, 3, 4])
@pytest.mark.parametrize("name", ["julia_24", "sphere"])
def test_the_whole_grid_is_the_supersampled_frame(name, g, ags, kifs, oracle):
    import torch
    screen, cam, gui, iters = AC.scene(kifs, name)
    _setup(ags, screen, cam, gui, iters)
    want = AA.aa_frame(oracle, kifs, screen, cam, gui, iters, g)
    st, dest = _call(ags, kifs, [cam] * (g * g), g * g, g, None)
    assert st == 0 and _hooks(ags) == HOOKS
    got = _pixels(dest, W)[0]
    _same(got[0], want, ("aa_frame", name, g))
    ssaa = torch.full((1, H, W, 4), SENT, dtype=torch.uint8, device="cuda:0")
    ags.set_supersampling(g)
    try:
        ags.render_batch_async([ssaa[0]], [cam])
        ags.synchronize()
    finally:
        ags.set_supersampling(1)
    _same(got, ssaa.cpu().numpy(), ("the supersampling kernel", name, g))


def test_a_grid_of_one_is_the_unjittered_call(ags, kifs, oracle):
    screen, cam, gui, iters = AC.scene(kifs, "julia_24")
    _setup(ags, screen, cam, gui, iters)
    cams = AC.blur_cameras(kifs, cam, 2, 3)
    for encode in (1, 0):
        st, plain = _call(ags, kifs, cams, 3, 0, None, encode=encode, unjittered=True)
        assert st == 0
        st, zero = _call(ags, kifs, cams, 3, 1, [(0, 0)] * 6, encode=encode)
        assert st == 0 and _hooks(ags) == HOOKS
        _same(_pixels(zero, W)[0], _pixels(plain, W)[0], ("zero cells", encode))
        _same(_pixels(zero, W)[0], AR.accumulate_frames(oracle, kifs, screen, cams, gui, iters, 3, encode), ("model", encode))
        st, one = _call(ags, kifs, cams, 1, 1, None, encode=encode)  # NULL: samples == 1 == 1 x 1, six frames
        assert st == 0
        st, batch = _call(ags, kifs, cams, 1, 0, None, encode=encode, unjittered=True)
        assert st == 0
        _same(_pixels(one, W)[0], _pixels(batch, W)[0], ("NULL cells", encode))


@pytest.mark.parametrize("name", ["julia_24", "sphere"])
def test_per_sub_frame_options(name, ags, kifs, oracle):
    """constant, power and both colours differ per sub-frame, whole tiles miss with differing backgrounds; the context
    holds ANOTHER pipeline's options while the call is made."""
    screen, cam, gui, iters = AC.scene(kifs, name)
    other = kifs.GuiData(primitive_shape=kifs.PrimitiveShape.Torus) if name != "sphere" else kifs.GuiData(fractal_group=kifs.FractalGroup.JuliaSet)
    _setup(ags, screen, cam, other, iters)
    options, cams = AC.varied(kifs, gui, cam, 2, 3)
    cells = [(1, 0), (0, 1), (1, 1), (0, 0), (1, 0), (0, 1)]
    for encode in (1, 0):
        st, dest = _call(ags, kifs, cams, 3, 2, cells, options=options, encode=encode)
        assert st == 0 and _hooks(ags) == HOOKS
        _same(_pixels(dest, W)[0], _want(("varied", name), oracle, kifs, screen, cams, options, iters, 3, 2, cells, encode), (name, encode))


def test_65_views_go_through_the_view_table(ags, kifs, oracle):
    from kifs_raymarching_amd.configs import jitter_cells
    screen, cam, gui, iters = AC.scene(kifs, "julia_24")
    _setup(ags, screen, cam, kifs.GuiData(), iters)
    options, cams = AC.varied(kifs, gui, cam, 13, 5, seed=1)
    for v, c in enumerate(cams):  # nearer than `varied` puts them: most of the frame hits
        if v % 5 != 1:
            cams[v] = kifs.CameraData(origin_distance=3.0 + 0.01 * v, phi=0.3 + 0.02 * v, theta=0.2).into_buffer_data()
    cells = [c for f in range(13) for c in jitter_cells(4, 5, f)]
    st, dest = _call(ags, kifs, cams, 5, 4, cells, options=options)
    assert st == 0 and _hooks(ags) == HOOKS
    want = _want(("views65", 0), oracle, kifs, screen, cams, options, iters, 5, 4, cells, 1)
    _same(_pixels(dest, W)[0], want, "13 x 5")
    assert (want[0] != want[12]).any()


def test_512_views_of_64_cells(ags, kifs, oracle):
    """8 x 64 at 40 x 13, a grid of 8: the LDS opt-in of the jitter kernel, every wave with 16 sub-frames, every cell of the
    grid used exactly once per frame."""
    from kifs_raymarching_amd.configs import jitter_cells
    screen, cam, gui, iters = AC.scene(kifs, "julia_24", 40, 13)
    _setup(ags, screen, cam, kifs.GuiData(), iters)
    cams = AC.blur_cameras(kifs, cam, 8, 64)
    options = []
    for v in range(512):
        u = AC.image(kifs, gui)
        u.constant[0] = np.float32(-0.2 + 0.0005 * v)
        u.fractal_color[1] = np.float32(0.2 + 0.0015 * v)
        u.background_color[2] = np.float32(0.001 * v)
        options.append(u)
    cells = [c for f in range(8) for c in jitter_cells(8, 64, f)]
    assert all(len(set(cells[64 * f:64 * f + 64])) == 64 for f in range(8))
    st, dest = _call(ags, kifs, cams, 64, 8, cells, options=options)
    assert st == 0 and _hooks(ags) == HOOKS
    frames = _pixels(dest, 40)[0]
    assert frames.shape == (8, 13, 40, 4)
    want = _want(("views512", 0), oracle, kifs, screen, cams, options, iters, 64, 8, cells, 1)
    _same(frames, want, "8 x 64")
    assert (want[0] != want[7]).any()


def test_five_samples_are_no_multiple_of_four(ags, kifs, oracle):
    screen, cam, gui, iters = AC.scene(kifs, "sierpinski")
    _setup(ags, screen, cam, gui, iters)
    cams = AC.blur_cameras(kifs, cam, 2, 5)
    cells = [(2, 1), (0, 0), (1, 2), (2, 2), (0, 1), (1, 1), (0, 2), (2, 0), (1, 0), (2, 1)]
    st, dest = _call(ags, kifs, cams, 5, 3, cells)
    assert st == 0
    _same(_pixels(dest, W)[0], _want(("five", 0), oracle, kifs, screen, cams, gui, iters, 5, 3, cells, 1), "2 x 5")


def test_band_and_padded_pitch(ags, kifs, oracle):
    """Rows [3, 38) into rows wider than 4 W: rows 3..37 of the whole frame -- pixel coordinates stay the frame's on the
    virtual screen too -- and the guard bytes beyond 4 W untouched."""
    screen, cam, gui, iters = AC.scene(kifs, "julia_24")
    _setup(ags, screen, cam, gui, iters)
    cams = AC.blur_cameras(kifs, cam, 2, 3)
    st, dest = _call(ags, kifs, cams, 3, 3, CELLS_2x3, y0=3, y1=38, pitch=4 * W + 32)
    assert st == 0
    frames, padding = _pixels(dest, W)
    assert frames.shape == (2, 35, W, 4) and padding.shape[-1] == 32 and (padding == SENT).all()
    _same(frames, _want(("pipeline", "julia_24"), oracle, kifs, screen, cams, gui, iters, 3, 3, CELLS_2x3, 1, y0=3, y1=38), "band")
    st, dest = _call(ags, kifs, cams, 3, 3, CELLS_2x3, y0=20, y1=20)  # an empty band: nothing to do, nothing written
    assert st == 0 and (dest.cpu().numpy() == SENT).all()


def test_heatmap_sub_frames(ags, kifs, oracle):
    screen, cam, gui, iters = AC.scene(kifs, "julia_24")
    heat = kifs.GuiData(**{**gui.__dict__, "is_heatmap": True, "fractal_color": (255, 128, 30)})
    _setup(ags, screen, cam, heat, iters)
    cams = AC.blur_cameras(kifs, cam, 2, 3)
    st, dest = _call(ags, kifs, cams, 3, 3, CELLS_2x3)
    assert st == 0
    want = _want(("heatmap", 0), oracle, kifs, screen, cams, heat, iters, 3, 3, CELLS_2x3, 1)
    _same(_pixels(dest, W)[0], want, "heatmap")
    assert (want != _want(("pipeline", "julia_24"), oracle, kifs, screen, cams, gui, iters, 3, 3, CELLS_2x3, 1)).any()


def test_soft_shadow_sub_frames(ags, kifs, oracle):
    screen, cam, gui, iters = AC.scene(kifs, "sierpinski")
    _setup(ags, screen, cam, gui, iters)
    cams = AC.blur_cameras(kifs, cam, 2, 3)
    ags.set_extensions(soft_shadow=True, shadow_steps=64, shadow_k=8.0, shadow_t0=0.02, shadow_max_t=10.0)
    try:
        st, dest = _call(ags, kifs, cams, 3, 3, CELLS_2x3)
    finally:
        ags.set_extensions(soft_shadow=False)
    assert st == 0
    want = _want(("shadow", 0), oracle, kifs, screen, cams, gui, iters, 3, 3, CELLS_2x3, 1, ext=oracle.Ext(1, 64, 8.0, 0.02, 10.0))
    _same(_pixels(dest, W)[0], want, "soft shadows")
    assert (want != _want(("pipeline", "sierpinski"), oracle, kifs, screen, cams, gui, iters, 3, 3, CELLS_2x3, 1)).any()


def test_six_calls_alternating_and_an_explicit_stream(ags, kifs, oracle):
    """Two calls more than the scene-table ring is deep without a wait between them, jittered and unjittered in turn: a
    table is rewritten only after the launch that read it, and an unjittered call's pad words are zero again.  Then the
    wrapper on a stream of the caller's."""
    import torch
    screen, cam, gui, iters = AC.scene(kifs, "julia_24")
    _setup(ags, screen, cam, kifs.GuiData(), iters)
    cells = [(1, 1), (0, 1), (1, 0)]
    calls = []
    for c in range(6):
        options, cams = AC.varied(kifs, gui, cam, 1, 3, seed=7 * c)
        for v in (0, 2):
            cams[v] = kifs.CameraData(origin_distance=3.0 + 0.1 * c, phi=0.3 + 0.1 * v, theta=0.1 * c).into_buffer_data()
        calls.append((options, cams, torch.full((1, H, 4 * W), SENT, dtype=torch.uint8, device="cuda:0")))
    torch.cuda.synchronize()
    for c, (options, cams, dest) in enumerate(calls):
        st, _ = _call(ags, kifs, cams, 3, 2, cells, options=options, sync=False, dest=dest, unjittered=bool(c % 2))
        assert st == 0
    ags.synchronize()
    wants = []
    for c, (options, cams, dest) in enumerate(calls):
        if c % 2:
            wants.append(AR.accumulate_frames(oracle, kifs, screen, cams, options, iters, 3))
        else:
            wants.append(_want(("ring", c), oracle, kifs, screen, cams, options, iters, 3, 2, cells, 1))
        _same(_pixels(dest, W)[0], wants[c], ("call", c))
    stream = torch.cuda.Stream(device=0)
    options, cams, _ = calls[2]
    out = ags.render_accumulate(cams, 3, options=options, stream=stream, jitter=(2, cells))
    stream.synchronize()
    assert tuple(out.shape) == (1, H, W, 4) and out.dtype == torch.uint8
    _same(out.cpu().numpy(), wants[2], "explicit stream")


def test_refusals_write_nothing(ags, kifs):
    screen, cam, gui, iters = AC.scene(kifs, "sierpinski", 40, 24)
    _setup(ags, screen, cam, gui, iters)
    cams = AC.blur_cameras(kifs, cam, 3, 2)
    good = [(0, 0), (2, 2), (1, 0), (2, 0), (0, 2), (1, 1)]

    def refused(want, grid, cells, samples=2, use=cams, **kw):
        st, dest = _call(ags, kifs, use, samples, grid, cells, **kw)
        assert st == want, (st, grid, cells, kw)
        assert (dest.cpu().numpy() == SENT).all(), (grid, cells, kw)

    refused(BAD_ARG, 0, [(0, 0)] * 6)
    refused(BAD_ARG, 9, good)
    refused(BAD_ARG, 3, good[:4] + [(3, 0)] + good[5:])  # a cell equal to the grid
    refused(BAD_ARG, 3, good[:5] + [(0, 3)])
    refused(BAD_ARG, 1, [(0, 0)] * 5 + [(1, 0)])
    refused(BAD_ARG, 3, None)                            # NULL cells: 2 samples are not 9
    refused(BAD_ARG, 2, None, samples=3)
    ags.set_supersampling(2)
    try:
        refused(BAD_ARG, 3, good)
    finally:
        ags.set_supersampling(1)
    refused(BAD_ARG, 3, good, encode=2)                  # what the unjittered call refuses
    refused(BAD_ARG, 3, good, y0=5, y1=25)
    refused(BAD_SIZE, 3, good, pitch=4 * 40 - 4)
    st, dest = _call(ags, kifs, cams, 2, 3, good)  # and the same arguments unrefused
    assert st == 0 and not (_pixels(dest, 40)[0] == SENT).all(-1).any()
    # the virtual screen: 8 x 8200 columns are more than 65536
    wide = kifs.ScreenData(8200, 1)
    _setup(ags, wide, cam, gui, iters)
    refused(BAD_SIZE, 8, [(7, 7)] * 2, use=cams[:2])
    st, dest = _call(ags, kifs, cams[:2], 2, 7, [(6, 6)] * 2)  # 57400 columns are not
    assert st == 0 and not (_pixels(dest, 8200)[0] == SENT).all(-1).any()


def test_the_context_is_left_as_it_was(kifs):
    """A 720p Julia frame has enough tiles for the tile-cost feedback: jittered launches in between neither record costs
    nor move the sort, and the plain frames around them are the same bytes from the same kernel."""
    import torch
    screen, cam, gui, iters = AC.scene(kifs, "julia_24", 1280, 720)
    with kifs.GraphicState(0, screen_data=screen, camera_data=cam, gui_data=gui) as g:
        g.set_iters(*iters)
        frames = [g.render() for _ in range(5)]
        assert all((f == frames[0]).all() for f in frames)
        kernel = g.debug_last_kernel()
        before = g.debug_get_tile_order()
        cams = AC.blur_cameras(kifs, cam, 2, 2)
        for jitter in ((2, [(0, 1), (1, 0), (1, 1), (0, 0)]), None, (4, [(3, 3), (0, 2), (1, 0), (2, 1)])):
            out = g.render_accumulate(cams, 2, jitter=jitter)
            g.synchronize()
            assert _hooks(g) == HOOKS
            assert (g.debug_get_tile_order() == before).all()
        assert tuple(out.shape) == (2, 720, 1280, 4) and out.dtype == torch.uint8
        after = g.render()
        assert (after == frames[0]).all() and g.debug_last_kernel() == kernel != "render_accumulate_kernel"
        assert not (out[0] == out[1]).all()
