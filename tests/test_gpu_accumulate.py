"""Accumulated frames on the GPU (kifs_render_accumulate_async, kifs_accumulate_kernels.hip), bit for bit: every byte of
every output frame equals tests/accumulate_reference.py -- the unmodified oracle's linear colour of every sub-frame,
summed in np.float32 in the contract's order, divided and encoded with the oracle's encoder.  No tolerance: both sides run
the contract's operation sequence.  Frames are 74 x 45 (ten columns past a tile edge, five rows past one) unless a case
says otherwise, and every destination is pre-filled with a sentinel so that a missing or a stray store shows.  The scenes
are tests/accumulate_cases.py's; tests/test_accumulate_reference.py holds them and the model to the oracle on the CPU."""
import ctypes as C

import numpy as np
import pytest

import accumulate_cases as AC
import accumulate_reference as AR
from geometry_cases import PIPELINES, Raw

pytestmark = pytest.mark.gpu

W, H = AC.W, AC.H
BAD_ARG, BAD_SIZE, UNCONFIGURED = 7, 3, 4
SENT = 0xA5
ACCUMULATE_KERNEL = 9
HOOKS = (ACCUMULATE_KERNEL, "render_accumulate_kernel", 0, -1, -1)


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


def _call(g, kifs, cams, samples, options=None, count=None, y0=0, y1=None, encode=1, pitch=None, sync=True, dest=None,
          null_cameras=False, null_outs=False):
    """The raw entry point on sentinel-filled destinations: (status, (count, rows, pitch) uint8 device tensor)."""
    import torch
    from kifs_raymarching_amd._lib import OptionsUniform, lib
    w, h = g.screen_data.width, g.screen_data.height
    y1 = h if y1 is None else y1
    rows = y1 - y0
    pitch = 4 * w if pitch is None else pitch
    count = len(cams) // max(samples, 1) if count is None else count
    n_dest = min(max(count, 1), 513)
    if dest is None:
        dest = torch.full((n_dest, max(rows, 1), pitch), SENT, dtype=torch.uint8, device="cuda:0")
        torch.cuda.synchronize()
    ptrs = (C.c_void_p * n_dest)(*[dest[i].data_ptr() for i in range(n_dest)])
    arr = None if options is None else (OptionsUniform * len(options))(*options)
    cam_arr = None if null_cameras else kifs.camera_array(cams)
    st = lib.kifs_render_accumulate_async(g._ctx, None, count, samples, cam_arr, arr, None if null_outs else ptrs, pitch, y0, y1, encode)
    if sync:
        assert lib.kifs_synchronize(g._ctx) == 0
    return st, dest


def _pixels(dest, w):
    """(count, rows, pitch) bytes -> ((count, rows, W, 4) pixels, (count, rows, pitch - 4 W) padding), on the host."""
    host = dest.cpu().numpy()
    return host[:, :, :4 * w].reshape(host.shape[0], host.shape[1], w, 4), host[:, :, 4 * w:]


def _hooks(g):
    from kifs_raymarching_amd._lib import lib
    return (lib.kifs_debug_last_kernel(g._ctx), g.debug_last_kernel(), g.debug_last_round_steps(), g.debug_last_group_tiles(),
            g.debug_last_bunny_form())


_LINEAR = {}  # the oracle's linear sub-frames, computed once per scene and shared by the encodes and tests that use it


def _linear(key, oracle, kifs, screen, cams, options, iters, ext=None):
    if key not in _LINEAR:
        _LINEAR[key] = AR.linear_views(oracle, kifs, screen, cams, options, iters, ext)
    return _LINEAR[key]


def _want(key, oracle, kifs, screen, cams, options, iters, samples, encode, ext=None, y0=0, y1=None):
    lin = _linear(key, oracle, kifs, screen, cams, options, iters, ext)
    return AR.accumulate_frames(oracle, kifs, screen, cams, options, iters, samples, encode, lin=lin, y0=y0, y1=y1)


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
    st, dest = _call(ags, kifs, cams, 3, encode=encode)  # options NULL: the context's
    assert st == 0 and _hooks(ags) == HOOKS
    frames, _ = _pixels(dest, W)
    want = _want(("pipeline", name), oracle, kifs, screen, cams, gui, iters, 3, encode)
    _same(frames, want, name)
    lin = _LINEAR[("pipeline", name)]
    if name != "unknown_id":  # (an unknown primitive's estimate is the constant 1: every ray of every sub-frame misses)
        assert (lin[0] != lin[1]).any() and (lin[1] != lin[2]).any() and (want[0] != want[1]).any()  # the sub-frames differ


@pytest.mark.parametrize("name", ["julia_24", "genjulia", "sphere"])
def test_per_sub_frame_options(name, ags, kifs, oracle):
    """constant, power and both colours differ per sub-frame; whole tiles miss in every sub-frame, with differing
    backgrounds; sub-frame 1 of each frame is turned away and misses everywhere while the others hit.  The context holds
    ANOTHER pipeline's options while the call is made: they are not read."""
    screen, cam, gui, iters = AC.scene(kifs, name)
    other = kifs.GuiData(primitive_shape=kifs.PrimitiveShape.Torus) if name != "sphere" else kifs.GuiData(fractal_group=kifs.FractalGroup.JuliaSet)
    _setup(ags, screen, cam, other, iters)
    options, cams = AC.varied(kifs, gui, cam, 2, 3)
    lin = _linear(("varied", name), oracle, kifs, screen, cams, options, iters)
    bg = [np.array(list(o.background_color), dtype=np.float32) for o in options]
    assert (lin[1] == bg[1]).all() and (lin[0] != bg[0]).any() and (lin[2] != bg[2]).any()
    assert all((lin[v][:8, :32] == bg[v]).all() for v in range(6)) and len({tuple(b) for b in bg[:3]}) == 3  # a whole tile of misses
    for encode in (1, 0):
        st, dest = _call(ags, kifs, cams, 3, options=options, encode=encode)
        assert st == 0 and _hooks(ags) == HOOKS
        _same(_pixels(dest, W)[0], _want(("varied", name), oracle, kifs, screen, cams, options, iters, 3, encode), (name, encode))


def test_one_sample_is_the_plain_batch(ags, kifs, oracle):
    import torch
    screen, cam, gui, iters = AC.scene(kifs, "julia_24")
    _setup(ags, screen, cam, gui, iters)
    cams = AC.blur_cameras(kifs, cam, 3, 1)
    for encode in (1, 0):
        st, dest = _call(ags, kifs, cams, 1, encode=encode)
        assert st == 0
        frames, _ = _pixels(dest, W)
        plain = torch.full((3, H, W, 4), SENT, dtype=torch.uint8, device="cuda:0")
        ags.render_batch_async([plain[i] for i in range(3)], cams, encode=encode)
        ags.synchronize()
        _same(frames, plain.cpu().numpy(), ("plain batch", encode))
        _same(frames, _want(("single", 0), oracle, kifs, screen, cams, gui, iters, 1, encode), ("model", encode))


def test_identical_cameras_are_the_models_frame(ags, kifs, oracle):
    """Three equal sub-frames: (c + c + c) / 3 in f32 -- the model's frame, whatever that is to the plain one."""
    screen, cam, gui, iters = AC.scene(kifs, "sierpinski")
    _setup(ags, screen, cam, gui, iters)
    cams = [cam] * 3
    for encode in (1, 0):
        st, dest = _call(ags, kifs, cams, 3, encode=encode)
        assert st == 0
        _same(_pixels(dest, W)[0], _want(("identical", 0), oracle, kifs, screen, cams, gui, iters, 3, encode), encode)


def test_65_views_go_through_the_view_table(ags, kifs, oracle):
    screen, cam, gui, iters = AC.scene(kifs, "julia_24")
    _setup(ags, screen, cam, kifs.GuiData(), iters)
    options, cams = AC.varied(kifs, gui, cam, 13, 5, seed=1)
    for v, c in enumerate(cams):  # nearer than `varied` puts them: most of the frame hits
        if v % 5 != 1:
            cams[v] = kifs.CameraData(origin_distance=3.0 + 0.01 * v, phi=0.3 + 0.02 * v, theta=0.2).into_buffer_data()
    st, dest = _call(ags, kifs, cams, 5, options=options)
    assert st == 0 and _hooks(ags) == HOOKS
    frames, _ = _pixels(dest, W)
    want = _want(("views65", 0), oracle, kifs, screen, cams, options, iters, 5, 1)
    _same(frames, want, "13 x 5")
    assert (want[0] != want[12]).any()


def test_512_views_of_64_samples(ags, kifs, oracle):
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
    st, dest = _call(ags, kifs, cams, 64, options=options)
    assert st == 0 and _hooks(ags) == HOOKS
    frames, _ = _pixels(dest, 40)
    assert frames.shape == (8, 13, 40, 4)
    want = _want(("views512", 0), oracle, kifs, screen, cams, options, iters, 64, 1)
    _same(frames, want, "8 x 64")
    assert (want[0] != want[7]).any()


def test_band_and_padded_pitch(ags, kifs, oracle):
    """Rows [3, 38) -- neither end a multiple of 8 -- into rows wider than 4 W: rows 3..37 of the whole frame, the guard
    bytes beyond 4 W untouched."""
    screen, cam, gui, iters = AC.scene(kifs, "julia_24")
    _setup(ags, screen, cam, gui, iters)
    cams = AC.blur_cameras(kifs, cam, 2, 3)
    st, whole = _call(ags, kifs, cams, 3)
    assert st == 0
    st, dest = _call(ags, kifs, cams, 3, y0=3, y1=38, pitch=4 * W + 32)
    assert st == 0
    frames, padding = _pixels(dest, W)
    assert frames.shape == (2, 35, W, 4) and padding.shape[-1] == 32 and (padding == SENT).all()
    _same(frames, _pixels(whole, W)[0][:, 3:38], "band against the whole frame")
    _same(frames, _want(("pipeline", "julia_24"), oracle, kifs, screen, cams, gui, iters, 3, 1, y0=3, y1=38), "band against the model")
    st, dest = _call(ags, kifs, cams, 3, y0=20, y1=20)  # an empty band: nothing to do, nothing written
    assert st == 0 and (dest.cpu().numpy() == SENT).all()


def test_heatmap_sub_frames(ags, kifs, oracle):
    screen, cam, gui, iters = AC.scene(kifs, "julia_24")
    heat = kifs.GuiData(**{**gui.__dict__, "is_heatmap": True, "fractal_color": (255, 128, 30)})
    _setup(ags, screen, cam, heat, iters)
    cams = AC.blur_cameras(kifs, cam, 2, 3)
    st, dest = _call(ags, kifs, cams, 3)
    assert st == 0
    want = _want(("heatmap", 0), oracle, kifs, screen, cams, heat, iters, 3, 1)
    _same(_pixels(dest, W)[0], want, "heatmap")
    assert (want != _want(("pipeline", "julia_24"), oracle, kifs, screen, cams, gui, iters, 3, 1)).any()


def test_soft_shadow_sub_frames(ags, kifs, oracle):
    screen, cam, gui, iters = AC.scene(kifs, "sierpinski")
    _setup(ags, screen, cam, gui, iters)
    cams = AC.blur_cameras(kifs, cam, 2, 3)
    ags.set_extensions(soft_shadow=True, shadow_steps=64, shadow_k=8.0, shadow_t0=0.02, shadow_max_t=10.0)
    try:
        st, dest = _call(ags, kifs, cams, 3)
    finally:
        ags.set_extensions(soft_shadow=False)
    assert st == 0
    want = _want(("shadow", 0), oracle, kifs, screen, cams, gui, iters, 3, 1, ext=oracle.Ext(1, 64, 8.0, 0.02, 10.0))
    _same(_pixels(dest, W)[0], want, "soft shadows")
    assert (want != _want(("pipeline", "sierpinski"), oracle, kifs, screen, cams, gui, iters, 3, 1)).any()  # the extension was on


def test_six_calls_back_to_back_and_an_explicit_stream(ags, kifs, oracle):
    """Two calls more than the scene-table ring is deep without a wait between them: a table is rewritten only after the
    launch that read it.  Then the wrapper on a stream of the caller's."""
    import torch
    screen, cam, gui, iters = AC.scene(kifs, "julia_24")
    _setup(ags, screen, cam, kifs.GuiData(), iters)
    calls = []
    for c in range(6):
        options, cams = AC.varied(kifs, gui, cam, 1, 3, seed=7 * c)
        for v in (0, 2):
            cams[v] = kifs.CameraData(origin_distance=3.0 + 0.1 * c, phi=0.3 + 0.1 * v, theta=0.1 * c).into_buffer_data()
        calls.append((options, cams, torch.full((1, H, 4 * W), SENT, dtype=torch.uint8, device="cuda:0")))
    torch.cuda.synchronize()
    for options, cams, dest in calls:
        st, _ = _call(ags, kifs, cams, 3, options=options, sync=False, dest=dest)
        assert st == 0
    ags.synchronize()
    wants = [_want(("ring", c), oracle, kifs, screen, cams, options, iters, 3, 1) for c, (options, cams, _) in enumerate(calls)]
    for c, (_, _, dest) in enumerate(calls):
        _same(_pixels(dest, W)[0], wants[c], ("call", c))
    assert (wants[0] != wants[5]).any()
    stream = torch.cuda.Stream(device=0)
    options, cams, _ = calls[2]
    out = ags.render_accumulate(cams, 3, options=options, stream=stream)
    stream.synchronize()
    assert tuple(out.shape) == (1, H, W, 4) and out.dtype == torch.uint8
    _same(out.cpu().numpy(), wants[2], "explicit stream")


def test_refusals_write_nothing(ags, kifs):
    screen, cam, gui, iters = AC.scene(kifs, "sierpinski", 40, 24)
    _setup(ags, screen, cam, gui, iters)
    cams = AC.blur_cameras(kifs, cam, 3, 2)
    options = [AC.image(kifs, gui) for _ in range(6)]

    def refused(want, samples=2, opts=options, use=cams, **kw):
        st, dest = _call(ags, kifs, use, samples, options=opts, **kw)
        assert st == want, (st, samples, kw)
        assert (dest.cpu().numpy() == SENT).all(), (samples, kw)

    refused(BAD_ARG, null_cameras=True)
    refused(BAD_ARG, null_outs=True)
    refused(BAD_ARG, samples=0, count=3)
    refused(BAD_ARG, samples=65, count=1, use=cams * 11, opts=None)
    refused(BAD_ARG, samples=1, count=513, use=cams * 86, opts=None)   # count * samples = 513
    refused(BAD_ARG, samples=57, count=9, use=cams * 86, opts=None)    # 513 again
    refused(BAD_ARG, count=0)
    ags.set_supersampling(2)
    try:
        refused(BAD_ARG)
    finally:
        ags.set_supersampling(1)
    for field, value in (("max_iterations", 255), ("max_distance", 999.0), ("is_heatmap", 1), ("fractal_group_id", 1), ("primitive_id", 3)):
        opts = [AC.image(kifs, gui) for _ in range(6)]
        setattr(opts[4], field, value)  # a forbidden field varies at view 4
        refused(BAD_ARG, opts=opts)
    ulp = [AC.image(kifs, gui) for _ in range(6)]
    ulp[4].epsilon = np.nextafter(np.float32(ulp[4].epsilon), np.float32(1.0))
    refused(BAD_ARG, opts=ulp)
    refused(BAD_ARG, encode=2)
    refused(BAD_ARG, y0=5, y1=25)
    refused(BAD_ARG, y0=-1, y1=8)
    refused(BAD_SIZE, pitch=4 * 40 - 4)
    refused(BAD_SIZE, pitch=4 * 40 + 2)
    # no screen; and no options of its own with options NULL
    from kifs_raymarching_amd._lib import lib
    st = C.c_int(-1)
    ctx = lib.kifs_create(0, C.byref(st))
    assert ctx and st.value == 0

    class Bare:  # what _call needs of a GraphicState
        _ctx = ctx
        screen_data = screen

    try:
        s, dest = _call(Bare, kifs, cams, 2, options=options)
        assert s == UNCONFIGURED and (dest.cpu().numpy() == SENT).all()
        u = screen.into_buffer_data()
        assert lib.kifs_set_screen(ctx, C.byref(u)) == 0
        s, dest = _call(Bare, kifs, cams, 2, options=None)
        assert s == UNCONFIGURED and (dest.cpu().numpy() == SENT).all()
        s, bare = _call(Bare, kifs, cams, 2, options=options)  # given its options, the bare context renders
        assert s == 0
    finally:
        lib.kifs_destroy(ctx)
    # and the same arguments unrefused
    st, dest = _call(ags, kifs, cams, 2, options=options)
    assert st == 0 and not (_pixels(dest, 40)[0] == SENT).all(-1).any()  # (alpha is 255: no pixel is the sentinel's)
    assert (dest.cpu().numpy() == bare.cpu().numpy()).all()


def test_the_context_is_left_as_it_was(kifs):
    """A 720p Julia frame has enough tiles for the tile-cost feedback: accumulated launches in between neither record
    costs nor move the sort, the context's options stay its own, and the plain frames around them are the same bytes from
    the same kernel."""
    import torch
    screen, cam, gui, iters = AC.scene(kifs, "julia_24", 1280, 720)
    with kifs.GraphicState(0, screen_data=screen, camera_data=cam, gui_data=gui) as g:
        g.set_iters(*iters)
        frames = [g.render() for _ in range(5)]
        assert all((f == frames[0]).all() for f in frames)
        kernel = g.debug_last_kernel()
        before = g.debug_get_tile_order()
        cams = AC.blur_cameras(kifs, cam, 2, 2)
        other = [AC.image(kifs, kifs.GuiData(**{**gui.__dict__, "background_color": (40 * v, 0, 40)})) for v in range(4)]
        for options in (None, other, None):
            out = g.render_accumulate(cams, 2, options=options)
            g.synchronize()
            assert _hooks(g) == HOOKS
            assert (g.debug_get_tile_order() == before).all()
        assert tuple(out.shape) == (2, 720, 1280, 4) and out.dtype == torch.uint8
        after = g.render()
        assert (after == frames[0]).all() and g.debug_last_kernel() == kernel != "render_accumulate_kernel"
        assert not (out[0] == out[1]).all()
