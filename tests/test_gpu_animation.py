"""Animated batches on the GPU (kifs_render_animation_async, kifs_animation_kernels.hip), bit for bit: every frame of a
launch whose frames differ in constant, power, colours and camera equals the context's own render after
kifs_set_camera / kifs_set_options with that frame's values, and the oracle's frame for them -- for every pipeline and
both encodes.  No tolerance: both sides run the contract's operation sequence.  Frames are 230 x 147 (width no multiple of
32, height no multiple of 8) unless a case says otherwise, and every destination is pre-filled with a sentinel so that a
missing or a stray store shows.  The seeded scenes of tests/extension_fuzz_cases.py run launches of 2, 5 and 9 small
frames whose cameras mix positions inside, on and outside the bounding sphere and whose constants include exact and negative
zeros."""
import ctypes as C

import numpy as np
import pytest

import extension_fuzz_cases as X
import extension_fuzz_support as S
from geometry_cases import PIPELINES, Raw, cases
from helpers import oracle_frame

pytestmark = pytest.mark.gpu

W, H = 230, 147
BAD_ARG, BAD_SIZE, UNCONFIGURED = 7, 3, 4
SENT = 0xA5
ANIMATION_KERNEL = 8


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


def _image(kifs, gui):
    """A fresh 80-byte options image of `gui` (GuiData, Raw or an image)."""
    from kifs_raymarching_amd._lib import OptionsUniform
    src = gui.into_buffer_data() if hasattr(gui, "into_buffer_data") else gui
    return OptionsUniform.from_buffer_copy(kifs.uniform_bytes(src))


def _variants(kifs, gui, n, seed=0):
    """`n` option images of `gui`'s pipeline that differ in constant, power and both colours (frame 0 is `gui` itself)."""
    out = [_image(kifs, gui)]
    for i in range(1, n):
        u = _image(kifs, gui)
        k = i + seed
        u.constant[0] += np.float32(0.07 * k)
        u.constant[1] -= np.float32(0.05 * k)
        u.constant[2] += np.float32(0.03 * k)
        u.constant[3] -= np.float32(0.04 * k)
        u.power = np.float32(u.power + 0.75 * k)
        for ch in range(3):
            u.fractal_color[ch] = np.float32(0.15 + 0.2 * ((k + ch) % 4))
            u.background_color[ch] = np.float32(0.02 + 0.11 * ((k + 2 * ch) % 5))
        u._padding1, u._padding2, u._padding3 = 0xdead0000 + i, 17 * i, 0xffffffff  # ignored by the contract
        out.append(u)
    return out


def _cameras(kifs, cam, n):
    return [kifs.CameraData(origin_distance=cam.origin_distance + 0.21 * i, phi=cam.phi + 0.4 * i, theta=cam.theta - 0.13 * i)
            for i in range(n)]


def _call(g, kifs, options, cams=None, count=None, y0=0, y1=None, encode=1, pitch=None, null_options=False, sync=True, dest=None):
    """The raw entry point on sentinel-filled destinations: (status, (count, rows, pitch) uint8 device tensor)."""
    import torch
    from kifs_raymarching_amd._lib import OptionsUniform, lib
    w, h = g.screen_data.width, g.screen_data.height
    y1 = h if y1 is None else y1
    rows = y1 - y0
    pitch = 4 * w if pitch is None else pitch
    count = len(options) if count is None else count
    n_dest = max(count, 1)
    if dest is None:
        dest = torch.full((n_dest, max(rows, 1), pitch), SENT, dtype=torch.uint8, device="cuda:0")
        torch.cuda.synchronize()
    ptrs = (C.c_void_p * n_dest)(*[dest[i].data_ptr() for i in range(n_dest)])
    arr = None if null_options else (OptionsUniform * max(len(options), 1))(*options)
    cam_arr = None if cams is None else kifs.camera_array(cams)
    st = lib.kifs_render_animation_async(g._ctx, None, count, cam_arr, arr, ptrs, pitch, y0, y1, encode)
    if sync:
        assert lib.kifs_synchronize(g._ctx) == 0
    return st, dest


def _pixels(dest, w):
    """(count, rows, pitch) bytes -> ((count, rows, W, 4) pixels, (count, rows, pitch - 4 W) padding), on the host."""
    host = dest.cpu().numpy()
    return host[:, :, :4 * w].reshape(host.shape[0], host.shape[1], w, 4), host[:, :, 4 * w:]


def _lone(g, cam, image, encode=1, y0=0, y1=None):
    """The contract's right-hand side: the context's own render after set_camera and set_options."""
    if cam is not None:
        g.set_camera(cam)
    g.update_options(image)
    return g.render(y0=y0, y1=y1, encode=encode)


def _hooks(g):
    from kifs_raymarching_amd._lib import lib
    return (lib.kifs_debug_last_kernel(g._ctx), g.debug_last_kernel(), g.debug_last_round_steps(), g.debug_last_group_tiles(),
            g.debug_last_bunny_form())


_ORACLE = {}


def _oracle(oracle, kifs, name, i, screen, cam, image, iters, encode):
    key = (name, i, encode)
    if key not in _ORACLE:
        _ORACLE[key] = oracle_frame(oracle, kifs, screen, cam, Raw(image), iters, encode=encode)
    return _ORACLE[key]


@pytest.mark.parametrize("name", PIPELINES)
@pytest.mark.parametrize("encode", [1, 0])
def test_every_pipeline_bit_exact(name, encode, ags, kifs, oracle):
    screen, cam, gui, iters = cases(kifs, W, H)[name]
    # the context holds ANOTHER pipeline's options while the call is made: they are not read
    other = kifs.GuiData(primitive_shape=kifs.PrimitiveShape.Torus) if name != "torus" else kifs.GuiData()
    _setup(ags, screen, cam, other, iters)
    options, cams = _variants(kifs, gui, 4), _cameras(kifs, cam, 4)
    st, dest = _call(ags, kifs, options, cams=cams, encode=encode)
    assert st == 0
    assert _hooks(ags) == (ANIMATION_KERNEL, "render_animation_kernel", 0, -1, -1)
    frames, _ = _pixels(dest, W)
    wants = [_oracle(oracle, kifs, name, i, screen, cams[i], options[i], iters, encode) for i in range(4)]
    for i in range(4):
        assert (frames[i] == _lone(ags, cams[i], options[i], encode=encode)).all(), (name, i)
        assert (frames[i] == wants[i]).all(), (name, i)
    if name.startswith("julia"):
        # not vacuous: some pixel is a hit in two frames (neither's background) and differs between them
        bg = [wants[i][0, 0] for i in (0, 1)]
        hit = (wants[0] != bg[0]).any(-1) & (wants[1] != bg[1]).any(-1)
        assert (wants[0][0, 0] == wants[0][-1, -1]).all() and hit.any()
        assert ((wants[0] != wants[1]).any(-1) & hit).any()
        # and the constant alone moves hit pixels: frames 0 and 1 again with frame 0's colours, power and camera
        moved = _image(kifs, options[0])
        for k in range(4):
            moved.constant[k] = options[1].constant[k]
        st, dest = _call(ags, kifs, [options[0], moved], cams=[cams[0], cams[0]], encode=encode)
        two, _ = _pixels(dest, W)
        assert st == 0 and (two[0] == wants[0]).all()
        assert (two[1] == _lone(ags, cams[0], moved, encode=encode)).all()
        both = (two[0] != bg[0]).any(-1) & (two[1] != bg[0]).any(-1)
        assert ((two[0] != two[1]).any(-1) & both).any()


def test_per_frame_background_through_culled_tiles(ags, kifs):
    """A far camera: nearly every tile leaves at the culls and stores its OWN view's encoded background."""
    screen, _, gui, iters = cases(kifs, W, H)["julia_24"]
    cam = kifs.CameraData(origin_distance=400.0, phi=0.3)
    _setup(ags, screen, cam, gui, iters)
    options = []
    for rgb in ((0.9, 0.1, 0.2), (0.05, 0.6, 0.3), (0.3, 0.3, 0.95)):
        u = _image(kifs, gui)
        for ch in range(3):
            u.background_color[ch] = np.float32(rgb[ch])
        options.append(u)
    for encode in (1, 0):
        st, dest = _call(ags, kifs, options, cams=[cam] * 3, encode=encode)
        assert st == 0
        frames, _ = _pixels(dest, W)
        for i in range(3):
            assert (frames[i] == _lone(ags, cam, options[i], encode=encode)).all(), i
            assert ((frames[i] == frames[i][0, 0]).all(-1)).mean() > 0.99  # background almost everywhere
        corners = {tuple(frames[i][0, 0]) for i in range(3)} | {tuple(frames[i][-1, -1]) for i in range(3)}
        assert len(corners) == 3 and all(tuple(frames[i][0, 0]) == tuple(frames[i][-1, -1]) for i in range(3))


def test_one_frame_and_the_context_camera(ags, kifs):
    screen, cam, gui, iters = cases(kifs, W, H)["julia_24"]
    _setup(ags, screen, cam, kifs.GuiData(), iters)
    options = _variants(kifs, gui, 3, seed=2)
    st, dest = _call(ags, kifs, options[1:2], cams=[cam])  # count = 1
    assert st == 0
    assert (_pixels(dest, W)[0][0] == _lone(ags, cam, options[1])).all()
    mine = kifs.CameraData(origin_distance=3.3, phi=1.1, theta=0.2)
    ags.set_camera(mine)
    ags.update_options(kifs.GuiData())
    st, dest = _call(ags, kifs, options, cams=None)  # cameras NULL, count = 3: the context's camera for every frame
    assert st == 0
    frames, _ = _pixels(dest, W)
    for i in range(3):
        assert (frames[i] == _lone(ags, mine, options[i])).all(), i
    st, dest = _call(ags, kifs, options[:1], cams=None)  # and for one
    assert st == 0 and (_pixels(dest, W)[0][0] == _lone(ags, mine, options[0])).all()


@pytest.mark.parametrize("name", ["julia_24", "torus"])
def test_band_and_padded_pitch(name, ags, kifs):
    """A band with neither end a multiple of 8 into rows wider than 4 W: the rows of the full frame, padding untouched."""
    screen, cam, gui, iters = cases(kifs, W, H)[name]
    _setup(ags, screen, cam, kifs.GuiData(), iters)
    options, cams = _variants(kifs, gui, 3, seed=1), _cameras(kifs, cam, 3)
    y0, y1 = 13, 101
    st, dest = _call(ags, kifs, options, cams=cams, y0=y0, y1=y1, pitch=4 * W + 32)
    assert st == 0
    frames, padding = _pixels(dest, W)
    assert padding.shape[-1] == 32 and (padding == SENT).all()
    for i in range(3):
        assert (frames[i] == _lone(ags, cams[i], options[i])[y0:y1]).all(), i
        assert (frames[i] == _lone(ags, cams[i], options[i], y0=y0, y1=y1)).all(), i
    st, dest = _call(ags, kifs, options, cams=cams, y0=60, y1=60)  # an empty band: nothing to do, nothing written
    assert st == 0 and (dest.cpu().numpy() == SENT).all()


@pytest.mark.parametrize("count", [70, 512])
def test_more_views_than_the_kernel_argument_holds(count, ags, kifs):
    """Beyond MAX_BATCH_INLINE = 64 views the cameras and destinations go through the view-table ring; the scenes always
    go through theirs."""
    screen, cam, gui, iters = cases(kifs, 40, 24)["julia_24"]
    _setup(ags, screen, cam, kifs.GuiData(), iters)
    options = []
    for i in range(count):
        u = _image(kifs, gui)
        u.constant[0] = np.float32(-0.2 + 0.001 * i)
        u.constant[2] = np.float32(0.2 - 0.0007 * i)
        u.fractal_color[1] = np.float32(0.2 + 0.0015 * i)
        u.background_color[2] = np.float32(0.001 * i)
        options.append(u)
    cams = [kifs.CameraData(origin_distance=3.0 + 0.002 * i, phi=0.3 + 0.011 * i, theta=0.1 * np.sin(i)) for i in range(count)]
    st, dest = _call(ags, kifs, options, cams=cams)
    assert st == 0
    frames, _ = _pixels(dest, 40)
    assert frames.shape == (count, 24, 40, 4) and not (frames == SENT).all(-1).any()
    for i in (0, 63, 64, count - 1):
        assert (frames[i] == _lone(ags, cams[i], options[i])).all(), i
    assert not (frames[0] == frames[count - 1]).all()


def test_ring_reuse_without_synchronisation(ags, kifs):
    """Two calls more than the scene-table ring is deep, back to back on one stream: a table is rewritten only after the
    launch that read it."""
    import torch
    from kifs_raymarching_amd.graphics import ANIMATION_RING
    screen, cam, gui, iters = cases(kifs, W, H)["julia_24"]
    _setup(ags, screen, cam, kifs.GuiData(), iters)
    calls = ANIMATION_RING + 2
    cams = _cameras(kifs, cam, 3)
    options = [_variants(kifs, gui, 3, seed=5 * c) for c in range(calls)]
    for c in range(calls):  # (frame 0 of every call differs too)
        options[c][0].constant[1] = np.float32(0.6 - 0.02 * c)
    dests = [torch.full((3, H, 4 * W), SENT, dtype=torch.uint8, device="cuda:0") for _ in range(calls)]
    torch.cuda.synchronize()
    for c in range(calls):
        st, _ = _call(ags, kifs, options[c], cams=cams, sync=False, dest=dests[c])
        assert st == 0
    ags.synchronize()
    for c in range(calls):
        frames, _ = _pixels(dests[c], W)
        for i in range(3):
            assert (frames[i] == _lone(ags, cams[i], options[c][i])).all(), (c, i)
    assert not (_pixels(dests[0], W)[0][0] == _pixels(dests[calls - 1], W)[0][0]).all()


def test_heatmap_sequence(ags, kifs, oracle):
    screen, cam, gui, iters = cases(kifs, W, H)["julia_24"]
    heat = kifs.GuiData(**{**gui.__dict__, "is_heatmap": True, "fractal_color": (255, 128, 30)})
    _setup(ags, screen, cam, kifs.GuiData(), iters)
    options, cams = _variants(kifs, heat, 3, seed=3), _cameras(kifs, cam, 3)
    st, dest = _call(ags, kifs, options, cams=cams)
    assert st == 0
    frames, _ = _pixels(dest, W)
    for i in range(3):
        assert (frames[i] == _lone(ags, cams[i], options[i])).all(), i
    assert (frames[1] == oracle_frame(oracle, kifs, screen, cams[1], Raw(options[1]), iters)).all()
    assert not (frames[0] == frames[1]).all()


def test_soft_shadow_sequence(ags, kifs, oracle):
    screen, cam, gui, iters = cases(kifs, W, H)["sierpinski"]
    _setup(ags, screen, cam, kifs.GuiData(), iters)
    options, cams = _variants(kifs, gui, 3, seed=4), _cameras(kifs, cam, 3)
    ags.set_extensions(soft_shadow=True, shadow_steps=64, shadow_k=8.0, shadow_t0=0.02, shadow_max_t=10.0)
    try:
        st, dest = _call(ags, kifs, options, cams=cams)
        assert st == 0
        frames, _ = _pixels(dest, W)
        shadowed = [_lone(ags, cams[i], options[i]) for i in range(3)]
    finally:
        ags.set_extensions(soft_shadow=False)
    for i in range(3):
        assert (frames[i] == shadowed[i]).all(), i
    assert not (shadowed[0] == _lone(ags, cams[0], options[0])).all()  # the extension was on
    s, c, o = (oracle.from_bytes(t, kifs.uniform_bytes(u)) for t, u in
               ((oracle.Screen, screen.into_buffer_data()), (oracle.Camera, cams[2].into_buffer_data()), (oracle.Options, options[2])))
    assert (frames[2] == oracle.render(s, c, o, oracle.iters(*iters), ext=oracle.Ext(1, 64, 8.0, 0.02, 10.0))).all()


def test_refusals_write_nothing(ags, kifs):
    screen, cam, gui, iters = cases(kifs, 40, 24)["sierpinski"]
    _setup(ags, screen, cam, gui, iters)
    options, cams = _variants(kifs, gui, 3), _cameras(kifs, cam, 3)

    def refused(want, opts, **kw):
        kw.setdefault("cams", cams[:len(opts)] if len(opts) <= 3 else None)
        st, dest = _call(ags, kifs, opts, **kw)
        assert st == want, (st, kw)
        assert (dest.cpu().numpy() == SENT).all(), kw

    ulp = _image(kifs, options[1])
    ulp.epsilon = np.nextafter(np.float32(ulp.epsilon), np.float32(1.0))
    assert ulp.epsilon != options[1].epsilon
    refused(BAD_ARG, [options[0], ulp, options[2]])
    prim = _image(kifs, options[2])
    prim.primitive_id = 3
    refused(BAD_ARG, [options[0], options[1], prim])
    for field, value in (("max_iterations", 255), ("max_distance", 999.0), ("is_heatmap", 1), ("fractal_group_id", 1)):
        u = _image(kifs, options[1])
        setattr(u, field, value)
        refused(BAD_ARG, [options[0], u])
    bad_group = _image(kifs, options[0])
    bad_group.fractal_group_id = 3
    refused(BAD_ARG, [bad_group])
    refused(BAD_ARG, options[:1], count=0)
    refused(BAD_ARG, [options[0]] * 513, cams=None)
    ags.set_supersampling(2)
    try:
        refused(BAD_ARG, options)
    finally:
        ags.set_supersampling(1)
    refused(BAD_ARG, options, null_options=True)
    refused(BAD_ARG, options, encode=2)
    refused(BAD_ARG, options, y0=5, y1=25)
    refused(BAD_ARG, options, y0=-1, y1=8)
    refused(BAD_SIZE, options, pitch=4 * 40 - 4)
    # and the same arguments unrefused
    st, dest = _call(ags, kifs, options, cams=cams)
    assert st == 0 and not (_pixels(dest, 40)[0] == SENT).all(-1).any()  # (alpha is 255: no pixel is the sentinel's)


def test_the_context_is_left_as_it_was(kifs):
    """A 720p Julia frame has enough tiles for the tile-cost feedback: animated launches in between neither record costs
    nor move the sort, the context's options stay its own, and the plain frames around them are the same bytes from the
    same kernel."""
    import torch
    screen, cam, gui, iters = cases(kifs, 1280, 720)["julia_24"]
    morph = [_image(kifs, kifs.GuiData(**{**gui.__dict__, "constant": (-0.2 + 0.1 * i, 0.6, 0.2 - 0.1 * i, 0.2),
                                          "background_color": (40 * i, 0, 40)})) for i in range(3)]
    with kifs.GraphicState(0, screen_data=screen, camera_data=cam, gui_data=gui) as g:
        g.set_iters(*iters)
        frames = [g.render() for _ in range(5)]
        assert all((f == frames[0]).all() for f in frames)
        kernel = g.debug_last_kernel()
        before = g.debug_get_tile_order()
        for _ in range(3):
            out = g.render_animation(morph[1:])
            g.synchronize()
            assert _hooks(g) == (ANIMATION_KERNEL, "render_animation_kernel", 0, -1, -1)
            assert (g.debug_get_tile_order() == before).all()
        assert tuple(out.shape) == (2, 720, 1280, 4) and out.dtype == torch.uint8
        after = g.render()
        assert (after == frames[0]).all() and g.debug_last_kernel() == kernel != "render_animation_kernel"
        got = out.cpu().numpy()
        for i in (1, 2):
            g.update_options(morph[i])
            assert (got[i - 1] == g.render()).all(), i
        assert not (got[0] == got[1]).all()


def test_a_context_without_options_or_camera(ags, kifs):
    """The context's options need not have been set, its camera only when cameras is NULL; the screen must be."""
    from kifs_raymarching_amd._lib import lib
    screen, cam, gui, iters = cases(kifs, 40, 24)["torus"]
    options, cams = _variants(kifs, gui, 2), _cameras(kifs, cam, 2)
    _setup(ags, screen, cam, gui, iters)
    want = [_lone(ags, cams[i], options[i]) for i in range(2)]
    st = C.c_int(-1)
    ctx = lib.kifs_create(0, C.byref(st))
    assert ctx and st.value == 0

    class Bare:  # what _call needs of a GraphicState
        _ctx = ctx
        screen_data = screen

    try:
        s, dest = _call(Bare, kifs, options, cams=cams)
        assert s == UNCONFIGURED and (dest.cpu().numpy() == SENT).all()  # no screen
        u = screen.into_buffer_data()
        assert lib.kifs_set_screen(ctx, C.byref(u)) == 0
        s, dest = _call(Bare, kifs, options, cams=None)
        assert s == UNCONFIGURED and (dest.cpu().numpy() == SENT).all()  # no camera of its own
        s, dest = _call(Bare, kifs, options, cams=cams)
        assert s == 0
        frames, _ = _pixels(dest, 40)
        assert (frames[0] == want[0]).all() and (frames[1] == want[1]).all()
        # its options are still unset: a plain render is still refused
        import torch
        one = torch.full((24, 160), SENT, dtype=torch.uint8, device="cuda:0")
        torch.cuda.synchronize()
        assert lib.kifs_set_camera(ctx, C.byref(cams[0].into_buffer_data())) == 0
        assert lib.kifs_render_async(ctx, None, one.data_ptr(), 160, 0, 24, 1) == UNCONFIGURED
    finally:
        lib.kifs_destroy(ctx)


@pytest.mark.parametrize("index", range(X.N))
def test_fuzz_sequence_bit_exact(index, ags, kifs, oracle):
    """A seeded scene's launch of 2, 5 or 9 frames, each with its own constant, power, colours and camera family: every
    frame is the oracle's for that frame's options, and one of them the bytes of update_options + render."""
    scene = X.scenes(kifs)[index]
    name, _, _, cam, gui, iters, encode = scene
    screen, frames, lone = X.animation(kifs, index, scene)
    w, h = screen.width, screen.height
    what = f"{S.describe(index, scene)}; {len(frames)} frames of {w} x {h}"
    shadow = S.shadow_of(oracle, kifs, index)
    cams = [c for c, _ in frames]
    options = [_image(kifs, g) for _, g in frames]
    S.setup(ags, screen, cam, gui, iters, shadow=shadow)
    try:
        st, dest = _call(ags, kifs, options, cams=cams, encode=encode, pitch=4 * w + 32)
        assert st == 0, what
        assert _hooks(ags) == (ANIMATION_KERNEL, "render_animation_kernel", 0, -1, -1), what
        alone = _lone(ags, cams[lone], options[lone], encode=encode)
    finally:
        ags.set_extensions(soft_shadow=False)
    got, padding = _pixels(dest, w)
    assert (padding == SENT).all(), f"{what}: the padding of the rows"
    for f, (c, g) in enumerate(frames):
        want = S.expected_colour(oracle, kifs, screen, c, Raw(options[f]), iters, encode, shadow)
        bad = (got[f] != want).any(-1)
        assert not bad.any(), (f"{what}; frame {f} ({c}, {X.options_of(g)}): {S.first(bad)}: got {got[f][bad][0]}, "
                               f"want {want[bad][0]}")
    bad = (got[lone] != alone).any(-1)
    assert not bad.any(), f"{what}; frame {lone} against update_options + render: {S.first(bad)}"
