"""The geometry output on the GPU (kifs_render_geometry_async, kifs_geometry_kernels.hip), bit for bit: for every
pipeline and both encodes the colour plane equals kifs_render's bytes and the oracle's, and every texel
(n.x, n.y, n.z, t) equals the CPU restatement of the contract (tests/geometry_reference.c, held to the oracle by
tests/test_geometry_reference.py).  f32 planes are compared by bit pattern, any NaN equal to any NaN; no tolerance: both
sides run the contract's operation sequence.  Frames are a few hundred pixels a side, width no multiple of 32, height no
multiple of 8, and every destination is pre-filled with a sentinel so that a missing store shows.  The seeded scenes of
tests/extension_fuzz_cases.py run the same comparison at small ragged sizes from cameras inside, on and just outside the
bounding sphere, lone and in batches that mix them."""
import ctypes as C

import numpy as np
import pytest

import extension_fuzz_cases as X
import extension_fuzz_support as S
import geometry_reference as GR
from geometry_cases import PIPELINES, Raw, cases
from helpers import oracle_frame, oracle_uniforms

pytestmark = pytest.mark.gpu

W, H = 230, 147
BAD_ARG = 7
SENT_U8 = 0xA5
SENT_F32 = np.float32(-12345.5)


@pytest.fixture(scope="module")
def ggs(kifs):
    g = kifs.GraphicState(0)
    yield g
    g.close()


def _setup(g, screen, cam, gui, iters):
    g.update_screen_data(screen)
    g.set_camera(cam)
    if isinstance(gui, Raw):
        g.set_raw_uniforms(options=gui.u)
    else:
        g.update_options(gui)
    g.set_iters(*iters)
    g.set_extensions(soft_shadow=False)
    g.set_supersampling(1)


def _call(g, kifs, cams=None, count=1, y0=0, y1=None, encode=1, gpitch=None, gstride=None, misalign=0, cpad=0):
    """The raw entry point on sentinel-filled destinations: (status, colour (count, rows, W, 4) uint8,
    geometry (count, rows, gpitch / 4) float32 -- whole rows, padding included).  `cpad`: bytes of padding after every
    colour row (and 64 after every frame's last row), asserted to hold the sentinel still."""
    import torch
    from kifs_raymarching_amd._lib import lib
    w, h = g.screen_data.width, g.screen_data.height
    y1 = h if y1 is None else y1
    rows = y1 - y0
    gpitch = 16 * w if gpitch is None else gpitch
    gstride = rows * gpitch if gstride is None else gstride
    cpitch = 4 * w + cpad
    colour = torch.full((count, rows * cpitch + (64 if cpad else 0)), SENT_U8, dtype=torch.uint8, device="cuda:0")
    floats = max(count * gstride, rows * gpitch) // 4 + 8
    plane = torch.full((floats,), float(SENT_F32), dtype=torch.float32, device="cuda:0")
    torch.cuda.synchronize()
    ptrs = (C.c_void_p * count)(*[colour[i].data_ptr() for i in range(count)])
    arr = None if cams is None else kifs.camera_array(cams)
    st = lib.kifs_render_geometry_async(g._ctx, None, count, arr, ptrs, cpitch, plane.data_ptr() + misalign, gpitch, gstride,
                                        y0, y1, encode)
    assert lib.kifs_synchronize(g._ctx) == 0
    host = plane.cpu().numpy()
    geom = None
    if st == 0:
        geom = np.stack([host[i * gstride // 4: i * gstride // 4 + rows * gpitch // 4].reshape(rows, gpitch // 4)
                         for i in range(count)])
    chost = colour.cpu().numpy()
    crows = chost[:, :rows * cpitch].reshape(count, rows, cpitch)
    assert (crows[:, :, 4 * w:] == SENT_U8).all() and (chost[:, rows * cpitch:] == SENT_U8).all(), "a colour store outside the frame"
    return st, np.ascontiguousarray(crows[:, :, :4 * w]).reshape(count, rows, w, 4), geom, host


def _texels(geom_rows, w):
    """(rows, pitch / 4) floats -> (rows, W, 4) texels."""
    return geom_rows[:, :4 * w].reshape(geom_rows.shape[0], w, 4)


_REF = {}


def _reference(oracle, kifs, name):
    if name not in _REF:
        screen, cam, gui, iters = cases(kifs, W, H)[name]
        _REF[name] = GR.geometry_frame(oracle, kifs, screen, cam, gui, iters)
    return _REF[name]


def _assert_same(got, want, what):
    same = GR.same_bits(got, want)
    if not same.all():
        at = tuple(np.argwhere(~same)[0])
        pytest.fail(f"{what}: {int((~same).sum())} of {same.size} floats differ; first at {at}: "
                    f"got {got[at]!r} ({got[at].view(np.uint32):#x}), want {want[at]!r} ({want[at].view(np.uint32):#x})")


@pytest.mark.parametrize("name", PIPELINES)
@pytest.mark.parametrize("encode", [1, 0])
def test_every_pipeline_bit_exact(name, encode, ggs, kifs, oracle):
    screen, cam, gui, iters = cases(kifs, W, H)[name]
    _setup(ggs, screen, cam, gui, iters)
    plain = ggs.render(encode=encode)
    st, colour, geom, _ = _call(ggs, kifs, encode=encode)
    assert st == 0
    assert ggs.debug_last_kernel() == "render_geometry_kernel"
    assert ggs.debug_last_round_steps() == 0 and ggs.debug_last_group_tiles() == -1 and ggs.debug_last_bunny_form() == -1
    assert (colour[0] == plain).all()
    assert (colour[0] == oracle_frame(oracle, kifs, screen, cam, gui, iters, encode=encode)).all()
    want, hit, _ = _reference(oracle, kifs, name)
    _assert_same(_texels(geom[0], W), want, name)
    if name != "unknown_id":
        assert hit.any() and not hit.all()


def test_python_methods_return_the_same_planes(ggs, kifs, oracle):
    screen, cam, gui, iters = cases(kifs, W, H)["sierpinski"]
    _setup(ggs, screen, cam, gui, iters)
    colour, geometry = ggs.render_geometry()
    assert tuple(colour.shape) == (H, W, 4) and tuple(geometry.shape) == (H, W, 4)
    assert (colour.cpu().numpy() == ggs.render()).all()
    _assert_same(geometry.cpu().numpy(), _reference(oracle, kifs, "sierpinski")[0], "render_geometry")


@pytest.mark.parametrize("name", ["julia_24", "torus"])
def test_bands_and_pitch(name, ggs, kifs, oracle):
    """A band with neither end a multiple of 8 into rows wider than 16 W: the rows of the full frame, padding untouched."""
    screen, cam, gui, iters = cases(kifs, W, H)[name]
    _setup(ggs, screen, cam, gui, iters)
    want = _reference(oracle, kifs, name)[0]
    whole = ggs.render()
    for y0, y1 in ((13, 101), (60, 61), (141, 147)):
        gpitch = 16 * W + 48
        st, colour, geom, host = _call(ggs, kifs, y0=y0, y1=y1, gpitch=gpitch)
        assert st == 0
        assert (colour[0] == whole[y0:y1]).all()
        _assert_same(_texels(geom[0], W), want[y0:y1], (name, y0, y1))
        assert (geom[0][:, 4 * W:] == SENT_F32).all()                       # the padding of every row
        assert (host[(y1 - y0) * gpitch // 4:] == SENT_F32).all()             # and nothing past the band


@pytest.mark.parametrize("count", [3, 66])
def test_batch_frames_equal_the_lone_call(count, ggs, kifs, oracle):
    """Several cameras in one launch -- 66: the views go through the device table -- each frame as the lone call."""
    screen, _, gui, iters = cases(kifs, 150, 94)["julia_24"]
    cams = [kifs.CameraData(origin_distance=3.0 + 0.01 * i, phi=0.37 * i, theta=0.2 * np.sin(i)) for i in range(count)]
    _setup(ggs, screen, cams[0], gui, iters)
    gpitch = 16 * 150
    gstride = 94 * gpitch + 32  # (more than the rows need: the gap keeps its sentinel)
    st, colour, geom, host = _call(ggs, kifs, cams=cams, count=count, gstride=gstride)
    assert st == 0
    for i in (range(count) if count < 10 else (0, 1, 31, 63, 64, 65)):
        ggs.set_camera(cams[i])
        st1, c1, g1, _ = _call(ggs, kifs)  # cameras NULL, count 1: the context's camera
        assert st1 == 0
        assert (colour[i] == c1[0]).all(), i
        _assert_same(geom[i], g1[0], ("batch frame", i))
        assert (host[(i * gstride + 94 * gpitch) // 4:((i + 1) * gstride) // 4] == SENT_F32).all()
    # the lone call with cameras NULL is the context's camera: the reference's frame for it
    ggs.set_camera(cams[1])
    _, _, g1, _ = _call(ggs, kifs)
    want = GR.geometry_frame(oracle, kifs, screen, cams[1], gui, iters)[0]
    _assert_same(_texels(g1[0], 150), want, "context camera")
    # and a one-frame batch with an explicit camera does not use the context's
    _, _, g2, _ = _call(ggs, kifs, cams=[cams[2]], count=1)
    _assert_same(g2[0], geom[2], "explicit camera")


def test_far_camera_every_texel_is_the_miss_texel(ggs, kifs, oracle):
    """Whole tiles and waves are culled: background colour and (0, 0, 0, +inf) everywhere that misses."""
    screen, _, gui, iters = cases(kifs, W, H)["julia_24"]
    cam = kifs.CameraData(origin_distance=400.0, phi=0.3)
    _setup(ggs, screen, cam, gui, iters)
    st, colour, geom, _ = _call(ggs, kifs)
    assert st == 0
    want, hit, _ = GR.geometry_frame(oracle, kifs, screen, cam, gui, iters)
    _assert_same(_texels(geom[0], W), want, "far camera")
    assert (_texels(geom[0], W)[~hit].view(np.uint32) == GR.MISS).all() and (~hit).sum() > 0.99 * hit.size
    assert (colour[0] == ggs.render()).all()
    # off the fractal altogether: the camera looks away from it
    cam_u = cam.into_buffer_data()
    for r in range(3):  # (the view direction is minus the first column)
        cam_u.matrix[0][r] = -cam_u.matrix[0][r]
    ggs.set_raw_uniforms(camera=cam_u)
    st, colour, geom, _ = _call(ggs, kifs)
    assert st == 0
    assert (_texels(geom[0], W).view(np.uint32) == GR.MISS).all()
    assert (colour[0] == ggs.render()).all()


def test_camera_inside_a_primitive_hits_at_t_zero(ggs, kifs, oracle):
    screen, cam, gui, iters = cases(kifs, W, H)["sphere"]
    _setup(ggs, screen, cam, gui, iters)
    cam_u = cam.into_buffer_data()
    cam_u.origin[0], cam_u.origin[1], cam_u.origin[2] = 0.25, -0.125, 0.5  # inside the unit sphere
    ggs.set_raw_uniforms(camera=cam_u)
    st, colour, geom, _ = _call(ggs, kifs)
    assert st == 0
    s, _, o = oracle_uniforms(oracle, kifs, (screen, cam, gui))
    c = oracle.from_bytes(oracle.Camera, kifs.uniform_bytes(cam_u))
    want, hit, _ = GR.march(oracle, s, c, o, oracle.iters(*iters))
    assert hit.all() and (want[..., 3] == 0).all()
    _assert_same(_texels(geom[0], W), want, "inside")
    assert (colour[0] == oracle.render(s, c, o, oracle.iters(*iters))).all()


def test_no_iterations_all_misses(ggs, kifs):
    screen, cam, gui, iters = cases(kifs, W, H)["box"]
    gui = kifs.GuiData(**{**gui.__dict__, "max_iterations": 0})
    _setup(ggs, screen, cam, gui, iters)
    st, colour, geom, _ = _call(ggs, kifs)
    assert st == 0
    assert (_texels(geom[0], W).view(np.uint32) == GR.MISS).all()
    assert (colour[0] == ggs.render()).all()


@pytest.mark.parametrize("name", ["julia_24", "sierpinski"])
def test_heatmap_and_soft_shadows_change_the_colour_only(name, ggs, kifs, oracle):
    screen, cam, gui, iters = cases(kifs, W, H)[name]
    want = _reference(oracle, kifs, name)[0]
    heat = kifs.GuiData(**{**gui.__dict__, "is_heatmap": True, "fractal_color": (255, 128, 30)})
    _setup(ggs, screen, cam, heat, iters)
    st, colour, geom, _ = _call(ggs, kifs)
    assert st == 0
    assert (colour[0] == oracle_frame(oracle, kifs, screen, cam, heat, iters)).all()
    _assert_same(_texels(geom[0], W), want, (name, "heatmap"))
    _setup(ggs, screen, cam, gui, iters)
    plain = ggs.render()
    ggs.set_extensions(soft_shadow=True, shadow_steps=64, shadow_k=8.0, shadow_t0=0.02, shadow_max_t=10.0)
    try:
        st, colour, geom, _ = _call(ggs, kifs)
    finally:
        ggs.set_extensions(soft_shadow=False)
    assert st == 0
    s, c, o = oracle_uniforms(oracle, kifs, (screen, cam, gui))
    shadowed = oracle.render(s, c, o, oracle.iters(*iters), ext=oracle.Ext(1, 64, 8.0, 0.02, 10.0))
    assert (colour[0] == shadowed).all() and not (shadowed == plain).all()
    _assert_same(_texels(geom[0], W), want, (name, "soft shadows"))


def test_refusals_write_nothing(ggs, kifs):
    screen, cam, gui, iters = cases(kifs, W, H)["torus"]
    _setup(ggs, screen, cam, gui, iters)
    ggs.set_supersampling(2)
    try:
        st, colour, _, host = _call(ggs, kifs)
    finally:
        ggs.set_supersampling(1)
    assert st == BAD_ARG and (colour == SENT_U8).all() and (host == SENT_F32).all()
    cams = [cam, cam]
    for kw in (dict(misalign=4), dict(misalign=8), dict(gpitch=16 * W - 16), dict(gpitch=16 * W + 8),
               dict(cams=cams, count=2, gstride=H * 16 * W - 16), dict(cams=cams, count=2, gstride=H * 16 * W + 8),
               dict(gstride=8)):
        st, colour, _, host = _call(ggs, kifs, **kw)
        assert st == BAD_ARG, kw
        assert (colour == SENT_U8).all() and (host == SENT_F32).all(), kw
    st, _, _, _ = _call(ggs, kifs, gstride=0)  # one frame: any multiple of 16 will do
    assert st == 0


def test_no_side_effects_on_the_plain_path(kifs, oracle):
    """A 720p Julia frame has enough tiles for the tile-cost feedback: geometry launches in between neither record
    costs nor move the sort, and the plain frames around them are the same bytes from the same kernel."""
    screen, cam, gui, iters = cases(kifs, 1280, 720)["julia_24"]
    with kifs.GraphicState(0, screen_data=screen, camera_data=cam, gui_data=gui) as g:
        g.set_iters(*iters)
        frames = [g.render() for _ in range(5)]
        assert all((f == frames[0]).all() for f in frames)
        kernel = g.debug_last_kernel()
        before = g.debug_get_tile_order()
        for _ in range(5):
            colour, geometry = g.render_geometry()
            assert g.debug_last_kernel() == "render_geometry_kernel"
            from kifs_raymarching_amd._lib import lib
            assert lib.kifs_debug_last_kernel(g._ctx) == 6
            assert (g.debug_get_tile_order() == before).all()
        assert (colour.cpu().numpy() == frames[0]).all()
        hit = np.isfinite(geometry.cpu().numpy()[..., 3])
        assert hit.any() and not hit.all()
        after = g.render()
        assert (after == frames[0]).all() and g.debug_last_kernel() == kernel != "render_geometry_kernel"


def _fuzz_band(index, h):
    """A band of the frame with neither end a multiple of 8 (frames are at least 9 rows high)."""
    rng = X.scene_rng(index, 0x6e0)
    y0 = int(rng.integers(1, min(8, h - 1)))
    y1 = int(rng.choice([y for y in range(y0 + 1, h + 1) if y % 8]))
    return y0, y1


@pytest.mark.parametrize("index", range(X.N))
def test_fuzz_scene_bit_exact(index, ggs, kifs, oracle):
    """A seeded scene, lone; every third one also as a 3-view batch that mixes camera families, every second of those as a
    band into a padded geometry pitch.  With soft shadows only the colour changes."""
    scene = X.scenes(kifs)[index]
    name, family, screen, cam, gui, iters, encode = scene
    what = S.describe(index, scene)
    w, h = screen.width, screen.height
    shadow = S.shadow_of(oracle, kifs, index)
    launches = [(None, 0, h, None)]
    if X.has_batch(index):
        band = X.has_band(index)
        launches.append((X.batch_cameras(kifs, index, scene, 0x6e0), *(_fuzz_band(index, h) if band else (0, h)),
                         16 * w + 48 if band else None))
    S.setup(ggs, screen, cam, gui, iters, shadow=shadow)
    try:
        results = []
        for cams, y0, y1, gpitch in launches:
            results.append(_call(ggs, kifs, cams=cams, count=1 if cams is None else len(cams), y0=y0, y1=y1, encode=encode,
                                 gpitch=gpitch, cpad=24))
            assert ggs.debug_last_kernel() == "render_geometry_kernel", what
    finally:
        ggs.set_extensions(soft_shadow=False)
    for (cams, y0, y1, gpitch), (st, colour, geom, host) in zip(launches, results):
        assert st == 0, what
        rows, gpitch = y1 - y0, 16 * w if gpitch is None else gpitch
        for v, c in enumerate([cam] if cams is None else cams):
            view = f"{what}; view {v} of {len(colour)} ({c}), rows {y0}..{y1}"
            bad = (colour[v] != S.expected_colour(oracle, kifs, screen, c, gui, iters, encode, shadow, y0, y1)).any(-1)
            assert not bad.any(), f"{view}: colour: {S.first(bad)}"
            # the texels never depend on the extension: the reference marches without it
            want = S.geometry(oracle, kifs, index)[0][y0:y1] if v == 0 else \
                GR.geometry_frame(oracle, kifs, screen, c, gui, iters, y0, y1)[0]
            bad = ~GR.same_bits(_texels(geom[v], w), want)
            assert not bad.any(), f"{view}: texels: {S.first(bad)}, got {_texels(geom[v], w)[bad][0]!r}, want {want[bad][0]!r}"
            assert (geom[v][:, 4 * w:] == SENT_F32).all(), f"{view}: the padding of the rows"
        assert (host[len(colour) * rows * gpitch // 4:] == SENT_F32).all(), f"{what}: past the last plane"
