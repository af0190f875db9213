"""k x k supersampled anti-aliasing on the GPU (kifs_set_supersampling, kifs_ssaa_kernels.hip): bit-exact against the
oracle's resolve of the virtual frame (tests/aa_reference.py) for every pipeline, k = 2..4 and both encodes; every
render entry point (lone frame, band, batch, batch through the device view table, packed and in-place shards,
kifs_multi) gives the lone frame's bytes; k = 1 is the plain path; the size limit of the virtual screen; the seeded scenes
of tests/extension_fuzz_cases.py, lone and in batches, from cameras inside, on and just outside the bounding sphere.  These tests use
their own contexts: the session's `gs` stays at k = 1."""
import ctypes as C

import numpy as np
import pytest

import aa_reference as AA
import extension_fuzz_cases as X
import extension_fuzz_support as S
from helpers import diff_report, oracle_frame

pytestmark = pytest.mark.gpu


class _Raw:
    """An options image passed through where the helpers expect GuiData (the unknown primitive id)."""

    def __init__(self, u):
        self.u = u

    def into_buffer_data(self):
        return self.u


def _cases(K):
    from kifs_raymarching_amd.configs import JULIA_C
    S, Cam, G = K.ScreenData, K.CameraData, K.GuiData
    FG, PS = K.FractalGroup, K.PrimitiveShape
    near = Cam(origin_distance=3.5, phi=0.6, theta=0.5)
    prim = lambda p: G(primitive_shape=p, fractal_color=(250, 120, 60), background_color=(5, 5, 30))
    unknown = G(background_color=(30, 60, 90)).into_buffer_data()
    unknown.primitive_id = 17
    return {  # name: (screen, camera, gui, iters, k)
        "julia_12": (S(150, 94), Cam(origin_distance=3.0, phi=0.3), G(max_iterations=128, fractal_group=FG.JuliaSet,
                                                                      constant=JULIA_C), (12, 10, 10), 2),
        "julia_100": (S(96, 64), Cam(origin_distance=2.5, phi=0.7, theta=0.4), G(max_iterations=128, fractal_group=FG.JuliaSet),
                      (100, 10, 10), 3),
        "julia_heatmap": (S(150, 94), Cam(origin_distance=3.0), G(fractal_group=FG.JuliaSet, is_heatmap=True, constant=JULIA_C,
                                                                  fractal_color=(255, 128, 30)), (12, 10, 10), 2),
        "genjulia_p2": (S(96, 64), Cam(origin_distance=3.0), G(max_iterations=64, fractal_group=FG.GeneralizedJuliaSet,
                                                               constant=JULIA_C), (8, 4, 10), 2),
        "genjulia_p3.5": (S(64, 48), Cam(origin_distance=3.0, phi=0.5), G(max_iterations=64, fractal_group=FG.GeneralizedJuliaSet,
                                                                          power=3.5), (8, 4, 10), 3),
        "sierpinski": (S(96, 64), Cam(origin_distance=3.0, phi=1.0, theta=0.3),
                       G(primitive_shape=PS.SierpinskiTetrahedron, background_color=(10, 40, 90)), (100, 10, 10), 4),
        "sphere": (S(150, 94), near, prim(PS.Sphere), (100, 10, 10), 2),
        "cylinder": (S(96, 64), near, prim(PS.Cylinder), (100, 10, 10), 3),
        "box": (S(96, 64), near, prim(PS.Box), (100, 10, 10), 4),
        "torus": (S(150, 94), near, prim(PS.Torus), (100, 10, 10), 2),
        "unknown_id": (S(64, 48), near, _Raw(unknown), (100, 10, 10), 3),
        "bunny": (S(64, 48), Cam(origin_distance=2.6, phi=2.1, theta=-0.4), prim(PS.Bunny), (100, 10, 10), 2),
    }


_LINEAR = {}


def _linear(oracle, kifs, name):
    if name not in _LINEAR:
        screen, cam, gui, iters, k = _cases(kifs)[name]
        _LINEAR[name] = AA.linear_samples(oracle, kifs, screen, cam, gui, iters, k)
    return _LINEAR[name]


@pytest.fixture(scope="module")
def ags(kifs):
    g = kifs.GraphicState(0)
    yield g
    g.close()


def _setup(g, screen, cam, gui, iters, k):
    g.update_screen_data(screen)
    g.set_camera(cam)
    if isinstance(gui, _Raw):
        g.set_raw_uniforms(options=gui.u)
    else:
        g.update_options(gui)
    g.set_iters(*iters)
    g.set_supersampling(k)


@pytest.mark.parametrize("name", ["julia_12", "julia_100", "julia_heatmap", "genjulia_p2", "genjulia_p3.5", "sierpinski",
                                  "sphere", "cylinder", "box", "torus", "unknown_id", "bunny"])
@pytest.mark.parametrize("encode", [1, 0])
def test_aa_frame_bit_exact(name, encode, ags, kifs, oracle):
    screen, cam, gui, iters, k = _cases(kifs)[name]
    want = AA.aa_frame(oracle, kifs, screen, cam, gui, iters, k, encode, lin=_linear(oracle, kifs, name))
    _setup(ags, screen, cam, gui, iters, k)
    got = ags.render(encode=encode)
    assert ags.debug_last_kernel() == "render_ssaa_kernel"
    assert ags.debug_last_round_steps() == 0 and ags.debug_last_group_tiles() == -1 and ags.debug_last_bunny_form() == -1
    assert got.shape == want.shape
    assert diff_report(got, want)["mismatched_pixels"] == 0, (name, k, encode, diff_report(got, want))
    if name != "unknown_id":  # anti-aliased: some pixels are neither of the plain frame's colours' extremes
        plain = oracle_frame(oracle, kifs, screen, cam, gui, iters, encode=encode)
        assert (got != plain).any()


def _julia(kifs):
    from kifs_raymarching_amd.configs import JULIA_C
    return kifs.GuiData(max_iterations=128, fractal_group=kifs.FractalGroup.JuliaSet, constant=JULIA_C), (12, 10, 10)


def test_back_to_k1_is_the_plain_path(kifs):
    gui, iters = _julia(kifs)
    screen = kifs.ScreenData(150, 94)
    cam = kifs.CameraData(origin_distance=3.0, phi=0.3)
    with kifs.GraphicState(0, screen_data=screen, camera_data=cam, gui_data=gui) as fresh, \
            kifs.GraphicState(0, screen_data=screen, camera_data=cam, gui_data=gui) as g:
        fresh.set_iters(*iters)
        g.set_iters(*iters)
        want = fresh.render()
        plain_kernel = fresh.debug_last_kernel()
        g.set_supersampling(2)
        aa = g.render()
        assert g.debug_last_kernel() == "render_ssaa_kernel" and not (aa == want).all()
        g.set_supersampling(1)
        got = g.render()
        assert (got == want).all() and g.debug_last_kernel() == plain_kernel != "render_ssaa_kernel"
        assert g.debug_last_round_steps() == fresh.debug_last_round_steps()


def test_plain_renders_around_aa_renders_match_the_oracle(kifs, oracle):
    """A 720p Julia frame has enough tiles for the tile-cost feedback; AA launches in between neither record costs nor
    move the sort, and every plain frame before and after stays the oracle's."""
    gui, iters = _julia(kifs)
    screen = kifs.ScreenData(1280, 720)
    cam = kifs.CameraData(origin_distance=3.0, phi=0.3)
    want = oracle_frame(oracle, kifs, screen, cam, gui, iters)
    with kifs.GraphicState(0, screen_data=screen, camera_data=cam, gui_data=gui) as g:
        g.set_iters(*iters)
        for _ in range(4):
            assert (g.render() == want).all()
        g.set_supersampling(2)
        aa = [g.render() for _ in range(5)]
        assert all((a == aa[0]).all() for a in aa) and g.debug_last_kernel() == "render_ssaa_kernel"
        g.set_supersampling(1)
        for _ in range(7):
            assert (g.render() == want).all()


def test_band_rows_equal_the_lone_frame(kifs):
    gui, iters = _julia(kifs)
    screen = kifs.ScreenData(150, 94)
    with kifs.GraphicState(0, screen_data=screen, camera_data=kifs.CameraData(origin_distance=3.0), gui_data=gui) as g:
        g.set_iters(*iters)
        g.set_supersampling(3)
        whole = g.render()
        for y0, y1 in ((0, 94), (13, 71), (40, 41), (88, 94)):
            band = g.render(y0=y0, y1=y1)
            assert (band == whole[y0:y1]).all(), (y0, y1)


@pytest.mark.parametrize("count", [3, 65])
def test_batch_frames_equal_lone_frames(kifs, count):
    import torch
    gui, iters = _julia(kifs)
    screen = kifs.ScreenData(96, 64)
    cams = [kifs.CameraData(origin_distance=3.0 + 0.01 * i, phi=0.37 * i, theta=0.2 * np.sin(i)) for i in range(count)]
    with kifs.GraphicState(0, screen_data=screen, camera_data=cams[0], gui_data=gui) as g:
        g.set_iters(*iters)
        g.set_supersampling(2)
        want = []
        for cam in cams:
            g.set_camera(cam)
            want.append(g.render())
        outs = [torch.full((64, 96, 4), 7, dtype=torch.uint8, device="cuda:0") for _ in cams]
        stream = torch.cuda.Stream()
        g.render_batch_async(outs, cams, stream=stream)
        stream.synchronize()
        assert g.debug_last_kernel() == "render_ssaa_kernel"
        for i, (o, w_) in enumerate(zip(outs, want)):
            assert (o.cpu().numpy() == w_).all(), i


def test_shards_packed_and_in_place_equal_the_lone_frame(kifs):
    import torch
    gui, iters = _julia(kifs)
    W, H = 150, 94
    screen = kifs.ScreenData(W, H)
    cams = [kifs.CameraData(origin_distance=3.0, phi=0.2 * i) for i in range(2)]
    with kifs.GraphicState(0, screen_data=screen, camera_data=cams[0], gui_data=gui) as g:
        g.set_iters(*iters)
        g.set_supersampling(2)
        want = []
        for cam in cams:
            g.set_camera(cam)
            want.append(g.render())
        stream = torch.cuda.Stream()
        inplace = torch.zeros((2, H, W, 4), dtype=torch.uint8, device="cuda:0")
        for r in range(3):
            stripes, rows = kifs.shard_stripes(H, r, 3)
            shard = torch.full((2, rows, W, 4), 0x5A, dtype=torch.uint8, device="cuda:0")
            g.render_shard_async([shard[i] for i in range(2)], cams, stripes, in_place=False, stream=stream)
            g.render_shard_async([inplace[i] for i in range(2)], cams, stripes, in_place=True, stream=stream)
            stream.synchronize()
            got = shard.cpu().numpy()
            for f in range(2):
                for slot, s in enumerate(stripes):
                    n = min(8, H - 8 * s)
                    assert (got[f, 8 * slot:8 * slot + n] == want[f][8 * s:8 * s + n]).all(), (r, f, s)
        for f in range(2):
            assert (inplace[f].cpu().numpy() == want[f]).all(), f


@pytest.mark.parametrize("gather", ["sparse", "dense"])
def test_multi_equals_the_single_device_frame(kifs, gather):
    import torch
    gui, iters = _julia(kifs)
    W, H = 150, 94
    screen = kifs.ScreenData(W, H)
    cams = [kifs.CameraData(origin_distance=3.0, phi=0.3 * i) for i in range(3)]
    with kifs.GraphicState(0, screen_data=screen, camera_data=cams[0], gui_data=gui) as g:
        g.set_iters(*iters)
        g.set_supersampling(2)
        want = []
        for cam in cams:
            g.set_camera(cam)
            want.append(g.render())
    with kifs.MultiGraphicState([0, 0], screen, cams[0], gui, iters=iters) as mg:
        mg.set_supersampling(2)
        mg.set_gather(gather, "copy")
        frames = torch.full((3, H, W, 4), 99, dtype=torch.uint8, device="cuda:0")
        mg.render_batch(frames, cams)
        for i in range(3):
            assert (frames[i].cpu().numpy() == want[i]).all(), (gather, i)
        assert mg.stats()["transport"] == "copy"
        assert (mg.render() == want[0]).all()


def test_soft_shadows_per_sample(kifs, oracle):
    """Shadows apply per sample: every output byte lies within +-1 of the range of its k^2 samples' bytes in the
    oracle's virtual frame with the extension (its mean lies in the range of the linear samples; encoding is monotone)."""
    from helpers import oracle_uniforms
    k = 2
    screen = kifs.ScreenData(96, 64)
    cam = kifs.CameraData(origin_distance=3.0, phi=1.0, theta=0.3)
    gui = kifs.GuiData(primitive_shape=kifs.PrimitiveShape.SierpinskiTetrahedron, background_color=(10, 40, 90))
    iters = (100, 10, 10)
    ext = dict(soft_shadow=True, shadow_steps=64, shadow_k=8.0, shadow_t0=0.02, shadow_max_t=10.0)
    s, c, o = oracle_uniforms(oracle, kifs, (screen, cam, gui))
    virt = oracle.render(AA.virtual_screen(oracle, s, k), c, o, oracle.iters(*iters),
                         ext=oracle.Ext(1, 64, 8.0, 0.02, 10.0)).astype(np.int16)
    blocks = virt.reshape(64, k, 96, k, 4)
    lo, hi = blocks.min(axis=(1, 3)), blocks.max(axis=(1, 3))
    with kifs.GraphicState(0, screen_data=screen, camera_data=cam, gui_data=gui) as g:
        g.set_iters(*iters)
        g.set_supersampling(k)
        plain_aa = g.render()
        g.set_extensions(**ext)
        a, b = g.render(), g.render()
    assert (a == b).all()
    assert not (a == plain_aa).all()
    a16 = a.astype(np.int16)
    assert ((a16 >= lo - 1) & (a16 <= hi + 1)).all()


def test_virtual_screen_beyond_the_limit(kifs):
    import torch
    gui, iters = _julia(kifs)
    from kifs_raymarching_amd._lib import lib
    for (W, H) in ((20000, 8), (8, 20000)):
        with kifs.GraphicState(0, screen_data=kifs.ScreenData(W, H), camera_data=kifs.CameraData(), gui_data=gui) as g:
            g.set_iters(*iters)
            g.set_supersampling(4)  # 4 x 20000 > 65536
            host = np.full((H, W, 4), 7, dtype=np.uint8)
            assert lib.kifs_render(g._ctx, host.ctypes.data, W * 4, 0, H, 1) == 3
            assert (host == 7).all()
            dev = torch.full((H, W, 4), 7, dtype=torch.uint8, device="cuda:0")
            torch.cuda.synchronize()
            assert lib.kifs_render_async(g._ctx, None, dev.data_ptr(), W * 4, 0, H, 1) == 3
            ptrs = (C.c_void_p * 1)(dev.data_ptr())
            cams = kifs.camera_array([kifs.CameraData()])
            assert lib.kifs_render_batch_async(g._ctx, None, 1, cams, ptrs, W * 4, 0, H, 1) == 3
            assert lib.kifs_synchronize(g._ctx) == 0
            assert bool((dev == 7).all())
            g.set_supersampling(3)  # 3 x 20000 <= 65536: renders
            assert lib.kifs_render_async(g._ctx, None, dev.data_ptr(), W * 4, 0, H, 1) == 0
            lib.kifs_synchronize(g._ctx)
            assert not bool((dev == 7).all())


FUZZ_SENT = 0xA5  # (alpha is 255 in every pixel a kernel stores)


def _fuzz_check(got, want, what):
    bad = (got != want).any(-1)
    assert not bad.any(), f"{what}: {S.first(bad)}: got {got[bad][0]}, want {want[bad][0]}"


@pytest.mark.parametrize("index", range(X.N))
def test_fuzz_scene_bit_exact(index, ags, kifs, oracle):
    """A seeded scene at k = 2 + index % 3 through `render`; every third one also as a 3-view batch that mixes camera
    families; then k = 1 again: the plain frame.  Every fourth scene runs with soft shadows, against the oracle's resolve of
    samples shaded with the extension (kor_shade_pixel_ext): bit for bit like the rest."""
    import torch
    scene = X.scenes(kifs)[index]
    name, family, screen, cam, gui, iters, encode = scene
    what = S.describe(index, scene)
    w, h, k = screen.width, screen.height, X.supersampling(index)
    shadow = S.shadow_of(oracle, kifs, index)
    cams = [cam] + (X.batch_cameras(kifs, index, scene, 0x55a) if X.has_batch(index) else [])
    pitch = 4 * w + 32
    dest = torch.full((len(cams), h * pitch + 64), FUZZ_SENT, dtype=torch.uint8, device="cuda:0")
    plain = torch.full((h * pitch + 64,), FUZZ_SENT, dtype=torch.uint8, device="cuda:0")
    torch.cuda.synchronize()
    S.setup(ags, screen, cam, gui, iters, k=k, shadow=shadow)
    try:
        ags.render(out=dest[0], encode=encode, pitch_bytes=pitch)
        assert ags.debug_last_kernel() == "render_ssaa_kernel", what
        if len(cams) > 1:
            stream = torch.cuda.Stream()
            ags.render_batch_async([dest[v] for v in range(1, 4)], cams[1:], stream=stream, encode=encode, pitch_bytes=pitch)
            stream.synchronize()
            assert ags.debug_last_kernel() == "render_ssaa_kernel", what
        ags.set_supersampling(1)
        ags.render(out=plain, encode=encode, pitch_bytes=pitch)
        assert ags.debug_last_kernel() != "render_ssaa_kernel", what
        ags.synchronize()
    finally:
        ags.set_supersampling(1)
        ags.set_extensions(soft_shadow=False)
    host = dest.cpu().numpy()
    rows = host[:, :h * pitch].reshape(len(cams), h, pitch)
    assert (rows[:, :, 4 * w:] == FUZZ_SENT).all() and (host[:, h * pitch:] == FUZZ_SENT).all(), f"{what}: a store outside the frame"
    for v, c in enumerate(cams):
        view = f"{what}; k {k}, {'lone' if v == 0 else f'batch view {v - 1}'} ({c})"
        got = rows[v][:, :4 * w].reshape(h, w, 4)
        if v == 1:  # the batch's first view has the lone frame's camera: the same bytes, already compared
            bad = (got != rows[0][:, :4 * w].reshape(h, w, 4)).any(-1)
            assert not bad.any(), f"{view}: not the lone frame: {S.first(bad)}"
            continue
        _fuzz_check(got, AA.aa_frame(oracle, kifs, screen, c, gui, iters, k, encode, ext=X.oracle_ext(oracle, shadow)), view)
    got = plain.cpu().numpy()
    assert (got[h * pitch:] == FUZZ_SENT).all() and (got[:h * pitch].reshape(h, pitch)[:, 4 * w:] == FUZZ_SENT).all(), what
    _fuzz_check(got[:h * pitch].reshape(h, pitch)[:, :4 * w].reshape(h, w, 4),
                S.expected_colour(oracle, kifs, screen, cam, gui, iters, encode, shadow), f"{what}; back at k 1")
