"""Ambient occlusion on the GPU (kifs_render_occlusion_async, kifs_occlusion_kernels.hip), bit for bit: for every pipeline
and both encodes the colour bytes and the plane of factors equal the CPU restatement of the contract
(tests/occlusion_reference.c, held to the oracle by tests/test_occlusion_reference.py, which also shows that these scenes
at this size exercise the term).  Planes are compared by bit pattern, any NaN equal to any NaN; bytes exactly; no
tolerance: both sides run the contract's operation sequence.  Frames are 102 x 45 unless said -- width no multiple of 32,
height no multiple of 8, four tile columns and six tile rows -- and every destination is pre-filled with a sentinel and
padded, so that a missing store and a store outside the frame both show."""
import ctypes as C

import numpy as np
import pytest

import occlusion_reference as OR
from geometry_cases import PIPELINES, Raw, cases

pytestmark = pytest.mark.gpu

W, H = 102, 45
OK, BAD_SIZE, UNCONFIGURED, BAD_ARG = 0, 3, 4, 7
SENT_U8 = 0xA5
SENT_F32 = np.float32(-12345.5)
SHADOWS = dict(soft_shadow=True, shadow_steps=64, shadow_k=8.0, shadow_t0=0.02, shadow_max_t=10.0)


@pytest.fixture(scope="module")
def ogs(kifs):
    g = kifs.GraphicState(0)
    yield g
    g.close()


def test_status_codes_are_the_headers(kifs):
    import re
    from pathlib import Path
    header = (Path(__file__).resolve().parent.parent / "include" / "kifs_hip.h").read_text()
    for name, value in (("KIFS_ERR_BAD_SIZE", BAD_SIZE), ("KIFS_ERR_UNCONFIGURED", UNCONFIGURED), ("KIFS_ERR_BAD_ARG", BAD_ARG)):
        assert re.search(rf"\b{name}\s*=\s*{value}\b", header), name


def _setup(g, screen, cam, gui, iters, k=1, shadows=False):
    g.update_screen_data(screen)
    g.set_camera(cam)
    if isinstance(gui, Raw):
        g.set_raw_uniforms(options=gui.u)
    else:
        g.update_options(gui)
    g.set_iters(*iters)
    g.set_extensions(**SHADOWS) if shadows else g.set_extensions(soft_shadow=False)
    g.set_supersampling(k)


class Result:
    def __init__(self, st, colour, plane, colour_raw, plane_raw):
        self.st, self.colour, self.plane, self.colour_raw, self.plane_raw = st, colour, plane, colour_raw, plane_raw

    def untouched(self):
        return (self.colour_raw == SENT_U8).all() and (self.plane_raw == SENT_F32).all()


def _call(g, kifs, ao=OR.DEFAULT, cams=None, count=1, y0=0, y1=None, encode=1, plane=True, ppad=20, spad=32, cpad=12,
          ppitch=None, pstride=None, misalign=0, term=None, outs="given", ctx="given", null_out=None):
    """The raw entry point on sentinel-filled, padded destinations.  colour: (count, rows, W, 4) uint8; plane:
    (count, rows, W) float32 or None.  The padding of every colour row, plane row and plane is asserted to hold the
    sentinel after a call that succeeded."""
    import torch
    from kifs_raymarching_amd._lib import AmbientOcclusionC, lib
    w, h = g.screen_data.width, g.screen_data.height
    y1 = h if y1 is None else y1
    rows = max(y1 - y0, 0)
    cpitch = 4 * w + cpad
    ppitch = 4 * w + ppad if ppitch is None else ppitch
    pstride = rows * ppitch + spad if pstride is None else pstride
    colour = torch.full((count, rows * cpitch + 64), SENT_U8, dtype=torch.uint8, device="cuda:0")
    floats = (count * max(pstride, rows * ppitch)) // 4 + 16
    pl = torch.full((floats,), float(SENT_F32), dtype=torch.float32, device="cuda:0")
    torch.cuda.synchronize()
    ptrs = (C.c_void_p * count)(*[colour[i].data_ptr() for i in range(count)])
    if null_out is not None:
        ptrs[null_out] = None
    arr = None if cams is None else kifs.camera_array(cams)
    t = AmbientOcclusionC(int(ao[0]), float(ao[1]), float(ao[2]), float(ao[3])) if term is None else term
    st = lib.kifs_render_occlusion_async(g._ctx if ctx == "given" else None, None, count, arr, ptrs if outs == "given" else None,
                                         cpitch, None if t == "null" else C.byref(t), (pl.data_ptr() + misalign) if plane else None,
                                         ppitch, pstride, y0, y1, encode)
    assert lib.kifs_synchronize(g._ctx) == 0
    chost, phost = colour.cpu().numpy(), pl.cpu().numpy()
    if st != OK:
        return Result(st, None, None, chost, phost)
    crows = chost[:, :rows * cpitch].reshape(count, rows, cpitch)
    assert (crows[:, :, 4 * w:] == SENT_U8).all() and (chost[:, rows * cpitch:] == SENT_U8).all(), "a colour store outside the frame"
    got = np.ascontiguousarray(crows[:, :, :4 * w]).reshape(count, rows, w, 4)
    if not plane:
        assert (phost == SENT_F32).all(), "a plane store without a plane"
        return Result(st, got, None, chost, phost)
    planes = np.stack([phost[i * pstride // 4: i * pstride // 4 + rows * ppitch // 4].reshape(rows, ppitch // 4)
                       for i in range(count)]) if rows else np.zeros((count, 0, w), dtype=np.float32)
    assert (planes[:, :, w:] == SENT_F32).all(), "a plane store beyond 4 W of a row"
    for i in range(count):
        gap = phost[(i * pstride + rows * ppitch) // 4: ((i + 1) * pstride) // 4 if i + 1 < count else None]
        assert (gap == SENT_F32).all(), "a plane store between or past the planes"
    return Result(st, got, np.ascontiguousarray(planes[:, :, :w]), chost, phost)


_MODEL = {}


def _model(oracle, kifs, scene, ao, shadows=False, key=None):
    """The modelled frame of a scene (screen, cam, gui, iters), computed once per (key, term, shadows)."""
    key = (key, tuple(ao), shadows)
    if key[0] is None or key not in _MODEL:
        screen, cam, gui, iters = scene
        ext = oracle.Ext(1, 64, 8.0, 0.02, 10.0) if shadows else None
        m = OR.occlusion_frame(oracle, kifs, screen, cam, gui, iters, ao, ext)
        if key[0] is None:
            return m
        _MODEL[key] = m
    return _MODEL[key]


def _assert_plane(got, want, what):
    same = OR.same_bits(got, want)
    if not same.all():
        at = tuple(np.argwhere(~same)[0])
        pytest.fail(f"{what}: {int((~same).sum())} of {same.size} factors differ; first at {at}: "
                    f"got {got[at]!r} ({got[at].view(np.uint32):#x}), want {want[at]!r} ({want[at].view(np.uint32):#x})")


def _assert_bytes(got, want, what):
    bad = (got != want).any(-1)
    if bad.any():
        at = tuple(np.argwhere(bad)[0])
        pytest.fail(f"{what}: {int(bad.sum())} of {bad.size} pixels differ; first at {at}: got {got[at]}, want {want[at]}")


@pytest.mark.parametrize("name", PIPELINES)
@pytest.mark.parametrize("encode", [1, 0])
def test_every_pipeline_bit_exact(name, encode, ogs, kifs, oracle):
    scene = cases(kifs, W, H)[name]
    _setup(ogs, *scene)
    m = _model(oracle, kifs, scene, OR.DEFAULT, key=name)
    r = _call(ogs, kifs, OR.DEFAULT, encode=encode)
    assert r.st == OK
    print(name, "hits", int(m.hit.sum()), "partial factors", int((m.hit & (m.plane > 0) & (m.plane < 1)).sum()))
    _assert_bytes(r.colour[0], OR.encode(oracle, m.rgb, encode), (name, encode))
    _assert_plane(r.plane[0], m.plane, (name, encode))
    # the bytes do not depend on whether the plane is asked for
    assert (_call(ogs, kifs, OR.DEFAULT, encode=encode, plane=False).colour == r.colour).all()
    if name != "unknown_id":
        assert m.hit.any() and not m.hit.all()


@pytest.mark.parametrize("name", ["julia_24", "sierpinski"])
def test_many_probes_without_decay(name, ogs, kifs, oracle):
    scene = cases(kifs, W, H)[name]
    _setup(ogs, *scene)
    m = _model(oracle, kifs, scene, OR.DEEP, key=name)
    r = _call(ogs, kifs, OR.DEEP)
    assert r.st == OK and int((m.hit & (m.plane == 0)).sum()) >= 20
    _assert_bytes(r.colour[0], OR.encode(oracle, m.rgb, 1), name)
    _assert_plane(r.plane[0], m.plane, name)


@pytest.mark.parametrize("name", ["julia_24", "sierpinski", "sphere"])
def test_strength_zero_is_the_plain_frame(name, ogs, kifs, oracle):
    scene = cases(kifs, W, H)[name]
    _setup(ogs, *scene)
    ao = (5, 0.02, 0.75, 0.0)
    m = _model(oracle, kifs, scene, ao, key=name)
    r = _call(ogs, kifs, ao)
    assert r.st == OK
    _assert_bytes(r.colour[0], OR.encode(oracle, m.rgb, 1), name)
    _assert_plane(r.plane[0], m.plane, name)
    _assert_bytes(r.colour[0], ogs.render(), (name, "GraphicState.render"))


@pytest.mark.parametrize("name", ["julia_24", "sierpinski"])
def test_soft_shadows_are_attenuated_too(name, ogs, kifs, oracle):
    scene = cases(kifs, W, H)[name]
    _setup(ogs, *scene, shadows=True)
    try:
        r = _call(ogs, kifs, OR.DEFAULT)
    finally:
        ogs.set_extensions(soft_shadow=False)
    assert r.st == OK
    m = _model(oracle, kifs, scene, OR.DEFAULT, shadows=True, key=name)
    plain = _model(oracle, kifs, scene, OR.DEFAULT, key=name)
    assert not OR.same_bits(m.rgb, plain.rgb).all()  # the shadows do change this frame
    _assert_bytes(r.colour[0], OR.encode(oracle, m.rgb, 1), name)
    _assert_plane(r.plane[0], m.plane, name)


def test_heatmap_colour_is_the_counters_and_the_plane_is_the_hits(ogs, kifs, oracle):
    screen, cam, gui, iters = cases(kifs, W, H)["julia_24"]
    heat = kifs.GuiData(**{**gui.__dict__, "is_heatmap": True, "fractal_color": (255, 128, 30)})
    scene = (screen, cam, heat, iters)
    _setup(ogs, *scene)
    r = _call(ogs, kifs, OR.DEFAULT)
    assert r.st == OK
    _assert_bytes(r.colour[0], ogs.render(), "plain heatmap render")
    m = _model(oracle, kifs, scene, OR.DEFAULT)
    _assert_bytes(r.colour[0], OR.encode(oracle, m.rgb, 1), "model")
    _assert_plane(r.plane[0], m.plane, "heatmap")
    assert (m.hit & (m.plane < 1)).sum() >= 32


@pytest.mark.parametrize("name", ["julia_24", "sierpinski"])
@pytest.mark.parametrize("k", [2, 3])
def test_supersampled_samples_are_attenuated_one_by_one(name, k, ogs, kifs, oracle):
    screen, cam, gui, iters = scene = cases(kifs, 70, 21)[name]
    _setup(ogs, *scene, k=k)
    try:
        r = _call(ogs, kifs, OR.DEFAULT, plane=False)
        refused = _call(ogs, kifs, OR.DEFAULT, plane=True) if k == 2 else None
    finally:
        ogs.set_supersampling(1)
    assert r.st == OK
    _assert_bytes(r.colour[0], OR.supersampled_bytes(oracle, kifs, screen, cam, gui, iters, OR.DEFAULT, k), (name, k))
    if refused is not None:  # a resolved pixel has no single factor
        assert refused.st == BAD_ARG and refused.untouched()


def _lone(g, kifs, cam, **kw):
    g.set_camera(cam)
    r = _call(g, kifs, **kw)  # cameras NULL, count 1: the context's camera
    assert r.st == OK
    return r


def test_three_views_one_inside_the_bounding_sphere(ogs, kifs, oracle):
    screen, cam, gui, iters = scene = cases(kifs, W, H)["julia_24"]
    cams = [cam, kifs.CameraData(origin_distance=1.6, phi=2.0, theta=-0.3), kifs.CameraData(origin_distance=4.5, phi=4.0, theta=0.6)]
    _setup(ogs, *scene)
    r = _call(ogs, kifs, cams=cams, count=3)
    assert r.st == OK
    for i, c in enumerate(cams):
        one = _lone(ogs, kifs, c)
        _assert_bytes(r.colour[i], one.colour[0], ("view", i))
        _assert_plane(r.plane[i], one.plane[0], ("view", i))
    # the lone call with cameras NULL is the context's camera: the model's frame for it ...
    m = _model(oracle, kifs, (screen, cams[1], gui, iters), OR.DEFAULT)
    origin = np.array(list(cams[1].into_buffer_data().origin), dtype=np.float64)
    assert np.linalg.norm(origin) < 2.0 and m.hit.any() and not m.hit.all()  # (inside the bounding sphere: no ray is culled)
    _assert_bytes(r.colour[1], OR.encode(oracle, m.rgb, 1), "inside")
    _assert_plane(r.plane[1], m.plane, "inside")
    # ... and a one-frame batch with an explicit camera does not use the context's
    ogs.set_camera(cams[0])
    one = _call(ogs, kifs, cams=[cams[2]], count=1)
    _assert_bytes(one.colour[0], r.colour[2], "explicit camera")


def test_sixty_four_views_each_the_lone_call(ogs, kifs):
    screen, cam, gui, iters = cases(kifs, 40, 24)["julia_24"]
    cams = [kifs.CameraData(origin_distance=2.2 + 0.02 * i, phi=0.37 * i, theta=0.4 * np.sin(i)) for i in range(64)]
    _setup(ogs, screen, cams[0], gui, iters)
    r = _call(ogs, kifs, cams=cams, count=64)
    assert r.st == OK
    for i in (0, 1, 17, 31, 62, 63):
        one = _lone(ogs, kifs, cams[i])
        _assert_bytes(r.colour[i], one.colour[0], ("view", i))
        _assert_plane(r.plane[i], one.plane[0], ("view", i))
    assert len({r.colour[i].tobytes() for i in range(64)}) == 64 and (r.plane < 1).any()


@pytest.mark.parametrize("name", ["julia_24", "torus"])
def test_band_equals_the_rows_of_the_full_frame(name, ogs, kifs, oracle):
    scene = cases(kifs, W, H)[name]
    _setup(ogs, *scene)
    m = _model(oracle, kifs, scene, OR.DEFAULT, key=name)
    full = _call(ogs, kifs)
    band = _call(ogs, kifs, y0=5, y1=30)
    assert full.st == OK and band.st == OK and band.colour.shape[1] == 25
    _assert_bytes(band.colour[0], full.colour[0][5:30], name)
    _assert_plane(band.plane[0], full.plane[0][5:30], name)
    _assert_plane(band.plane[0], m.plane[5:30], (name, "model"))
    empty = _call(ogs, kifs, y0=7, y1=7)
    assert empty.st == OK and empty.untouched()


def _bad_terms():
    from kifs_raymarching_amd._lib import AmbientOcclusionC as T
    nan, inf = float("nan"), float("inf")
    return [T(0, 0.02, 0.75, 4.0), T(17, 0.02, 0.75, 4.0), T(-1, 0.02, 0.75, 4.0),
            T(5, 0.0, 0.75, 4.0), T(5, -0.02, 0.75, 4.0), T(5, nan, 0.75, 4.0), T(5, inf, 0.75, 4.0),
            T(5, 0.02, 0.0, 4.0), T(5, 0.02, -0.5, 4.0), T(5, 0.02, 1.0000001, 4.0), T(5, 0.02, nan, 4.0), T(5, 0.02, inf, 4.0),
            T(5, 0.02, 0.75, -1.0e-6), T(5, 0.02, 0.75, nan), T(5, 0.02, 0.75, inf)]


def test_refusals_write_nothing(ogs, kifs):
    screen, cam, gui, iters = scene = cases(kifs, W, H)["torus"]
    _setup(ogs, *scene)
    two = [cam, cam]
    row = 4 * W + 20
    refusals = [dict(outs=None), dict(term="null"), dict(count=0, cams=[]), dict(count=65, cams=[cam] * 65),
                dict(count=2, cams=None), dict(encode=2), dict(encode=-1),
                dict(y0=-1), dict(y1=H + 1), dict(y0=10, y1=9),
                dict(ppitch=4 * W - 4), dict(ppitch=4 * W + 2), dict(misalign=2), dict(misalign=1), dict(pstride=H * row + 2),
                dict(cams=two, count=2, pstride=H * row - 4), dict(cams=two, count=2, pstride=0),
                dict(cams=two, count=2, null_out=1)]
    refusals += [dict(term=t) for t in _bad_terms()]
    for kw in refusals:
        r = _call(ogs, kifs, **kw)
        assert r.st == BAD_ARG, (kw, r.st)
        assert r.untouched(), kw
    r = _call(ogs, kifs, ctx=None)
    assert r.st == BAD_ARG and r.untouched()
    for kw in (dict(cpad=-4), dict(cpad=2)):  # the colour pitch: as the batch call refuses it
        r = _call(ogs, kifs, **kw)
        assert r.st == BAD_SIZE and r.untouched(), kw
    # the edges of the ranges are accepted; one frame needs no stride
    from kifs_raymarching_amd._lib import AmbientOcclusionC as T
    for t in (T(1, 1.0e-30, 1.0, 0.0), T(16, 3.0e38, 1.0e-30, 3.0e38)):
        assert _call(ogs, kifs, term=t).st == OK
    assert _call(ogs, kifs, pstride=0).st == OK and _call(ogs, kifs, ppad=0, spad=0, cpad=0).st == OK


def test_unconfigured_context_is_refused(kifs):
    screen, cam, gui, iters = cases(kifs, W, H)["torus"]
    from kifs_raymarching_amd._lib import lib
    g = kifs.GraphicState(0, screen_data=screen, camera_data=cam, gui_data=gui)
    try:
        st = C.c_int(-1)
        bare = lib.kifs_create(0, C.byref(st))
        assert bare and st.value == OK
        keep = g._ctx
        g._ctx = bare  # (the helper sizes its buffers from the GraphicState's screen)
        try:
            r = _call(g, kifs)
            assert r.st == UNCONFIGURED and r.untouched()
        finally:
            g._ctx = keep
            lib.kifs_destroy(bare)
    finally:
        g.close()


def _walk(kifs, screen, cam, gui, iters, with_call):
    """48-frame batch, lone render, [the occlusion calls], lone render, 48-frame batch on a fresh context: what each left
    behind.  In this arrangement the one set of costs that is ever sorted is the first batch's -- work counts, the same in
    every run; the lone render behind it sorts them beside the stream, the next one adopts the order -- so the order at
    the end is a property of the sequence (a lone launch's own costs are run times: an order made of them is not), and the
    calls sit where a sort is pending."""
    import torch
    cams = [kifs.CameraData(origin_distance=3.0 + 0.004 * i, phi=0.3 + 0.01 * i) for i in range(48)]
    seen = []
    with kifs.GraphicState(0, screen_data=screen, camera_data=cam, gui_data=gui) as g:
        g.set_iters(*iters)
        h, w = screen.height, screen.width

        def lone():
            seen.append((torch.from_numpy(g.render().copy()), g.debug_last_kernel(), g.debug_last_round_steps()))

        def batch():
            outs = torch.zeros((48, h, w, 4), dtype=torch.uint8, device="cuda:0")
            g.render_batch_async([outs[i] for i in range(48)], cams)
            g.synchronize()
            seen.append((outs.cpu(), g.debug_last_kernel(), g.debug_last_round_steps()))

        batch()
        lone()
        if with_call:
            from kifs_raymarching_amd._lib import lib
            before = (g.debug_last_kernel(), lib.kifs_debug_last_kernel(g._ctx), g.debug_last_round_steps(), g.debug_get_tile_order())
            colour, plane = g.render_occlusion(occlusion=True)
            after = (g.debug_last_kernel(), lib.kifs_debug_last_kernel(g._ctx), g.debug_last_round_steps(), g.debug_get_tile_order())
            assert before[:3] == after[:3] and (before[3] == after[3]).all()
            assert bool((plane < 1).any()) and bool((plane == 1).any())
            batch3, _ = g.render_occlusion_batch(cams[:3])
            g.synchronize()
            assert (g.debug_get_tile_order() == before[3]).all() and g.debug_last_kernel() == before[0]
            assert bool((batch3[0] == colour).all())  # (cams[0] is the context's camera)
        lone()
        batch()
        seen.append(g.debug_get_tile_order())
    return seen


def test_a_long_lived_context_does_not_notice_the_call(kifs):
    """1024 x 512 Julia: 2048 tiles, enough for the tile-cost feedback of lone frames and batches."""
    import torch
    screen, _, gui, iters = cases(kifs, 1024, 512)["julia_24"]
    cam = kifs.CameraData(origin_distance=3.0, phi=0.3)
    without = _walk(kifs, screen, cam, gui, iters, False)
    with_call = _walk(kifs, screen, cam, gui, iters, True)
    assert len(without) == len(with_call) == 5
    for step, (a, b) in enumerate(zip(without[:4], with_call[:4])):
        assert a[1:] == b[1:], (step, a[1:], b[1:])
        assert torch.equal(a[0], b[0]), step
    assert (without[4] == with_call[4]).all()
    ids = np.arange(2048)
    assert not (np.sort(without[4]) != np.sort((ids % 32) | ((ids // 32) << 16))).any()  # a permutation of the tiles


def test_the_python_layer_feeds_the_library_64_at_a_time(ogs, kifs):
    screen, cam, gui, iters = cases(kifs, 40, 24)["sierpinski"]
    cams = [kifs.CameraData(origin_distance=2.6 + 0.01 * i, phi=0.21 * i, theta=0.5 * np.cos(i)) for i in range(70)]
    _setup(ogs, screen, cams[0], gui, iters)
    ao = kifs.AmbientOcclusion(samples=7, step=0.03, decay=0.8, strength=3.0)
    colour, plane = ogs.render_occlusion_batch(cams, ao=ao, occlusion=True)
    only, none = ogs.render_occlusion_batch(cams, ao=ao)
    ogs.synchronize()
    assert tuple(colour.shape) == (70, 24, 40, 4) and tuple(plane.shape) == (70, 24, 40) and none is None
    assert bool((only == colour).all())
    colour, plane = colour.cpu().numpy(), plane.cpu().numpy()
    for i, c in enumerate(cams):
        ogs.set_camera(c)
        c1, p1 = ogs.render_occlusion(ao=ao, occlusion=True)
        _assert_bytes(colour[i], c1.cpu().numpy(), ("frame", i))
        _assert_plane(plane[i], p1.cpu().numpy(), ("frame", i))
    one = _lone(ogs, kifs, cams[69], ao=(7, 0.03, 0.8, 3.0))  # ... which is the raw entry point's frame
    _assert_bytes(colour[69], one.colour[0], "raw")
    assert (kifs.AmbientOcclusion().samples, kifs.AmbientOcclusion().step, kifs.AmbientOcclusion().decay,
            kifs.AmbientOcclusion().strength) == (5, 0.02, 0.75, 4.0)
