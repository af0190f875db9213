"""The configurable light on the GPU (kifs_render_lit_async, kifs_lighting_kernels.hip), bit for bit: for every pipeline
and both encodes the bytes equal the CPU restatement of the contract (tests/lighting_reference.c, held to the oracle and
to the occlusion model by tests/test_lighting_reference.py, which also shows that these scenes at this size exercise the
light), and with the reference's light they are the bytes of the plain render and of the occlusion call.  Bytes exactly,
no tolerance: both sides run the contract's operation sequence.  Frames are 102 x 45 unless said -- width no multiple of
32, height no multiple of 8, four tile columns and six tile rows -- and every destination is pre-filled with a sentinel and
padded, so that a missing store and a store outside the frame both show.  The lights at the edges of what the entry point
accepts are compared like any other (test_accepted_edges_bit_exact); tests/test_gpu_shading_fuzz.py has the seeded scenes."""
import ctypes as C

import numpy as np
import pytest

import lighting_reference as LR
import occlusion_reference as OR
from geometry_cases import PIPELINES, Raw, cases

pytestmark = pytest.mark.gpu

W, H = 102, 45
OK, BAD_SIZE, UNCONFIGURED, BAD_ARG = 0, 3, 4, 7
SENT_U8 = 0xA5
SHADOWS = dict(soft_shadow=True, shadow_steps=64, shadow_k=8.0, shadow_t0=0.02, shadow_max_t=10.0)


@pytest.fixture(scope="module")
def lgs(kifs):
    g = kifs.GraphicState(0)
    yield g
    g.close()


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
    def __init__(self, st, colour, colour_raw):
        self.st, self.colour, self.colour_raw = st, colour, colour_raw

    def untouched(self):
        return (self.colour_raw == SENT_U8).all()


def _clight(spec):
    from kifs_raymarching_amd._lib import KifsLightC
    if isinstance(spec, KifsLightC):
        return spec
    return KifsLightC((C.c_float * 3)(*spec["direction"]), spec["ambient"], spec["diffuse"], (C.c_float * 3)(*spec["specular"]),
                      spec["shininess_log2"])


def _call(g, kifs, spec=LR.A, ao=None, cams=None, count=1, y0=0, y1=None, encode=1, cpad=12, outs="given", ctx="given",
          null_out=None, misalign_out=None, term=None):
    """The raw entry point on sentinel-filled, padded destinations.  colour: (count, rows, W, 4) uint8.  The padding of
    every row and the tail of every destination are asserted to hold the sentinel after a call that succeeded."""
    import torch
    from kifs_raymarching_amd._lib import AmbientOcclusionC, lib
    w, h = g.screen_data.width, g.screen_data.height
    y1 = h if y1 is None else y1
    rows = max(y1 - y0, 0)
    cpitch = 4 * w + cpad
    colour = torch.full((count, rows * cpitch + 64), SENT_U8, dtype=torch.uint8, device="cuda:0")
    torch.cuda.synchronize()
    ptrs = (C.c_void_p * count)(*[colour[i].data_ptr() for i in range(count)])
    if null_out is not None:
        ptrs[null_out] = None
    if misalign_out is not None:
        ptrs[misalign_out] = colour[misalign_out].data_ptr() + 2
    arr = None if cams is None else kifs.camera_array(cams)
    light = None if spec == "null" else _clight(spec)
    t = term if term is not None else (None if ao is None else AmbientOcclusionC(int(ao[0]), float(ao[1]), float(ao[2]), float(ao[3])))
    st = lib.kifs_render_lit_async(g._ctx if ctx == "given" else None, None, count, arr, ptrs if outs == "given" else None, cpitch,
                                   None if light is None else C.byref(light), None if t is None else C.byref(t), y0, y1, encode)
    assert lib.kifs_synchronize(g._ctx) == 0
    chost = colour.cpu().numpy()
    if st != OK:
        return Result(st, None, chost)
    crows = chost[:, :rows * cpitch].reshape(count, rows, cpitch)
    assert (crows[:, :, 4 * w:] == SENT_U8).all() and (chost[:, rows * cpitch:] == SENT_U8).all(), "a colour store outside the frame"
    return Result(st, np.ascontiguousarray(crows[:, :, :4 * w]).reshape(count, rows, w, 4), chost)


def _occlusion_bytes(g, ao, encode=1):
    """kifs_render_occlusion_async's bytes of the context's frame."""
    import torch
    from kifs_raymarching_amd._lib import AmbientOcclusionC, lib
    w, h = g.screen_data.width, g.screen_data.height
    out = torch.full((h, w, 4), SENT_U8, dtype=torch.uint8, device="cuda:0")
    torch.cuda.synchronize()
    ptrs = (C.c_void_p * 1)(out.data_ptr())
    t = AmbientOcclusionC(int(ao[0]), float(ao[1]), float(ao[2]), float(ao[3]))
    assert lib.kifs_render_occlusion_async(g._ctx, None, 1, None, ptrs, 4 * w, C.byref(t), None, 0, 0, 0, h, encode) == OK
    assert lib.kifs_synchronize(g._ctx) == 0
    return out.cpu().numpy()


_MODEL = {}


def _model(oracle, kifs, scene, spec_name, ao=None, shadows=False, key=None):
    """The modelled frame of a scene (screen, cam, gui, iters), computed once per (key, light, term, shadows)."""
    key = (key, spec_name, None if ao is None else tuple(ao), shadows)
    if key[0] is None or key not in _MODEL:
        screen, cam, gui, iters = scene
        ext = oracle.Ext(1, 64, 8.0, 0.02, 10.0) if shadows else None
        m = LR.lit_frame(oracle, kifs, screen, cam, gui, iters, getattr(LR, spec_name), ao, ext)
        if key[0] is None:
            return m
        _MODEL[key] = m
    return _MODEL[key]


def _assert_bytes(got, want, what):
    bad = (got != want).any(-1)
    if bad.any():
        at = tuple(np.argwhere(bad)[0])
        pytest.fail(f"{what}: {int(bad.sum())} of {bad.size} pixels differ; first at {at}: got {got[at]}, want {want[at]}")


@pytest.mark.parametrize("name", PIPELINES)
@pytest.mark.parametrize("encode", [1, 0])
def test_every_pipeline_bit_exact(name, encode, lgs, kifs, oracle):
    scene = cases(kifs, W, H)[name]
    _setup(lgs, *scene)
    m = _model(oracle, kifs, scene, "A", key=name)
    r = _call(lgs, kifs, LR.A, encode=encode)
    assert r.st == OK
    print(name, "hits", int(m.hit.sum()), "partially lit", int((m.hit & (m.lit0 > 0) & (m.lit0 < 1)).sum()),
          "highlit", int((m.hit & (m.lit0 > 0) & (m.s > 0.02)).sum()))
    _assert_bytes(r.colour[0], LR.encode(oracle, m.rgb, encode), (name, encode))
    if name != "unknown_id":
        assert m.hit.any() and not m.hit.all()


@pytest.mark.parametrize("shadows", [False, True])
@pytest.mark.parametrize("name", ["julia_24", "sierpinski", "sphere", "bunny"])
def test_reference_light_is_the_plain_render_and_the_occlusion_call(name, shadows, lgs, kifs):
    scene = cases(kifs, W, H)[name]
    _setup(lgs, *scene, shadows=shadows)
    try:
        plain = _call(lgs, kifs, LR.REFERENCE)
        any_e = _call(lgs, kifs, dict(LR.REFERENCE, shininess_log2=0))
        with_term = _call(lgs, kifs, LR.REFERENCE, ao=OR.DEFAULT)
        want_plain = lgs.render()
        want_term = _occlusion_bytes(lgs, OR.DEFAULT)
    finally:
        lgs.set_extensions(soft_shadow=False)
    assert plain.st == OK and any_e.st == OK and with_term.st == OK
    _assert_bytes(plain.colour[0], want_plain, (name, shadows, "GraphicState.render"))
    _assert_bytes(any_e.colour[0], want_plain, (name, shadows, "any e"))
    _assert_bytes(with_term.colour[0], want_term, (name, shadows, "kifs_render_occlusion_async"))


def test_reference_light_identities_hold_supersampled(lgs, kifs):
    scene = cases(kifs, 70, 21)["julia_24"]
    _setup(lgs, *scene, k=2, shadows=True)
    try:
        plain = _call(lgs, kifs, LR.REFERENCE)
        with_term = _call(lgs, kifs, LR.REFERENCE, ao=OR.DEFAULT)
        want_plain = lgs.render()
        want_term = _occlusion_bytes(lgs, OR.DEFAULT)
    finally:
        lgs.set_supersampling(1)
        lgs.set_extensions(soft_shadow=False)
    assert plain.st == OK and with_term.st == OK
    _assert_bytes(plain.colour[0], want_plain, "k = 2, GraphicState.render")
    _assert_bytes(with_term.colour[0], want_term, "k = 2, kifs_render_occlusion_async")


@pytest.mark.parametrize("name", ["julia_24", "sierpinski"])
def test_shadows_fall_away_from_the_light(name, lgs, kifs, oracle):
    scene = cases(kifs, W, H)[name]
    _setup(lgs, *scene, shadows=True)
    try:
        r = _call(lgs, kifs, LR.A)
    finally:
        lgs.set_extensions(soft_shadow=False)
    assert r.st == OK
    m = _model(oracle, kifs, scene, "A", shadows=True, key=name)
    plain = _model(oracle, kifs, scene, "A", key=name)
    assert not LR.same_bits(m.rgb, plain.rgb).all()  # the shadows do change this frame
    _assert_bytes(r.colour[0], LR.encode(oracle, m.rgb, 1), name)


@pytest.mark.parametrize("name", ["julia_24", "sierpinski"])
def test_everything_at_once(name, lgs, kifs, oracle):
    """Light A, the highlight at e = 5, shadows and the deep term."""
    scene = cases(kifs, W, H)[name]
    _setup(lgs, *scene, shadows=True)
    try:
        r = _call(lgs, kifs, LR.A5, ao=OR.DEEP)
    finally:
        lgs.set_extensions(soft_shadow=False)
    assert r.st == OK
    m = _model(oracle, kifs, scene, "A5", ao=OR.DEEP, shadows=True, key=name)
    assert (m.hit & (m.a == 0)).sum() >= 20 and (m.hit & (m.sh < 1)).any() and (m.hit & (m.s > 0)).any()
    _assert_bytes(r.colour[0], LR.encode(oracle, m.rgb, 1), name)


def test_no_weight_no_highlight_whatever_the_shininess(lgs, kifs):
    scene = cases(kifs, W, H)["julia_24"]
    _setup(lgs, *scene)
    dull = dict(LR.A, specular=(0.0, 0.0, 0.0))
    a = _call(lgs, kifs, dict(dull, shininess_log2=10))
    b = _call(lgs, kifs, dict(dull, shininess_log2=0))
    shiny = _call(lgs, kifs, LR.A)
    assert a.st == OK and b.st == OK and shiny.st == OK
    _assert_bytes(a.colour[0], b.colour[0], "e = 10 against e = 0")
    assert (shiny.colour[0] != a.colour[0]).any()


def test_heatmap_colour_is_the_counters(lgs, kifs, oracle):
    screen, cam, gui, iters = cases(kifs, W, H)["julia_24"]
    heat = kifs.GuiData(**{**gui.__dict__, "is_heatmap": True, "fractal_color": (255, 128, 30)})
    scene = (screen, cam, heat, iters)
    _setup(lgs, *scene)
    r = _call(lgs, kifs, LR.A, ao=OR.DEFAULT)
    assert r.st == OK
    _assert_bytes(r.colour[0], lgs.render(), "plain heatmap render")
    m = _model(oracle, kifs, scene, "A", ao=OR.DEFAULT)
    _assert_bytes(r.colour[0], LR.encode(oracle, m.rgb, 1), "model")


@pytest.mark.parametrize("name", ["julia_24", "sierpinski"])
@pytest.mark.parametrize("k", [2, 3])
def test_supersampled_samples_are_lit_one_by_one(name, k, lgs, kifs, oracle):
    screen, cam, gui, iters = scene = cases(kifs, 70, 21)[name]
    _setup(lgs, *scene, k=k)
    try:
        r = _call(lgs, kifs, LR.A, ao=OR.DEFAULT)
    finally:
        lgs.set_supersampling(1)
    assert r.st == OK
    _assert_bytes(r.colour[0], LR.supersampled_bytes(oracle, kifs, screen, cam, gui, iters, LR.A, k, ao=OR.DEFAULT), (name, k))


def _lone(g, kifs, cam, **kw):
    g.set_camera(cam)
    r = _call(g, kifs, **kw)  # cameras NULL, count 1: the context's camera
    assert r.st == OK
    return r


def test_three_views_one_inside_the_bounding_sphere(lgs, kifs, oracle):
    screen, cam, gui, iters = scene = cases(kifs, W, H)["julia_24"]
    cams = [cam, kifs.CameraData(origin_distance=1.6, phi=2.0, theta=-0.3), kifs.CameraData(origin_distance=4.5, phi=4.0, theta=0.6)]
    _setup(lgs, *scene)
    r = _call(lgs, kifs, cams=cams, count=3)
    assert r.st == OK
    for i, c in enumerate(cams):
        _assert_bytes(r.colour[i], _lone(lgs, kifs, c).colour[0], ("view", i))
    m = _model(oracle, kifs, (screen, cams[1], gui, iters), "A")
    origin = np.array(list(cams[1].into_buffer_data().origin), dtype=np.float64)
    assert np.linalg.norm(origin) < 2.0 and m.hit.any() and not m.hit.all()  # (inside the bounding sphere: no ray is culled)
    _assert_bytes(r.colour[1], LR.encode(oracle, m.rgb, 1), "inside")
    # a one-frame batch with an explicit camera does not use the context's
    lgs.set_camera(cams[0])
    one = _call(lgs, kifs, cams=[cams[2]], count=1)
    _assert_bytes(one.colour[0], r.colour[2], "explicit camera")


def test_sixty_four_views_each_the_lone_call(lgs, kifs):
    screen, cam, gui, iters = cases(kifs, 40, 24)["julia_24"]
    cams = [kifs.CameraData(origin_distance=2.2 + 0.02 * i, phi=0.37 * i, theta=0.4 * np.sin(i)) for i in range(64)]
    _setup(lgs, screen, cams[0], gui, iters)
    r = _call(lgs, kifs, cams=cams, count=64)
    assert r.st == OK
    for i in (0, 1, 17, 31, 62, 63):
        _assert_bytes(r.colour[i], _lone(lgs, kifs, cams[i]).colour[0], ("view", i))
    assert len({r.colour[i].tobytes() for i in range(64)}) == 64


@pytest.mark.parametrize("name", ["julia_24", "torus"])
def test_band_equals_the_rows_of_the_full_frame(name, lgs, kifs, oracle):
    scene = cases(kifs, W, H)[name]
    _setup(lgs, *scene)
    m = _model(oracle, kifs, scene, "A", key=name)
    full = _call(lgs, kifs)
    band = _call(lgs, kifs, y0=5, y1=30)
    assert full.st == OK and band.st == OK and band.colour.shape[1] == 25
    _assert_bytes(band.colour[0], full.colour[0][5:30], name)
    _assert_bytes(band.colour[0], LR.encode(oracle, m.rgb, 1)[5:30], (name, "model"))
    empty = _call(lgs, kifs, y0=7, y1=7)
    assert empty.st == OK and empty.untouched()


# The edges of the ranges a light is accepted at, and a fourth light whose weights carry an infinite channel into the encode.
EDGES = [dict(LR.A, direction=(1.1e-19, 0.0, 0.0), shininess_log2=0),            # dot3 = 1.21e-38: the smallest normals
         dict(LR.A, direction=(1.0e19, -1.0e19, 1.0e19), shininess_log2=10),
         dict(LR.A, ambient=0.0, diffuse=0.0, specular=(3.0e38, 0.0, 0.0)),
         dict(LR.A, ambient=3.0e38, diffuse=3.0e38)]


@pytest.mark.parametrize("edge", range(len(EDGES)))
@pytest.mark.parametrize("name", ["julia_24", "torus"])
def test_accepted_edges_bit_exact(name, edge, lgs, kifs, oracle):
    """What the accepted edges write, not only that they are accepted: the model's bytes in both encodes."""
    screen, cam, gui, iters = scene = cases(kifs, W, H)[name]
    _setup(lgs, *scene)
    m = LR.lit_frame(oracle, kifs, screen, cam, gui, iters, EDGES[edge])
    assert m.hit.any() and not m.hit.all()
    print(name, edge, "hits", int(m.hit.sum()), "lit0 > 0:", int((m.hit & (m.lit0 > 0)).sum()), "lit0 = 1:", int((m.hit & (m.lit0 == 1)).sum()),
          "s > 0:", int((m.hit & (m.s > 0)).sum()), "non-finite channels:", int((~np.isfinite(m.rgb)).sum()))
    for encode in (1, 0):
        r = _call(lgs, kifs, spec=EDGES[edge], encode=encode)
        assert r.st == OK
        _assert_bytes(r.colour[0], LR.encode(oracle, m.rgb, encode), (name, edge, encode))


def _bad_lights():
    nan, inf = float("nan"), float("inf")
    good = dict(LR.A)
    bad = []
    for i in range(3):
        for v in (nan, inf, -inf):
            d = list(good["direction"])
            d[i] = v
            bad.append(dict(good, direction=tuple(d)))
        for v in (-1.0e-6, nan, inf):
            s = list(good["specular"])
            s[i] = v
            bad.append(dict(good, specular=tuple(s)))
    bad += [dict(good, direction=(0.0, 0.0, 0.0)), dict(good, direction=(0.0, -0.0, 0.0)),
            dict(good, direction=(1.0e-20, 1.0e-20, 0.0)),     # dot3 = 2e-40: subnormal
            dict(good, direction=(1.0e-30, 0.0, 1.0e-30)),     # dot3 underflows to zero
            dict(good, direction=(2.0e19, 2.0e19, 2.0e19))]    # dot3 overflows
    for field in ("ambient", "diffuse"):
        bad += [dict(good, **{field: v}) for v in (-1.0e-6, nan, inf, -inf)]
    bad += [dict(good, shininess_log2=v) for v in (-1, 11, 1 << 20, -(1 << 31))]
    return bad


def _bad_terms():
    from kifs_raymarching_amd._lib import AmbientOcclusionC as T
    nan, inf = float("nan"), float("inf")
    return [T(0, 0.02, 0.75, 4.0), T(17, 0.02, 0.75, 4.0), T(-1, 0.02, 0.75, 4.0),
            T(5, 0.0, 0.75, 4.0), T(5, -0.02, 0.75, 4.0), T(5, nan, 0.75, 4.0), T(5, inf, 0.75, 4.0),
            T(5, 0.02, 0.0, 4.0), T(5, 0.02, -0.5, 4.0), T(5, 0.02, 1.0000001, 4.0), T(5, 0.02, nan, 4.0), T(5, 0.02, inf, 4.0),
            T(5, 0.02, 0.75, -1.0e-6), T(5, 0.02, 0.75, nan), T(5, 0.02, 0.75, inf)]


def test_refusals_write_nothing(lgs, kifs):
    screen, cam, gui, iters = scene = cases(kifs, W, H)["torus"]
    _setup(lgs, *scene)
    two = [cam, cam]
    refusals = [dict(outs=None), dict(spec="null"), dict(count=0, cams=[]), dict(count=65, cams=[cam] * 65),
                dict(count=2, cams=None), dict(encode=2), dict(encode=-1),
                dict(y0=-1), dict(y1=H + 1), dict(y0=10, y1=9),
                dict(cams=two, count=2, null_out=1), dict(cams=two, count=2, misalign_out=1), dict(misalign_out=0)]
    refusals += [dict(spec=s) for s in _bad_lights()]
    refusals += [dict(term=t) for t in _bad_terms()]
    for kw in refusals:
        r = _call(lgs, kifs, **kw)
        assert r.st == BAD_ARG, (kw, r.st)
        assert r.untouched(), kw
    r = _call(lgs, kifs, ctx=None)
    assert r.st == BAD_ARG and r.untouched()
    for kw in (dict(cpad=-4), dict(cpad=2)):  # the colour pitch: as the batch call refuses it
        r = _call(lgs, kifs, **kw)
        assert r.st == BAD_SIZE and r.untouched(), kw
    # the edges of the ranges are accepted
    for s in EDGES[:3]:
        assert _call(lgs, kifs, spec=s).st == OK, s
    assert _call(lgs, kifs, cpad=0).st == OK


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


def test_the_python_layer_feeds_the_library_64_at_a_time(lgs, kifs):
    screen, cam, gui, iters = cases(kifs, 40, 24)["sierpinski"]
    cams = [kifs.CameraData(origin_distance=2.6 + 0.01 * i, phi=0.21 * i, theta=0.5 * np.cos(i)) for i in range(70)]
    _setup(lgs, screen, cams[0], gui, iters)
    light = kifs.Light(**LR.A)
    ao = kifs.AmbientOcclusion(samples=7, step=0.03, decay=0.8, strength=3.0)
    colour = lgs.render_lit_batch(cams, light, ao=ao)
    bare = lgs.render_lit_batch(cams, light)
    lgs.synchronize()
    assert tuple(colour.shape) == (70, 24, 40, 4) and tuple(bare.shape) == (70, 24, 40, 4)
    assert bool((bare != colour).any())
    colour = colour.cpu().numpy()
    for i, c in enumerate(cams):
        lgs.set_camera(c)
        _assert_bytes(colour[i], lgs.render_lit(light, ao=ao).cpu().numpy(), ("frame", i))
    one = _lone(lgs, kifs, cams[69], ao=(7, 0.03, 0.8, 3.0))  # ... which is the raw entry point's frame
    _assert_bytes(colour[69], one.colour[0], "raw")
    d = kifs.Light()
    assert (tuple(d.direction), d.ambient, d.diffuse, tuple(d.specular), d.shininess_log2) == ((1, 1, 1), 0.1, 0.9, (0, 0, 0), 5)
    lgs.set_camera(cams[3])
    _assert_bytes(lgs.render_lit(d).cpu().numpy(), lgs.render(), "Light() is the reference's light")


def _walk(kifs, screen, cam, gui, iters, with_call):
    """tests/test_gpu_occlusion.py's walk with the lit calls in the occlusion calls' place: 48-frame batch, lone render,
    [the lit calls], lone render, 48-frame batch on a fresh context, and what each left behind."""
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
            light = kifs.Light(**LR.A)
            before = (g.debug_last_kernel(), lib.kifs_debug_last_kernel(g._ctx), g.debug_last_round_steps(), g.debug_get_tile_order())
            colour = g.render_lit(light, ao=kifs.AmbientOcclusion())
            after = (g.debug_last_kernel(), lib.kifs_debug_last_kernel(g._ctx), g.debug_last_round_steps(), g.debug_get_tile_order())
            assert before[:3] == after[:3] and (before[3] == after[3]).all()
            assert bool((colour.cpu() != seen[1][0]).any())  # (the light does change this frame)
            batch3 = g.render_lit_batch(cams[:3], light, ao=kifs.AmbientOcclusion())
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
