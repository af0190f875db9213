"""Kaleidoscopic IFS scenes on the GPU (kifs_render_folded_async and kifs_eval_fold, kifs_fold_kernels.hip), bit for bit:
for every KIFS pipeline and both encodes the bytes equal the CPU restatement of the contract (tests/fold_reference.c, held
to the oracle and to the lighting model by tests/test_fold_reference.py, which also shows that the test systems fold these
frames), every estimate and normal of kifs_eval_fold equals the model's, with no iterations the bytes are those of the lit
call, the plain render and the occlusion call, and a scene that lies wholly outside the base primitive's bounding sphere
is not culled.  Bytes exactly, no tolerance, no excluded pixels: both sides run the contract's operation sequence.  Frames
are 102 x 45 unless said -- width no multiple of 32, height no multiple of 8 -- and every destination is pre-filled with a
sentinel and padded, so that a missing store and a store outside the frame both show."""
import ctypes as C

import numpy as np
import pytest

import fold_reference as FR
import lighting_reference as LR
import occlusion_reference as OR
from geometry_cases import PIPELINES, Raw, cases
from helpers import oracle_uniforms
from test_fold_reference import KIFS_PIPELINES, UNFOLDED
from test_gpu_lighting import _call as lit_call
from test_gpu_lighting import _occlusion_bytes

pytestmark = pytest.mark.gpu

W, H = 102, 45
OK, BAD_SIZE, UNCONFIGURED, BAD_ARG = 0, 3, 4, 7
SENT_U8 = 0xA5
SHADOWS = dict(soft_shadow=True, shadow_steps=64, shadow_k=8.0, shadow_t0=0.02, shadow_max_t=10.0)


@pytest.fixture(scope="module")
def fgs(kifs):
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


def _cfold(spec):
    from kifs_raymarching_amd._lib import KifsFoldSystemC
    if isinstance(spec, KifsFoldSystemC):
        return spec
    f = FR.fold(spec)
    return KifsFoldSystemC(f.stages, f.iterations, f.scale, (C.c_float * 3)(*f.offset), (C.c_float * 9)(*f.rotation))


def _clight(spec):
    from kifs_raymarching_amd._lib import KifsLightC
    return KifsLightC((C.c_float * 3)(*spec["direction"]), spec["ambient"], spec["diffuse"], (C.c_float * 3)(*spec["specular"]),
                      spec["shininess_log2"])


def _call(g, kifs, fold=FR.ALL_STAGES, spec=LR.A, ao=None, cams=None, count=1, y0=0, y1=None, encode=1, cpad=12, outs="given",
          ctx="given", null_out=None, misalign_out=None, term=None, stream=None):
    """The raw entry point on sentinel-filled, padded destinations.  colour: (count, rows, W, 4) uint8.  The padding of
    every row and the tail of every destination are asserted to hold the sentinel after a call that succeeded.  `spec`
    None: a NULL light; `fold` None: a NULL system."""
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
    record = None if fold is None else _cfold(fold)
    light = None if spec is None else _clight(spec)
    t = term if term is not None else (None if ao is None else AmbientOcclusionC(int(ao[0]), float(ao[1]), float(ao[2]), float(ao[3])))
    st = lib.kifs_render_folded_async(g._ctx if ctx == "given" else None, stream, count, arr, ptrs if outs == "given" else None,
                                      cpitch, None if record is None else C.byref(record), None if light is None else C.byref(light),
                                      None if t is None else C.byref(t), y0, y1, encode)
    torch.cuda.synchronize()
    assert lib.kifs_synchronize(g._ctx) == 0
    chost = colour.cpu().numpy()
    if st != OK:
        return Result(st, None, chost)
    crows = chost[:, :rows * cpitch].reshape(count, rows, cpitch)
    assert (crows[:, :, 4 * w:] == SENT_U8).all() and (chost[:, rows * cpitch:] == SENT_U8).all(), "a colour store outside the frame"
    return Result(st, np.ascontiguousarray(crows[:, :, :4 * w]).reshape(count, rows, w, 4), chost)


def _ext(oracle, shadows):
    return oracle.Ext(1, 64, 8.0, 0.02, 10.0) if shadows else None


def _model(oracle, kifs, scene, fold, spec=LR.A, ao=None, shadows=False):
    screen, cam, gui, iters = scene
    return FR.folded_frame(oracle, kifs, screen, cam, gui, iters, fold, spec, ao, _ext(oracle, shadows))


def _assert_bytes(got, want, what):
    bad = (got != want).any(-1)
    if bad.any():
        at = tuple(np.argwhere(bad)[0])
        pytest.fail(f"{what}: {int(bad.sum())} of {bad.size} pixels differ; first at {at}: got {got[at]}, want {want[at]}")


# ---- (a) every KIFS pipeline under the all-stages system
@pytest.mark.parametrize("name", KIFS_PIPELINES)
@pytest.mark.parametrize("encode", [1, 0])
def test_every_pipeline_bit_exact(name, encode, fgs, kifs, oracle):
    scene = cases(kifs, W, H)[name]
    _setup(fgs, *scene)
    m = _model(oracle, kifs, scene, FR.ALL_STAGES)
    r = _call(fgs, kifs, FR.ALL_STAGES, LR.A, encode=encode)
    assert r.st == OK
    print(name, "hits", int(m.hit.sum()))
    _assert_bytes(r.colour[0], FR.encode(oracle, m.rgb, encode), (name, encode))
    if name != "unknown_id":
        assert m.hit.any() and not m.hit.all()


# ---- (b) the named systems on their natural bases
@pytest.mark.parametrize("mode", ["shadows", "heatmap"])
@pytest.mark.parametrize("name", list(FR.NAMED))
def test_named_systems_bit_exact(name, mode, fgs, kifs, oracle):
    """Light A with its highlight and the default term, once with soft shadows and once as a heatmap."""
    (screen, cam, gui, iters), fold = FR.named_scene(kifs, cases, name, W, H)
    if mode == "heatmap":
        gui = kifs.GuiData(**{**gui.__dict__, "is_heatmap": True, "fractal_color": (255, 128, 30)})
    scene = (screen, cam, gui, iters)
    shadows = mode == "shadows"
    _setup(fgs, *scene, shadows=shadows)
    try:
        r = _call(fgs, kifs, fold, LR.A, ao=OR.DEFAULT)
    finally:
        fgs.set_extensions(soft_shadow=False)
    assert r.st == OK
    m = _model(oracle, kifs, scene, fold, LR.A, OR.DEFAULT, shadows)
    print(name, mode, "hits", int(m.hit.sum()))
    assert m.hit.sum() >= 100
    _assert_bytes(r.colour[0], FR.encode(oracle, m.rgb, 1), (name, mode))


# ---- (c) kifs_eval_fold
EVAL_SYSTEMS = [dict(stages=FR.ABS | FR.SORT | FR.MIRROR_Z, scale=3.0, offset=(1.0, 1.0, 1.0)),
                dict(stages=FR.TETRA | FR.ROTATE, scale=2.0, offset=(1.0, 1.0, 1.0), rotation=FR.TETRA_TORUS["rotation"]),
                dict(FR.ALL_STAGES, scale=1.7)]


@pytest.mark.parametrize("name", KIFS_PIPELINES)
def test_eval_fold_every_bit(name, fgs, kifs, oracle):
    """2048 seeded points inside |p| < 2.5 per pipeline, N in {0, 1, 7, 24} x three stage masks: every bit of every
    estimate and normal; N = 0 is kifs_eval_points."""
    scene = cases(kifs, W, H)[name]
    _setup(fgs, *scene)
    _, _, o = oracle_uniforms(oracle, kifs, scene[:3])
    it = oracle.iters(*scene[3])
    rng = np.random.default_rng([0xf01d, PIPELINES.index(name)])
    v = rng.normal(size=(2048, 3))
    pts = (v / np.linalg.norm(v, axis=1, keepdims=True) * (2.5 * rng.uniform(0.0, 1.0, (2048, 1)) ** (1.0 / 3.0))).astype(np.float32)
    assert (np.linalg.norm(pts.astype(np.float64), axis=1) < 2.5).all()
    for N in (0, 1, 7, 24):
        for system in EVAL_SYSTEMS:
            spec = dict(system, iterations=N)
            sdf, nrm = fgs.eval_fold(_cfold(spec), pts)
            want_sdf, want_nrm = FR.eval_points(oracle, o, it, spec, pts)
            bad = ~FR.same_bits(sdf, want_sdf)
            assert not bad.any(), (name, N, spec["stages"], "sdf", int(bad.sum()), pts[bad][0], sdf[bad][0], want_sdf[bad][0])
            bad = ~FR.same_bits(nrm, want_nrm).all(-1)
            assert not bad.any(), (name, N, spec["stages"], "normal", int(bad.sum()), pts[bad][0], nrm[bad][0], want_nrm[bad][0])
    plain_sdf, plain_nrm = np.zeros(2048, dtype=np.float32), np.zeros((2048, 3), dtype=np.float32)
    from kifs_raymarching_amd._lib import lib
    fp = lambda a: a.ctypes.data_as(C.POINTER(C.c_float))
    assert lib.kifs_eval_points(fgs._ctx, fp(pts), 2048, fp(plain_sdf), fp(plain_nrm)) == OK
    sdf, nrm = fgs.eval_fold(_cfold(UNFOLDED), pts)
    assert FR.same_bits(sdf, plain_sdf).all() and FR.same_bits(nrm, plain_nrm).all()
    # either output may be NULL
    only_sdf, none = fgs.eval_fold(_cfold(dict(EVAL_SYSTEMS[0], iterations=7)), pts[:300], normal=False)
    none2, only_nrm = fgs.eval_fold(_cfold(dict(EVAL_SYSTEMS[0], iterations=7)), pts[:300], sdf=False)
    both = fgs.eval_fold(_cfold(dict(EVAL_SYSTEMS[0], iterations=7)), pts[:300])
    assert none is None and none2 is None and FR.same_bits(only_sdf, both[0]).all() and FR.same_bits(only_nrm, both[1]).all()


def test_eval_fold_refusals(fgs, kifs):
    from kifs_raymarching_amd._lib import lib
    scene = cases(kifs, W, H)["torus"]
    _setup(fgs, *scene)
    pts = np.zeros(12, dtype=np.float32)
    u = np.zeros(4, dtype=np.float32)
    fp = lambda a: a.ctypes.data_as(C.POINTER(C.c_float))
    for bad in _bad_folds():
        rec = _cfold(bad)
        assert lib.kifs_eval_fold(fgs._ctx, C.byref(rec), fp(pts), 4, fp(u), None) == BAD_ARG, bad
    rec = _cfold(FR.MENGER)
    assert lib.kifs_eval_fold(fgs._ctx, None, fp(pts), 4, fp(u), None) == BAD_ARG
    assert lib.kifs_eval_fold(fgs._ctx, C.byref(rec), None, 4, fp(u), None) == BAD_ARG
    assert lib.kifs_eval_fold(fgs._ctx, C.byref(rec), fp(pts), -1, fp(u), None) == BAD_ARG
    assert lib.kifs_eval_fold(fgs._ctx, C.byref(rec), fp(pts), 0, fp(u), None) == OK
    assert lib.kifs_eval_fold(fgs._ctx, C.byref(rec), fp(pts), 4, None, None) == OK and (u == 0).all()
    julia = cases(kifs, W, H)["julia_24"]
    _setup(fgs, *julia)
    assert lib.kifs_eval_fold(fgs._ctx, C.byref(rec), fp(pts), 4, fp(u), None) == BAD_ARG and (u == 0).all()


# ---- (d) the identity
@pytest.mark.parametrize("shadows", [False, True])
@pytest.mark.parametrize("name", ["sphere", "sierpinski", "bunny"])
def test_no_iterations_is_the_lit_the_plain_and_the_occlusion_call(name, shadows, fgs, kifs):
    scene = cases(kifs, W, H)[name]
    _setup(fgs, *scene, shadows=shadows)
    try:
        want_lit = lit_call(fgs, kifs, LR.A, ao=OR.DEFAULT)
        want_bare = lit_call(fgs, kifs, LR.A)
        want_plain = fgs.render()
        want_term = _occlusion_bytes(fgs, OR.DEFAULT)
        got = _call(fgs, kifs, UNFOLDED, LR.A, ao=OR.DEFAULT)
        bare = _call(fgs, kifs, UNFOLDED, LR.A)
        null = _call(fgs, kifs, UNFOLDED, None)
        null_term = _call(fgs, kifs, UNFOLDED, None, ao=OR.DEFAULT)
        assert got.st == OK and bare.st == OK and null.st == OK and null_term.st == OK
        _assert_bytes(got.colour[0], want_lit.colour[0], (name, shadows, "kifs_render_lit_async with a term"))
        _assert_bytes(bare.colour[0], want_bare.colour[0], (name, shadows, "kifs_render_lit_async"))
        _assert_bytes(null.colour[0], want_plain, (name, shadows, "GraphicState.render"))
        _assert_bytes(null_term.colour[0], want_term, (name, shadows, "kifs_render_occlusion_async"))
        folded = _call(fgs, kifs, FR.ALL_STAGES, LR.A)
        assert (folded.colour[0] != want_bare.colour[0]).any()  # (the system does change this frame)
    finally:
        fgs.set_extensions(soft_shadow=False)


def test_the_identity_holds_supersampled_and_in_heatmap_mode(fgs, kifs):
    screen, cam, gui, iters = cases(kifs, 70, 21)["sierpinski"]
    _setup(fgs, screen, cam, gui, iters, k=2, shadows=True)
    try:
        want_lit = lit_call(fgs, kifs, LR.A, ao=OR.DEFAULT)
        want_plain = fgs.render()
        got = _call(fgs, kifs, UNFOLDED, LR.A, ao=OR.DEFAULT)
        null = _call(fgs, kifs, UNFOLDED, None)
        assert got.st == OK and null.st == OK
        _assert_bytes(got.colour[0], want_lit.colour[0], "k = 2, kifs_render_lit_async")
        _assert_bytes(null.colour[0], want_plain, "k = 2, GraphicState.render")
    finally:
        fgs.set_supersampling(1)
        fgs.set_extensions(soft_shadow=False)
    heat = kifs.GuiData(**{**gui.__dict__, "is_heatmap": True, "fractal_color": (255, 128, 30)})
    _setup(fgs, screen, cam, heat, iters)
    r = _call(fgs, kifs, UNFOLDED, LR.A, ao=OR.DEFAULT)
    assert r.st == OK
    _assert_bytes(r.colour[0], fgs.render(), "plain heatmap render")


# ---- (e) the wide system: nothing of the base primitive's cull is left on
def test_a_scene_outside_the_base_primitives_bounding_sphere_is_not_culled(fgs, kifs, oracle):
    scene, fold = FR.wide_scene(kifs, cases, W, H)
    _setup(fgs, *scene)
    m = _model(oracle, kifs, scene, fold)
    r = np.linalg.norm(m.pos[m.hit].astype(np.float64), axis=1)
    origin = list(scene[1].into_buffer_data().origin)
    outside = FR.closest_approach(origin, m.pos[m.hit]) > 1.2
    print("wide: hits", int(m.hit.sum()), "least |p|", r.min(), "hits whose ray stays outside radius 1.2:", int(outside.sum()))
    assert m.hit.sum() >= 20 and (r > 1.2).all() and outside.sum() >= 20
    for encode in (1, 0):
        got = _call(fgs, kifs, fold, LR.A, encode=encode)
        assert got.st == OK
        _assert_bytes(got.colour[0], FR.encode(oracle, m.rgb, encode), ("wide", encode))
    # ... where the plain render of the base, whose culls are on, shows the unit sphere
    assert (fgs.render() != got.colour[0]).any()


# ---- (f) bands, batches, supersampling, a caller's stream
def test_bands_equal_the_rows_of_the_full_frame(fgs, kifs, oracle):
    scene, fold = FR.named_scene(kifs, cases, "flake", W, H)
    _setup(fgs, *scene)
    m = _model(oracle, kifs, scene, fold, LR.A, OR.DEFAULT)
    want = FR.encode(oracle, m.rgb, 1)
    full = _call(fgs, kifs, fold, ao=OR.DEFAULT)
    assert full.st == OK
    _assert_bytes(full.colour[0], want, "frame")
    for y0, y1 in ((8, 29), (5, 45)):
        band = _call(fgs, kifs, fold, ao=OR.DEFAULT, y0=y0, y1=y1)
        assert band.st == OK and band.colour.shape[1] == y1 - y0
        _assert_bytes(band.colour[0], full.colour[0][y0:y1], (y0, y1))
    empty = _call(fgs, kifs, fold, y0=7, y1=7)
    assert empty.st == OK and empty.untouched()


def _lone(g, kifs, cam, **kw):
    g.set_camera(cam)
    r = _call(g, kifs, **kw)  # cameras NULL, count 1: the context's camera
    assert r.st == OK
    return r


def test_three_views_each_the_lone_call(fgs, kifs, oracle):
    (screen, cam, gui, iters), fold = FR.named_scene(kifs, cases, "tetra_torus", W, H)
    cams = [cam, kifs.CameraData(origin_distance=1.6, phi=2.0, theta=-0.3), kifs.CameraData(origin_distance=4.5, phi=4.0, theta=0.6)]
    _setup(fgs, screen, cam, gui, iters)
    r = _call(fgs, kifs, fold, cams=cams, count=3)
    assert r.st == OK
    for i, c in enumerate(cams):
        _assert_bytes(r.colour[i], _lone(fgs, kifs, c, fold=fold).colour[0], ("view", i))
    m = _model(oracle, kifs, (screen, cams[1], gui, iters), fold)
    assert m.hit.any() and not m.hit.all()
    _assert_bytes(r.colour[1], FR.encode(oracle, m.rgb, 1), "view 1, model")
    fgs.set_camera(cams[0])  # a one-frame batch with an explicit camera does not use the context's
    one = _call(fgs, kifs, fold, cams=[cams[2]], count=1)
    _assert_bytes(one.colour[0], r.colour[2], "explicit camera")


def test_sixty_four_views_each_the_lone_call(fgs, kifs):
    screen, _, gui, iters = cases(kifs, 40, 24)["box"]
    cams = [kifs.CameraData(origin_distance=2.4 + 0.02 * i, phi=0.37 * i, theta=0.4 * np.sin(i)) for i in range(64)]
    _setup(fgs, screen, cams[0], gui, iters)
    r = _call(fgs, kifs, FR.FLAKE, cams=cams, count=64)
    assert r.st == OK
    for i in (0, 1, 17, 31, 62, 63):
        _assert_bytes(r.colour[i], _lone(fgs, kifs, cams[i], fold=FR.FLAKE).colour[0], ("view", i))
    assert len({r.colour[i].tobytes() for i in range(64)}) == 64


@pytest.mark.parametrize("k", [1, 2, 3, 4])
def test_supersampled_samples_are_folded_one_by_one(k, fgs, kifs, oracle):
    (screen, cam, gui, iters), fold = FR.named_scene(kifs, cases, "tetra_sphere", 70, 21)
    _setup(fgs, screen, cam, gui, iters, k=k)
    try:
        r = _call(fgs, kifs, fold, LR.A, ao=OR.DEFAULT)
    finally:
        fgs.set_supersampling(1)
    assert r.st == OK
    _assert_bytes(r.colour[0], FR.supersampled_bytes(oracle, kifs, screen, cam, gui, iters, fold, k, LR.A, ao=OR.DEFAULT), k)


def test_a_launch_on_the_callers_stream(fgs, kifs):
    import torch
    scene, fold = FR.named_scene(kifs, cases, "flake", W, H)
    _setup(fgs, *scene)
    want = _call(fgs, kifs, fold)
    s = torch.cuda.Stream(device="cuda:0")
    got = _call(fgs, kifs, fold, stream=s.cuda_stream)
    assert want.st == OK and got.st == OK
    _assert_bytes(got.colour[0], want.colour[0], "caller's stream")


# ---- (g) refusals
def _bad_folds():
    nan, inf = float("nan"), float("inf")
    good = dict(FR.ALL_STAGES)
    bad = [dict(good, stages=32), dict(good, stages=0xffffffff), dict(good, iterations=-1), dict(good, iterations=25),
           dict(good, iterations=1 << 20), dict(good, scale=0.5), dict(good, scale=17.0), dict(good, scale=-2.0),
           dict(good, scale=nan), dict(good, scale=inf)]
    for i in range(3):
        for v in (nan, inf, -inf):
            c = list(good["offset"])
            c[i] = v
            bad.append(dict(good, offset=tuple(c)))
    for i in (0, 4, 8):
        for v in (nan, inf):
            m = list(good["rotation"])
            m[i] = v
            bad.append(dict(good, rotation=tuple(m)))  # (ALL_STAGES has ROTATE)
    return bad


def test_refusals_write_nothing(fgs, kifs):
    from test_gpu_lighting import _bad_lights, _bad_terms
    screen, cam, gui, iters = scene = cases(kifs, W, H)["torus"]
    _setup(fgs, *scene)
    two = [cam, cam]
    refusals = [dict(outs=None), dict(fold=None), dict(count=0, cams=[]), dict(count=65, cams=[cam] * 65),
                dict(count=2, cams=None), dict(encode=2), dict(encode=-1),
                dict(y0=-1), dict(y1=H + 1), dict(y0=10, y1=9),
                dict(cams=two, count=2, null_out=1), dict(cams=two, count=2, misalign_out=1), dict(misalign_out=0)]
    refusals += [dict(fold=f) for f in _bad_folds()]
    refusals += [dict(spec=s) for s in _bad_lights()]
    refusals += [dict(term=t) for t in _bad_terms()]
    for kw in refusals:
        r = _call(fgs, kifs, **kw)
        assert r.st == BAD_ARG, (kw, r.st)
        assert r.untouched(), kw
    r = _call(fgs, kifs, ctx=None)
    assert r.st == BAD_ARG and r.untouched()
    for kw in (dict(cpad=-4), dict(cpad=2)):  # the colour pitch: as the batch call refuses it
        r = _call(fgs, kifs, **kw)
        assert r.st == BAD_SIZE and r.untouched(), kw
    # the edges of the ranges are accepted, and so are a NULL light and a NaN in a matrix that the stages do not name
    nan_matrix = tuple([float("nan")] + list(FR.IDENTITY[1:]))
    for f in (dict(FR.ALL_STAGES, iterations=0), dict(FR.ALL_STAGES, iterations=24), dict(FR.ALL_STAGES, scale=1.0),
              dict(FR.ALL_STAGES, scale=16.0), dict(FR.ALL_STAGES, stages=0), dict(FR.ALL_STAGES, stages=31 & ~FR.ROTATE, rotation=nan_matrix)):
        assert _call(fgs, kifs, fold=f).st == OK, f
    assert _call(fgs, kifs, cpad=0).st == OK and _call(fgs, kifs, spec=None).st == OK
    # ... which then writes what the same system writes with a finite matrix
    a = _call(fgs, kifs, fold=dict(FR.ALL_STAGES, stages=31 & ~FR.ROTATE, rotation=nan_matrix))
    b = _call(fgs, kifs, fold=dict(FR.ALL_STAGES, stages=31 & ~FR.ROTATE))
    _assert_bytes(a.colour[0], b.colour[0], "a matrix that is not read")
    # the two Julia groups have no folded form
    for name in ("julia_24", "genjulia"):
        _setup(fgs, *cases(kifs, W, H)[name])
        r = _call(fgs, kifs)
        assert r.st == BAD_ARG and r.untouched(), name


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
            u = np.zeros(2, dtype=np.float32)
            p = np.zeros(6, dtype=np.float32)
            rec = _cfold(FR.MENGER)
            fp = lambda a: a.ctypes.data_as(C.POINTER(C.c_float))
            assert lib.kifs_eval_fold(bare, C.byref(rec), fp(p), 2, fp(u), None) == UNCONFIGURED
        finally:
            g._ctx = keep
            lib.kifs_destroy(bare)
    finally:
        g.close()


def test_the_python_layer_feeds_the_library_64_at_a_time(fgs, kifs):
    from kifs_raymarching_amd.configs import FOLD_PRESETS
    base, fold = FOLD_PRESETS["tetra"]
    screen, _, gui, iters = cases(kifs, 40, 24)["torus"]
    cams = [kifs.CameraData(origin_distance=2.6 + 0.01 * i, phi=0.21 * i, theta=0.5 * np.cos(i)) for i in range(70)]
    _setup(fgs, screen, cams[0], gui, iters)
    light = kifs.Light(**LR.A)
    ao = kifs.AmbientOcclusion(samples=7, step=0.03, decay=0.8, strength=3.0)
    colour = fgs.render_folded_batch(cams, fold, light=light, ao=ao)
    bare = fgs.render_folded_batch(cams, fold)
    fgs.synchronize()
    assert tuple(colour.shape) == (70, 24, 40, 4) and tuple(bare.shape) == (70, 24, 40, 4)
    assert bool((bare != colour).any())
    colour = colour.cpu().numpy()
    for i, c in enumerate(cams):
        fgs.set_camera(c)
        _assert_bytes(colour[i], fgs.render_folded(fold, light=light, ao=ao).cpu().numpy(), ("frame", i))
    one = _lone(fgs, kifs, cams[69], fold=fold.into_buffer_data(), ao=(7, 0.03, 0.8, 3.0))  # ... which is the raw entry point's frame
    _assert_bytes(colour[69], one.colour[0], "raw")
    fgs.set_camera(cams[3])
    _assert_bytes(fgs.render_folded(kifs.FoldSystem()).cpu().numpy(), fgs.render(), "no iterations under the default light")


def test_a_long_lived_context_does_not_notice_the_call(kifs):
    """512 x 256 Sierpinski: the debug values and the tile order are where the plain renders left them."""
    from kifs_raymarching_amd._lib import lib
    screen, cam, gui, iters = cases(kifs, 512, 256)["sierpinski"]
    with kifs.GraphicState(0, screen_data=screen, camera_data=cam, gui_data=gui) as g:
        g.set_iters(*iters)
        first = g.render().copy()
        before = (g.debug_last_kernel(), lib.kifs_debug_last_kernel(g._ctx), g.debug_last_round_steps(), g.debug_get_tile_order())
        fold = kifs.FoldSystem(stages=("tetra",), iterations=3)
        colour = g.render_folded(fold, light=kifs.Light(**LR.A), ao=kifs.AmbientOcclusion())
        g.render_folded_batch([cam, cam, cam], fold)
        g.synchronize()
        g.eval_fold(fold, np.zeros((5, 3), dtype=np.float32))
        after = (g.debug_last_kernel(), lib.kifs_debug_last_kernel(g._ctx), g.debug_last_round_steps(), g.debug_get_tile_order())
        assert before[:3] == after[:3] and (before[3] == after[3]).all()
        assert bool((colour.cpu().numpy() != first).any())
        assert (g.render() == first).all()
