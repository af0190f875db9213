"""Orbit-trap surface colouring on the GPU (kifs_render_trapped_async and kifs_eval_trap, kifs_trap_kernels.hip), bit for
bit: for every pipeline and both encodes the bytes equal the CPU restatement of the contract (tests/trap_reference.c, held
to the oracle and to the lighting model by tests/test_trap_reference.py, which also shows that the test traps colour these
frames), every u of kifs_eval_trap equals the model's, and with a flat gradient the bytes are those of the lit call, the
plain render and the occlusion call.  Bytes exactly, no tolerance, no excluded pixels: both sides run the contract's
operation sequence.  Frames are 102 x 45 unless said -- width no multiple of 32, height no multiple of 8 -- and every
destination is pre-filled with a sentinel and padded, so that a missing store and a store outside the frame both show."""
import ctypes as C

import numpy as np
import pytest

import lighting_reference as LR
import occlusion_reference as OR
import trap_reference as TR
from geometry_cases import PIPELINES, Raw, cases
from helpers import oracle_uniforms
from test_gpu_lighting import _call as lit_call
from test_gpu_lighting import _occlusion_bytes

pytestmark = pytest.mark.gpu

W, H = 102, 45
OK, BAD_SIZE, UNCONFIGURED, BAD_ARG = 0, 3, 4, 7
SENT_U8 = 0xA5
SHADOWS = dict(soft_shadow=True, shadow_steps=64, shadow_k=8.0, shadow_t0=0.02, shadow_max_t=10.0)


@pytest.fixture(scope="module")
def tgs(kifs):
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


def _ctrap(spec):
    from kifs_raymarching_amd._lib import KifsOrbitTrapC
    if isinstance(spec, KifsOrbitTrapC):
        return spec
    return KifsOrbitTrapC((C.c_float * 4)(*spec["centre"]), spec["axes"], spec["iterations"], spec["scale"], spec["bias"],
                          (C.c_float * 3)(*spec["mid"]), (C.c_float * 3)(*spec["far"]))


def _clight(spec):
    from kifs_raymarching_amd._lib import KifsLightC
    return KifsLightC((C.c_float * 3)(*spec["direction"]), spec["ambient"], spec["diffuse"], (C.c_float * 3)(*spec["specular"]),
                      spec["shininess_log2"])


def _call(g, kifs, trap=TR.J, spec=LR.A, ao=None, cams=None, count=1, y0=0, y1=None, encode=1, cpad=12, outs="given", ctx="given",
          null_out=None, misalign_out=None, term=None):
    """The raw entry point on sentinel-filled, padded destinations.  colour: (count, rows, W, 4) uint8.  The padding of
    every row and the tail of every destination are asserted to hold the sentinel after a call that succeeded.  `spec`
    None: a NULL light; `trap` None: a NULL trap."""
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
    record = None if trap is None else _ctrap(trap)
    light = None if spec is None else _clight(spec)
    t = term if term is not None else (None if ao is None else AmbientOcclusionC(int(ao[0]), float(ao[1]), float(ao[2]), float(ao[3])))
    st = lib.kifs_render_trapped_async(g._ctx if ctx == "given" else None, None, count, arr, ptrs if outs == "given" else None,
                                       cpitch, None if record is None else C.byref(record), None if light is None else C.byref(light),
                                       None if t is None else C.byref(t), y0, y1, encode)
    assert lib.kifs_synchronize(g._ctx) == 0
    chost = colour.cpu().numpy()
    if st != OK:
        return Result(st, None, chost)
    crows = chost[:, :rows * cpitch].reshape(count, rows, cpitch)
    assert (crows[:, :, 4 * w:] == SENT_U8).all() and (chost[:, rows * cpitch:] == SENT_U8).all(), "a colour store outside the frame"
    return Result(st, np.ascontiguousarray(crows[:, :, :4 * w]).reshape(count, rows, w, 4), chost)


def _ext(oracle, shadows):
    return oracle.Ext(1, 64, 8.0, 0.02, 10.0) if shadows else None


def _model(oracle, kifs, scene, trap, spec=LR.A, ao=None, shadows=False):
    screen, cam, gui, iters = scene
    return TR.trapped_frame(oracle, kifs, screen, cam, gui, iters, trap, spec, ao, _ext(oracle, shadows))


def _assert_bytes(got, want, what):
    bad = (got != want).any(-1)
    if bad.any():
        at = tuple(np.argwhere(bad)[0])
        pytest.fail(f"{what}: {int(bad.sum())} of {bad.size} pixels differ; first at {at}: got {got[at]}, want {want[at]}")


def _flat(trap):
    return dict(trap, scale=0.0, bias=0.0)


def _fractal_colour(kifs, gui):
    return tuple(float(v) for v in gui.into_buffer_data().fractal_color)


@pytest.mark.parametrize("name", PIPELINES)
@pytest.mark.parametrize("encode", [1, 0])
def test_every_pipeline_bit_exact(name, encode, tgs, kifs, oracle):
    scene = cases(kifs, W, H)[name]
    _setup(tgs, *scene)
    trap = TR.for_scene(name)
    m = _model(oracle, kifs, scene, trap)
    r = _call(tgs, kifs, trap, LR.A, encode=encode)
    assert r.st == OK
    t = m.t[m.hit]
    print(name, "hits", int(m.hit.sum()), "codes of t", len(np.unique(np.rint(255.0 * t.astype(np.float64)))), "upper segment", int((t >= 0.5).sum()))
    _assert_bytes(r.colour[0], TR.encode(oracle, m.rgb, encode), (name, encode))
    if name != "unknown_id":
        assert m.hit.any() and not m.hit.all()


EVAL_CENTRE = (0.1, -0.2, 0.3, 0.05)


@pytest.mark.parametrize("name", PIPELINES)
def test_eval_trap_every_bit(name, tgs, kifs, oracle):
    """2048 seeded points inside |p| < 1.5 per pipeline, K in {0, 1, 8, 32} x axes in {1, 6, 15}."""
    scene = cases(kifs, W, H)[name]
    _setup(tgs, *scene)
    _, _, o = oracle_uniforms(oracle, kifs, scene[:3])
    rng = np.random.default_rng([0x7a9, PIPELINES.index(name)])
    v = rng.normal(size=(2048, 3))
    pts = (v / np.linalg.norm(v, axis=1, keepdims=True) * (1.5 * rng.uniform(0.0, 1.0, (2048, 1)) ** (1.0 / 3.0))).astype(np.float32)
    assert (np.linalg.norm(pts.astype(np.float64), axis=1) < 1.5).all()
    for K in (0, 1, 8, 32):
        for axes in (1, 6, 15):
            spec = dict(TR.J, centre=EVAL_CENTRE, axes=axes, iterations=K)
            got = tgs.eval_trap(_ctrap(spec), pts)
            want = TR.eval_u(oracle, o, spec, pts)
            bad = ~TR.same_bits(got, want)
            assert not bad.any(), (name, K, axes, int(bad.sum()), pts[bad][0], got[bad][0], want[bad][0])
    # only centre, axes and iterations are read and validated
    from kifs_raymarching_amd._lib import lib
    odd = _ctrap(dict(TR.J, scale=float("nan"), bias=float("inf"), mid=(-1.0, 0.0, 0.0)))
    assert (tgs.eval_trap(odd, pts[:64]).view(np.uint32) == tgs.eval_trap(_ctrap(TR.J), pts[:64]).view(np.uint32)).all()
    u = np.zeros(4, dtype=np.float32)
    fp = lambda a: a.ctypes.data_as(C.POINTER(C.c_float))
    for bad_spec in (dict(TR.J, axes=0), dict(TR.J, axes=16), dict(TR.J, iterations=-1), dict(TR.J, iterations=33),
                     dict(TR.J, centre=(0.0, float("nan"), 0.0, 0.0))):
        rec = _ctrap(bad_spec)
        assert lib.kifs_eval_trap(tgs._ctx, C.byref(rec), fp(pts), 4, fp(u)) == BAD_ARG, bad_spec
    assert lib.kifs_eval_trap(tgs._ctx, None, fp(pts), 4, fp(u)) == BAD_ARG and (u == 0).all()


@pytest.mark.parametrize("shadows", [False, True])
@pytest.mark.parametrize("name", ["julia_24", "genjulia", "sierpinski", "sphere", "bunny"])
def test_a_flat_gradient_is_the_lit_the_plain_and_the_occlusion_call(name, shadows, tgs, kifs):
    """Identities (a) and (b)."""
    scene = cases(kifs, W, H)[name]
    _setup(tgs, *scene, shadows=shadows)
    trap = TR.for_scene(name)
    fc = _fractal_colour(kifs, scene[2])
    try:
        want_lit = lit_call(tgs, kifs, LR.A, ao=OR.DEFAULT)
        want_bare = lit_call(tgs, kifs, LR.A)
        want_plain = tgs.render()
        want_term = _occlusion_bytes(tgs, OR.DEFAULT)
        for what, t in (("a", _flat(trap)), ("b", dict(trap, mid=fc, far=fc))):
            got = _call(tgs, kifs, t, LR.A, ao=OR.DEFAULT)
            bare = _call(tgs, kifs, t, LR.A)
            null = _call(tgs, kifs, t, None)
            null_term = _call(tgs, kifs, t, None, ao=OR.DEFAULT)
            assert got.st == OK and bare.st == OK and null.st == OK and null_term.st == OK
            _assert_bytes(got.colour[0], want_lit.colour[0], (name, shadows, what, "kifs_render_lit_async with a term"))
            _assert_bytes(bare.colour[0], want_bare.colour[0], (name, shadows, what, "kifs_render_lit_async"))
            _assert_bytes(null.colour[0], want_plain, (name, shadows, what, "GraphicState.render"))
            _assert_bytes(null_term.colour[0], want_term, (name, shadows, what, "kifs_render_occlusion_async"))
        coloured = _call(tgs, kifs, trap, LR.A)
        assert (coloured.colour[0] != want_bare.colour[0]).any()  # (the trap does change this frame)
    finally:
        tgs.set_extensions(soft_shadow=False)


def test_identities_hold_in_heatmap_mode(tgs, kifs, oracle):
    screen, cam, gui, iters = cases(kifs, W, H)["julia_24"]
    heat = kifs.GuiData(**{**gui.__dict__, "is_heatmap": True, "fractal_color": (255, 128, 30)})
    scene = (screen, cam, heat, iters)
    _setup(tgs, *scene)
    want = tgs.render()
    for t in (_flat(TR.J), TR.J):  # no trap is evaluated: any trap writes the counter's colour
        r = _call(tgs, kifs, t, LR.A, ao=OR.DEFAULT)
        assert r.st == OK
        _assert_bytes(r.colour[0], want, "plain heatmap render")
    m = _model(oracle, kifs, scene, TR.J, LR.A, OR.DEFAULT)
    _assert_bytes(r.colour[0], TR.encode(oracle, m.rgb, 1), "model")


def test_identities_hold_supersampled(tgs, kifs):
    scene = cases(kifs, 70, 21)["julia_24"]
    _setup(tgs, *scene, k=2, shadows=True)
    fc = _fractal_colour(kifs, scene[2])
    try:
        want_lit = lit_call(tgs, kifs, LR.A, ao=OR.DEFAULT)
        want_plain = tgs.render()
        for t in (_flat(TR.J), dict(TR.J, mid=fc, far=fc)):
            got = _call(tgs, kifs, t, LR.A, ao=OR.DEFAULT)
            null = _call(tgs, kifs, t, None)
            assert got.st == OK and null.st == OK
            _assert_bytes(got.colour[0], want_lit.colour[0], "k = 2, kifs_render_lit_async")
            _assert_bytes(null.colour[0], want_plain, "k = 2, GraphicState.render")
    finally:
        tgs.set_supersampling(1)
        tgs.set_extensions(soft_shadow=False)


@pytest.mark.parametrize("name", ["julia_24", "sierpinski"])
def test_everything_at_once(name, tgs, kifs, oracle):
    """The trap, light A with the highlight at e = 5, shadows and the deep term."""
    scene = cases(kifs, W, H)[name]
    _setup(tgs, *scene, shadows=True)
    trap = TR.for_scene(name)
    try:
        r = _call(tgs, kifs, trap, LR.A5, ao=OR.DEEP)
    finally:
        tgs.set_extensions(soft_shadow=False)
    assert r.st == OK
    m = _model(oracle, kifs, scene, trap, LR.A5, OR.DEEP, shadows=True)
    assert (m.hit & (m.t > 0) & (m.t < 1)).sum() >= 20
    _assert_bytes(r.colour[0], TR.encode(oracle, m.rgb, 1), name)


@pytest.mark.parametrize("name", ["julia_24", "sierpinski"])
@pytest.mark.parametrize("k", [2, 3])
def test_supersampled_samples_are_coloured_one_by_one(name, k, tgs, kifs, oracle):
    screen, cam, gui, iters = scene = cases(kifs, 70, 21)[name]
    _setup(tgs, *scene, k=k)
    trap = TR.for_scene(name)
    try:
        r = _call(tgs, kifs, trap, LR.A, ao=OR.DEFAULT)
    finally:
        tgs.set_supersampling(1)
    assert r.st == OK
    _assert_bytes(r.colour[0], TR.supersampled_bytes(oracle, kifs, screen, cam, gui, iters, trap, k, LR.A, ao=OR.DEFAULT), (name, k))


def _lone(g, kifs, cam, **kw):
    g.set_camera(cam)
    r = _call(g, kifs, **kw)  # cameras NULL, count 1: the context's camera
    assert r.st == OK
    return r


def test_three_views_one_inside_the_bounding_sphere(tgs, kifs, oracle):
    screen, cam, gui, iters = scene = cases(kifs, W, H)["julia_24"]
    cams = [cam, kifs.CameraData(origin_distance=1.6, phi=2.0, theta=-0.3), kifs.CameraData(origin_distance=4.5, phi=4.0, theta=0.6)]
    _setup(tgs, *scene)
    r = _call(tgs, kifs, cams=cams, count=3)
    assert r.st == OK
    for i, c in enumerate(cams):
        _assert_bytes(r.colour[i], _lone(tgs, kifs, c).colour[0], ("view", i))
    m = _model(oracle, kifs, (screen, cams[1], gui, iters), TR.J)
    origin = np.array(list(cams[1].into_buffer_data().origin), dtype=np.float64)
    assert np.linalg.norm(origin) < 2.0 and m.hit.any() and not m.hit.all()  # (inside the bounding sphere: no ray is culled)
    _assert_bytes(r.colour[1], TR.encode(oracle, m.rgb, 1), "inside")
    # a one-frame batch with an explicit camera does not use the context's
    tgs.set_camera(cams[0])
    one = _call(tgs, kifs, cams=[cams[2]], count=1)
    _assert_bytes(one.colour[0], r.colour[2], "explicit camera")


def test_sixty_four_views_each_the_lone_call(tgs, kifs):
    screen, cam, gui, iters = cases(kifs, 40, 24)["julia_24"]
    cams = [kifs.CameraData(origin_distance=2.2 + 0.02 * i, phi=0.37 * i, theta=0.4 * np.sin(i)) for i in range(64)]
    _setup(tgs, screen, cams[0], gui, iters)
    r = _call(tgs, kifs, cams=cams, count=64)
    assert r.st == OK
    for i in (0, 1, 17, 31, 62, 63):
        _assert_bytes(r.colour[i], _lone(tgs, kifs, cams[i]).colour[0], ("view", i))
    assert len({r.colour[i].tobytes() for i in range(64)}) == 64


@pytest.mark.parametrize("name", ["julia_24", "sierpinski"])
def test_band_equals_the_rows_of_the_full_frame(name, tgs, kifs, oracle):
    scene = cases(kifs, W, H)[name]
    _setup(tgs, *scene)
    trap = TR.for_scene(name)
    m = _model(oracle, kifs, scene, trap)
    full = _call(tgs, kifs, trap)
    band = _call(tgs, kifs, trap, y0=5, y1=30)
    assert full.st == OK and band.st == OK and band.colour.shape[1] == 25
    _assert_bytes(band.colour[0], full.colour[0][5:30], name)
    _assert_bytes(band.colour[0], TR.encode(oracle, m.rgb, 1)[5:30], (name, "model"))
    empty = _call(tgs, kifs, trap, y0=7, y1=7)
    assert empty.st == OK and empty.untouched()


# The edges of what a trap is accepted at.
EDGES = [dict(TR.J, iterations=0), dict(TR.J, iterations=32),
         dict(TR.J, axes=8, centre=(0.0, 0.0, 0.0, 0.3), scale=4.0, bias=0.0),   # a single-axis trap on w
         dict(TR.J, scale=-TR.J["scale"], bias=1.5),                             # an inverted gradient
         dict(TR.J, bias=1.0), dict(TR.J, bias=7.5),                             # everything `far`
         dict(TR.J, centre=(1.0e30, 0.0, 0.0, 0.0)),                             # u overflows to +inf: t = 1
         dict(TR.J, mid=(0.0, 0.0, 0.0), far=(0.0, 0.0, 0.0))]


@pytest.mark.parametrize("edge", range(len(EDGES)))
@pytest.mark.parametrize("name", ["julia_24", "sierpinski"])
def test_accepted_edges_bit_exact(name, edge, tgs, kifs, oracle):
    """What the accepted edges write, not only that they are accepted: the model's bytes in both encodes."""
    scene = cases(kifs, W, H)[name]
    _setup(tgs, *scene)
    trap = EDGES[edge]
    m = _model(oracle, kifs, scene, trap)
    assert m.hit.any() and not m.hit.all()
    t = m.t[m.hit]
    print(name, edge, "hits", len(t), "t = 0:", int((t == 0).sum()), "t = 1:", int((t == 1).sum()), "u = inf:", int(np.isinf(m.u[m.hit]).sum()))
    if edge == 6:
        assert np.isinf(m.u[m.hit]).all() and (t == 1).all()
    if edge in (4, 5):
        assert (t == 1).all()
    for encode in (1, 0):
        r = _call(tgs, kifs, trap, encode=encode)
        assert r.st == OK
        _assert_bytes(r.colour[0], TR.encode(oracle, m.rgb, encode), (name, edge, encode))


# (draw 1's range saturates every hit of its scene, t is 0 or 1 at each of them; the other five leave hits inside the gradient)
FUZZ_SEEDS = [0x7a901, 0x7a902, 0x7a903, 0x7a904, 0x7a905, 0x7a906]
FUZZ_PIPELINES = ["julia_24", "julia_25", "genjulia", "sierpinski", "torus", "bunny"]


def _fuzz(kifs, index):
    """Scene, trap, light, term, shadows and encode of seeded draw `index`: one pipeline each, camera, constant, colours
    and every field of the trap drawn."""
    rng = np.random.default_rng(FUZZ_SEEDS[index])
    name = FUZZ_PIPELINES[index]
    screen, _, gui, iters = cases(kifs, 70, 37)[name]
    cam = kifs.CameraData(origin_distance=float(rng.uniform(2.4, 3.6)), phi=float(rng.uniform(0.0, 6.28)), theta=float(rng.uniform(-0.8, 0.8)))
    changes = dict(fractal_color=tuple(int(v) for v in rng.integers(0, 256, 3)), background_color=tuple(int(v) for v in rng.integers(0, 256, 3)))
    if name != "sierpinski" and name != "torus" and name != "bunny":
        changes["constant"] = tuple(float(c + rng.uniform(-0.05, 0.05)) for c in gui.constant)
    gui = kifs.GuiData(**{**gui.__dict__, **changes})
    lo = float(rng.uniform(0.0, 0.6))
    s, b = TR.trap_range(lo, lo + float(rng.uniform(0.3, 1.5)))
    trap = dict(centre=tuple(float(v) for v in rng.uniform(-1.0, 1.0, 4)), axes=int(rng.integers(1, 16)), iterations=int(rng.integers(0, 33)),
                scale=float(s), bias=float(b), mid=tuple(float(v) for v in rng.uniform(0.0, 1.5, 3)),
                far=tuple(float(v) for v in rng.uniform(0.0, 1.5, 3)))
    spec = dict(LR.A if index % 2 == 0 else LR.B, direction=LR._unit32(rng.normal(size=3)))
    ao = OR.DEFAULT if index % 3 != 1 else None
    return (screen, cam, gui, iters), trap, spec, ao, index % 2 == 1, int(index % 3 != 2)


@pytest.mark.parametrize("index", range(len(FUZZ_SEEDS)))
def test_seeded_scenes_and_traps(index, tgs, kifs, oracle):
    scene, trap, spec, ao, shadows, encode = _fuzz(kifs, index)
    _setup(tgs, *scene, shadows=shadows)
    try:
        r = _call(tgs, kifs, trap, spec, ao=ao, encode=encode, cpad=24)
    finally:
        tgs.set_extensions(soft_shadow=False)
    assert r.st == OK
    m = _model(oracle, kifs, scene, trap, spec, ao, shadows)
    print(index, FUZZ_PIPELINES[index], trap, "hits", int(m.hit.sum()), "0 < t < 1:", int((m.hit & (m.t > 0) & (m.t < 1)).sum()))
    _assert_bytes(r.colour[0], TR.encode(oracle, m.rgb, encode), (index, trap, spec, ao, shadows))


def _bad_traps():
    nan, inf = float("nan"), float("inf")
    good = dict(TR.J)
    bad = [dict(good, axes=0), dict(good, axes=16), dict(good, axes=0xffffffff), dict(good, iterations=-1), dict(good, iterations=33),
           dict(good, iterations=1 << 20)]
    for i in range(4):
        for v in (nan, inf, -inf):
            c = list(good["centre"])
            c[i] = v
            bad.append(dict(good, centre=tuple(c)))
    for field in ("scale", "bias"):
        bad += [dict(good, **{field: v}) for v in (nan, inf, -inf)]
    for field in ("mid", "far"):
        for i in range(3):
            for v in (-1.0e-6, nan, inf, -inf):
                c = list(good[field])
                c[i] = v
                bad.append(dict(good, **{field: tuple(c)}))
    return bad


def test_refusals_write_nothing(tgs, kifs):
    from test_gpu_lighting import _bad_lights, _bad_terms
    screen, cam, gui, iters = scene = cases(kifs, W, H)["torus"]
    _setup(tgs, *scene)
    two = [cam, cam]
    refusals = [dict(outs=None), dict(trap=None), dict(count=0, cams=[]), dict(count=65, cams=[cam] * 65),
                dict(count=2, cams=None), dict(encode=2), dict(encode=-1),
                dict(y0=-1), dict(y1=H + 1), dict(y0=10, y1=9),
                dict(cams=two, count=2, null_out=1), dict(cams=two, count=2, misalign_out=1), dict(misalign_out=0)]
    refusals += [dict(trap=t) for t in _bad_traps()]
    refusals += [dict(spec=s) for s in _bad_lights()]
    refusals += [dict(term=t) for t in _bad_terms()]
    for kw in refusals:
        r = _call(tgs, kifs, **kw)
        assert r.st == BAD_ARG, (kw, r.st)
        assert r.untouched(), kw
    r = _call(tgs, kifs, ctx=None)
    assert r.st == BAD_ARG and r.untouched()
    for kw in (dict(cpad=-4), dict(cpad=2)):  # the colour pitch: as the batch call refuses it
        r = _call(tgs, kifs, **kw)
        assert r.st == BAD_SIZE and r.untouched(), kw
    # the edges of the ranges are accepted, and so is a NULL light
    for t in EDGES:
        assert _call(tgs, kifs, trap=t).st == OK, t
    assert _call(tgs, kifs, cpad=0).st == OK and _call(tgs, kifs, spec=None).st == OK


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
            rec = _ctrap(TR.J)
            fp = lambda a: a.ctypes.data_as(C.POINTER(C.c_float))
            assert lib.kifs_eval_trap(bare, C.byref(rec), fp(p), 2, fp(u)) == UNCONFIGURED
        finally:
            g._ctx = keep
            lib.kifs_destroy(bare)
    finally:
        g.close()


def test_the_python_layer_feeds_the_library_64_at_a_time(tgs, kifs):
    screen, cam, gui, iters = cases(kifs, 40, 24)["sierpinski"]
    cams = [kifs.CameraData(origin_distance=2.6 + 0.01 * i, phi=0.21 * i, theta=0.5 * np.cos(i)) for i in range(70)]
    _setup(tgs, screen, cams[0], gui, iters)
    from kifs_raymarching_amd.configs import trap_range
    s, b = trap_range(0.0, 2.0)
    trap = kifs.OrbitTrap(centre=(1.0, 1.0, 1.0, 0.0), axes=7, iterations=6, scale=float(s), bias=float(b))
    light = kifs.Light(**LR.A)
    ao = kifs.AmbientOcclusion(samples=7, step=0.03, decay=0.8, strength=3.0)
    colour = tgs.render_trapped_batch(cams, trap, light=light, ao=ao)
    bare = tgs.render_trapped_batch(cams, trap)
    tgs.synchronize()
    assert tuple(colour.shape) == (70, 24, 40, 4) and tuple(bare.shape) == (70, 24, 40, 4)
    assert bool((bare != colour).any())
    colour = colour.cpu().numpy()
    for i, c in enumerate(cams):
        tgs.set_camera(c)
        _assert_bytes(colour[i], tgs.render_trapped(trap, light=light, ao=ao).cpu().numpy(), ("frame", i))
    one = _lone(tgs, kifs, cams[69], trap=trap.into_buffer_data(), ao=(7, 0.03, 0.8, 3.0))  # ... which is the raw entry point's frame
    _assert_bytes(colour[69], one.colour[0], "raw")
    tgs.set_camera(cams[3])
    flat = kifs.OrbitTrap(scale=0.0, bias=0.0)
    _assert_bytes(tgs.render_trapped(flat).cpu().numpy(), tgs.render(), "a flat gradient under the default light")


def _walk(kifs, screen, cam, gui, iters, with_call):
    """tests/test_gpu_lighting.py's walk with the trapped calls in the lit calls' place: 48-frame batch, lone render,
    [the trapped calls], lone render, 48-frame batch on a fresh context, and what each left behind."""
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
            trap, light = _ctrap(TR.J), kifs.Light(**LR.A)
            before = (g.debug_last_kernel(), lib.kifs_debug_last_kernel(g._ctx), g.debug_last_round_steps(), g.debug_get_tile_order())
            colour = g.render_trapped(trap, light=light, ao=kifs.AmbientOcclusion())
            after = (g.debug_last_kernel(), lib.kifs_debug_last_kernel(g._ctx), g.debug_last_round_steps(), g.debug_get_tile_order())
            assert before[:3] == after[:3] and (before[3] == after[3]).all()
            assert bool((colour.cpu() != seen[1][0]).any())  # (the trap does change this frame)
            batch3 = g.render_trapped_batch(cams[:3], trap, light=light, ao=kifs.AmbientOcclusion())
            g.synchronize()
            assert (g.debug_get_tile_order() == before[3]).all() and g.debug_last_kernel() == before[0]
            assert bool((batch3[0] == colour).all())  # (cams[0] is the context's camera)
            g.eval_trap(trap, np.zeros((5, 3), dtype=np.float32))
            assert (g.debug_get_tile_order() == before[3]).all() and g.debug_last_kernel() == before[0]
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
