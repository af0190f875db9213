"""Orbit-trap colouring of folded scenes on the GPU (kifs_render_folded_trapped_async and kifs_eval_fold_trap,
kifs_fold_trap_kernels.hip), bit for bit: the bytes and every f32 of the plane of u equal the CPU restatement of the
contract (tests/fold_trap_reference.c, held to the folded and the trapped model by tests/test_fold_trap_reference.py, which
also shows that these frames and evaluation cases exercise the orbit), every u of kifs_eval_fold_trap equals the model's,
a neutral trap writes the folded call's bytes and no iterations of the fold write the trapped call's, and the record that
carries the fold system and the trap survives more calls in flight than its ring is deep.  Bytes exactly, no tolerance, no
excluded pixels.  Frames are 102 x 45 unless said -- width no multiple of 32, height no multiple of 8 -- and every
destination and plane is pre-filled with a sentinel and padded, so that a missing store and a store outside the frame both
show."""
import ctypes as C

import numpy as np
import pytest

import fold_reference as FR
import fold_trap_reference as FT
import lighting_reference as LR
import occlusion_reference as OR
import trap_reference as TR
from geometry_cases import Raw, cases
from helpers import oracle_uniforms
from test_fold_reference import KIFS_PIPELINES, UNFOLDED
from test_gpu_fold import _bad_folds, _cfold, _clight
from test_gpu_fold import _call as folded_call
from test_gpu_lighting import _occlusion_bytes
from test_gpu_trap import _bad_traps, _ctrap
from test_gpu_trap import _call as trapped_call

pytestmark = pytest.mark.gpu

W, H = 102, 45
OK, BAD_SIZE, UNCONFIGURED, BAD_ARG = 0, 3, 4, 7
SENT_U8 = 0xA5
SHADOWS = dict(soft_shadow=True, shadow_steps=64, shadow_k=8.0, shadow_t0=0.02, shadow_max_t=10.0)
NEUTRAL = dict(FT.POINT8, scale=0.0, bias=0.0)


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


class Pending:
    """A call that has been enqueued: its status and the device buffers it writes."""

    def __init__(self, st, colour, plane, shape):
        self.st, self.colour, self.plane, self.shape = st, colour, plane, shape


class Result:
    def __init__(self, st, colour, colour_raw, plane, plane_raw):
        self.st, self.colour, self.colour_raw, self.plane, self.plane_raw = st, colour, colour_raw, plane, plane_raw

    def untouched(self):
        return (self.colour_raw == SENT_U8).all() and (self.plane_raw is None or (self.plane_raw == SENT_U8).all())


def _enqueue(g, kifs, fold=FR.ALL_STAGES, trap=FT.POINT8, spec=LR.A, ao=None, cams=None, count=1, y0=0, y1=None, encode=1, cpad=12,
             outs="given", ctx="given", null_out=None, misalign_out=None, term=None, stream=None, plane=False, ppad=8, pstride=None,
             plane_offset=0, buffers=None):
    """The raw entry point on sentinel-filled, padded destinations, not waited for.  `spec` None: a NULL light; `fold` /
    `trap` None: a NULL record; `plane`: with a plane of u, rows ppad bytes apart beyond the frame's width; `buffers`: the
    pair (colour, plane) of sentinel-filled tensors that have settled -- then nothing here waits for the device."""
    import torch
    from kifs_raymarching_amd._lib import AmbientOcclusionC, lib
    w, h = g.screen_data.width, g.screen_data.height
    y1 = h if y1 is None else y1
    rows = max(y1 - y0, 0)
    cpitch, ppitch = 4 * w + cpad, 4 * w + ppad
    if buffers is None:
        colour = torch.full((count, rows * cpitch + 64), SENT_U8, dtype=torch.uint8, device="cuda:0")
        pbuf = torch.full((count, rows * ppitch + 64), SENT_U8, dtype=torch.uint8, device="cuda:0") if plane else None
        torch.cuda.synchronize()
    else:
        colour, pbuf = buffers
    ptrs = (C.c_void_p * count)(*[colour[i].data_ptr() for i in range(count)])
    if null_out is not None:
        ptrs[null_out] = None
    if misalign_out is not None:
        ptrs[misalign_out] = colour[misalign_out].data_ptr() + 2
    arr = None if cams is None else kifs.camera_array(cams)
    system = None if fold is None else _cfold(fold)
    record = None if trap is None else _ctrap(trap)
    light = None if spec is None else _clight(spec)
    t = term if term is not None else (None if ao is None else AmbientOcclusionC(int(ao[0]), float(ao[1]), float(ao[2]), float(ao[3])))
    st = lib.kifs_render_folded_trapped_async(
        g._ctx if ctx == "given" else None, stream, count, arr, ptrs if outs == "given" else None, cpitch,
        None if system is None else C.byref(system), None if record is None else C.byref(record), None if light is None else C.byref(light),
        None if t is None else C.byref(t), None if pbuf is None else pbuf.data_ptr() + plane_offset, ppitch,
        (rows * ppitch + 64) if pstride is None else pstride, y0, y1, encode)
    return Pending(st, colour, pbuf, (count, rows, w, cpitch, ppitch))


def _collect(p):
    """The frames (count, rows, W, 4) uint8 and the plane's bits (count, rows, W) uint32 of a call that is over.  The
    padding of every row and the tail of every buffer are asserted to hold the sentinel after a call that succeeded."""
    count, rows, w, cpitch, ppitch = p.shape
    chost = p.colour.cpu().numpy()
    phost = None if p.plane is None else p.plane.cpu().numpy()
    if p.st != OK:
        return Result(p.st, None, chost, None, phost)
    crows = chost[:, :rows * cpitch].reshape(count, rows, cpitch)
    assert (crows[:, :, 4 * w:] == SENT_U8).all() and (chost[:, rows * cpitch:] == SENT_U8).all(), "a colour store outside the frame"
    bits = None
    if phost is not None:
        prows = phost[:, :rows * ppitch].reshape(count, rows, ppitch)
        assert (prows[:, :, 4 * w:] == SENT_U8).all() and (phost[:, rows * ppitch:] == SENT_U8).all(), "a plane store outside the frame"
        bits = np.ascontiguousarray(prows[:, :, :4 * w]).view(np.uint32).reshape(count, rows, w)
    return Result(p.st, np.ascontiguousarray(crows[:, :, :4 * w]).reshape(count, rows, w, 4), chost, bits, phost)


def _call(g, kifs, **kw):
    import torch
    from kifs_raymarching_amd._lib import lib
    p = _enqueue(g, kifs, **kw)
    torch.cuda.synchronize()
    assert lib.kifs_synchronize(g._ctx) == 0
    return _collect(p)


def _ext(oracle, shadows):
    return oracle.Ext(1, 64, 8.0, 0.02, 10.0) if shadows else None


def _model(oracle, kifs, scene, fold, trap, spec=LR.A, ao=None, shadows=False):
    screen, cam, gui, iters = scene
    return FT.frame(oracle, kifs, screen, cam, gui, iters, fold, trap, spec, ao, _ext(oracle, shadows))


def _assert_bytes(got, want, what):
    bad = (got != want).any(-1)
    if bad.any():
        at = tuple(np.argwhere(bad)[0])
        pytest.fail(f"{what}: {int(bad.sum())} of {bad.size} pixels differ; first at {at}: got {got[at]}, want {want[at]}")


def _assert_plane(bits, u, what):
    want = np.ascontiguousarray(u, dtype=np.float32).view(np.uint32)
    bad = bits != want
    if bad.any():
        at = tuple(np.argwhere(bad)[0])
        pytest.fail(f"{what}: {int(bad.sum())} of {bad.size} values of the plane differ; first at {at}: got {bits[at]:#x}, want {want[at]:#x}")


def _heat(kifs, gui):
    return kifs.GuiData(**{**gui.__dict__, "is_heatmap": True, "fractal_color": (255, 128, 30)})


def _fractal_colour(gui):
    return tuple(float(v) for v in gui.into_buffer_data().fractal_color)


# ---- (a) bytes against the model
@pytest.mark.parametrize("name", KIFS_PIPELINES)
@pytest.mark.parametrize("encode", [1, 0])
def test_every_pipeline_bit_exact(name, encode, fgs, kifs, oracle):
    scene = cases(kifs, W, H)[name]
    _setup(fgs, *scene)
    m = _model(oracle, kifs, scene, FR.ALL_STAGES, FT.POINT8)
    r = _call(fgs, kifs, encode=encode)
    assert r.st == OK
    print(name, "hits", int(m.hit.sum()))
    _assert_bytes(r.colour[0], FT.encode(oracle, m.rgb, encode), (name, encode))
    if name != "unknown_id":
        assert m.hit.any() and not m.hit.all()


@pytest.mark.parametrize("name", list(FT.NAMED))
def test_named_frames_with_soft_shadows_bit_exact(name, fgs, kifs, oracle):
    """Light A with its highlight and the default term, soft shadows on; the trap's range is the model's own."""
    scene, fold, trap = FT.named_scene(oracle, kifs, cases, name, W, H)
    _setup(fgs, *scene, shadows=True)
    try:
        r = _call(fgs, kifs, fold=fold, trap=trap, ao=OR.DEFAULT)
    finally:
        fgs.set_extensions(soft_shadow=False)
    assert r.st == OK
    m = _model(oracle, kifs, scene, fold, trap, LR.A, OR.DEFAULT, True)
    assert m.hit.sum() >= 100
    _assert_bytes(r.colour[0], FT.encode(oracle, m.rgb, 1), name)


def test_a_heatmap_frame_is_the_folded_calls(fgs, kifs, oracle):
    (screen, cam, gui, iters), fold, trap = FT.named_scene(oracle, kifs, cases, "flake", W, H)
    scene = (screen, cam, _heat(kifs, gui), iters)
    _setup(fgs, *scene)
    r = _call(fgs, kifs, fold=fold, trap=trap, ao=OR.DEFAULT)
    assert r.st == OK
    m = _model(oracle, kifs, scene, fold, trap, LR.A, OR.DEFAULT)
    _assert_bytes(r.colour[0], FT.encode(oracle, m.rgb, 1), "model")
    _assert_bytes(r.colour[0], folded_call(fgs, kifs, fold, LR.A, ao=OR.DEFAULT).colour[0], "kifs_render_folded_async")


# ---- (b) the plane of u
@pytest.mark.parametrize("mode", ["bare", "term", "heatmap"])
def test_the_plane_holds_every_hits_u_and_inf_on_a_miss(mode, fgs, kifs, oracle):
    (screen, cam, gui, iters), fold, trap = FT.named_scene(oracle, kifs, cases, "flake", W, H)
    scene = (screen, cam, _heat(kifs, gui) if mode == "heatmap" else gui, iters)
    ao = OR.DEFAULT if mode == "term" else None
    _setup(fgs, *scene)
    m = _model(oracle, kifs, scene, fold, trap, LR.A, ao)
    r = _call(fgs, kifs, fold=fold, trap=trap, ao=ao, plane=True)
    assert r.st == OK
    _assert_bytes(r.colour[0], FT.encode(oracle, m.rgb, 1), mode)
    _assert_plane(r.plane[0], m.u, mode)
    got = r.plane[0].view(np.float32)
    assert m.hit.sum() >= 100 and (~m.hit).sum() >= 100
    assert np.isposinf(got[~m.hit]).all() and np.isfinite(got[m.hit]).all()
    # identity (c): the plane at a hit pixel is kifs_eval_fold_trap at the model's hit position
    u = fgs.eval_fold_trap(_cfold(fold), _ctrap(trap), m.pos[m.hit])
    assert FT.same_bits(u, got[m.hit]).all()
    # ... and the colour does not depend on the plane
    _assert_bytes(_call(fgs, kifs, fold=fold, trap=trap, ao=ao).colour[0], r.colour[0], "without a plane")


# ---- (c) kifs_eval_fold_trap
@pytest.mark.parametrize("name", FT.EVAL_PIPELINES)
def test_eval_fold_trap_every_bit(name, fgs, kifs, oracle):
    """2048 seeded points per case, N in {0, 1, 7, 24} x K in {0, 1, 8, 32} x three stage masks x three trap kinds, with
    a max_distance that cuts orbits (tests/test_fold_trap_reference.py counts them): every bit of every u."""
    scene = FT.eval_scene(kifs, cases, name)
    _setup(fgs, *scene)
    _, _, o = oracle_uniforms(oracle, kifs, scene[:3])
    pts = FT.eval_points(name)
    for fold, trap in FT.eval_cases():
        u = fgs.eval_fold_trap(_cfold(fold), _ctrap(trap), pts)
        want = FT.eval_u(oracle, o, fold, trap, pts)
        bad = ~FT.same_bits(u, want)
        assert not bad.any(), (name, fold["iterations"], trap["iterations"], fold["stages"], trap["axes"], int(bad.sum()), pts[bad][0],
                               u[bad][0], want[bad][0])
    # identity (b): with no iterations of the fold, kifs_eval_trap's values
    for K in (0, 6, 32):
        trap = dict(TR.S, iterations=K)
        assert FT.same_bits(fgs.eval_fold_trap(_cfold(UNFOLDED), _ctrap(trap), pts), fgs.eval_trap(_ctrap(trap), pts)).all(), (name, K)


def test_eval_fold_trap_refusals(fgs, kifs):
    from kifs_raymarching_amd._lib import lib
    _setup(fgs, *cases(kifs, W, H)["torus"])
    pts = np.zeros(12, dtype=np.float32)
    u = np.zeros(4, dtype=np.float32)
    fp = lambda a: a.ctypes.data_as(C.POINTER(C.c_float))
    good_f, good_t = _cfold(FR.MENGER), _ctrap(FT.POINT8)
    for bad in _bad_folds():
        rec = _cfold(bad)
        assert lib.kifs_eval_fold_trap(fgs._ctx, C.byref(rec), C.byref(good_t), fp(pts), 4, fp(u)) == BAD_ARG, bad
    for bad in _bad_traps():
        rec = _ctrap(bad)
        orbit = any(bad[f] != TR.J[f] for f in ("centre", "axes", "iterations"))  # only these are validated
        assert lib.kifs_eval_fold_trap(fgs._ctx, C.byref(good_f), C.byref(rec), fp(pts), 4, fp(u)) == (BAD_ARG if orbit else OK), bad
    u[:] = 0
    assert lib.kifs_eval_fold_trap(fgs._ctx, None, C.byref(good_t), fp(pts), 4, fp(u)) == BAD_ARG
    assert lib.kifs_eval_fold_trap(fgs._ctx, C.byref(good_f), None, fp(pts), 4, fp(u)) == BAD_ARG
    assert lib.kifs_eval_fold_trap(fgs._ctx, C.byref(good_f), C.byref(good_t), None, 4, fp(u)) == BAD_ARG
    assert lib.kifs_eval_fold_trap(fgs._ctx, C.byref(good_f), C.byref(good_t), fp(pts), 4, None) == BAD_ARG
    assert lib.kifs_eval_fold_trap(fgs._ctx, C.byref(good_f), C.byref(good_t), fp(pts), -1, fp(u)) == BAD_ARG
    assert lib.kifs_eval_fold_trap(fgs._ctx, C.byref(good_f), C.byref(good_t), fp(pts), 0, fp(u)) == OK
    _setup(fgs, *cases(kifs, W, H)["julia_24"])
    assert lib.kifs_eval_fold_trap(fgs._ctx, C.byref(good_f), C.byref(good_t), fp(pts), 4, fp(u)) == BAD_ARG and (u == 0).all()


# ---- (d) the identities
@pytest.mark.parametrize("shadows", [False, True])
@pytest.mark.parametrize("name", ["sphere", "sierpinski", "bunny"])
def test_a_neutral_trap_is_the_folded_call_and_no_iterations_are_the_trapped_call(name, shadows, fgs, kifs):
    screen, cam, gui, iters = scene = cases(kifs, W, H)[name]
    _setup(fgs, *scene, shadows=shadows)
    fc = _fractal_colour(gui)
    try:
        # (a) against kifs_render_folded_async
        want = folded_call(fgs, kifs, FR.ALL_STAGES, LR.A, ao=OR.DEFAULT)
        for trap in (NEUTRAL, dict(FT.POINT8, mid=fc, far=fc)):
            got = _call(fgs, kifs, trap=trap, ao=OR.DEFAULT)
            assert got.st == OK
            _assert_bytes(got.colour[0], want.colour[0], (name, shadows, "kifs_render_folded_async", trap["scale"]))
        coloured = _call(fgs, kifs, ao=OR.DEFAULT)
        assert (coloured.colour[0] != want.colour[0]).any()  # (the trap does change this frame)
        # (b) against kifs_render_trapped_async
        want = trapped_call(fgs, kifs, TR.S, LR.A, ao=OR.DEFAULT)
        got = _call(fgs, kifs, fold=UNFOLDED, trap=TR.S, ao=OR.DEFAULT)
        assert got.st == OK
        _assert_bytes(got.colour[0], want.colour[0], (name, shadows, "kifs_render_trapped_async"))
        # ... and with a NULL light and a neutral trap against the plain render and the occlusion call
        null = _call(fgs, kifs, fold=UNFOLDED, trap=NEUTRAL, spec=None)
        null_term = _call(fgs, kifs, fold=UNFOLDED, trap=NEUTRAL, spec=None, ao=OR.DEFAULT)
        _assert_bytes(null.colour[0], fgs.render(), (name, shadows, "GraphicState.render"))
        _assert_bytes(null_term.colour[0], _occlusion_bytes(fgs, OR.DEFAULT), (name, shadows, "kifs_render_occlusion_async"))
    finally:
        fgs.set_extensions(soft_shadow=False)


def test_the_identities_hold_supersampled_and_in_heatmap_mode(fgs, kifs):
    screen, cam, gui, iters = cases(kifs, 70, 21)["sierpinski"]
    _setup(fgs, screen, cam, gui, iters, k=2, shadows=True)
    try:
        _assert_bytes(_call(fgs, kifs, trap=NEUTRAL, ao=OR.DEFAULT).colour[0],
                      folded_call(fgs, kifs, FR.ALL_STAGES, LR.A, ao=OR.DEFAULT).colour[0], "k = 2, kifs_render_folded_async")
        _assert_bytes(_call(fgs, kifs, fold=UNFOLDED, trap=TR.S, ao=OR.DEFAULT).colour[0],
                      trapped_call(fgs, kifs, TR.S, LR.A, ao=OR.DEFAULT).colour[0], "k = 2, kifs_render_trapped_async")
    finally:
        fgs.set_supersampling(1)
        fgs.set_extensions(soft_shadow=False)
    _setup(fgs, screen, cam, _heat(kifs, gui), iters)
    _assert_bytes(_call(fgs, kifs, ao=OR.DEFAULT).colour[0], folded_call(fgs, kifs, FR.ALL_STAGES, LR.A, ao=OR.DEFAULT).colour[0],
                  "heatmap, kifs_render_folded_async")
    _assert_bytes(_call(fgs, kifs, fold=UNFOLDED, trap=TR.S, ao=OR.DEFAULT).colour[0],
                  trapped_call(fgs, kifs, TR.S, LR.A, ao=OR.DEFAULT).colour[0], "heatmap, kifs_render_trapped_async")


def test_a_scene_outside_the_base_primitives_bounding_sphere_is_not_culled(fgs, kifs, oracle):
    """The two balls of the folded tests with a trap: the rays that stay outside the unit sphere's cull radius are hits."""
    scene, fold = FR.wide_scene(kifs, cases, W, H)
    _setup(fgs, *scene)
    trap = dict(centre=(1.5, 0.0, 0.0, 0.0), axes=15, iterations=1, scale=2.0, bias=0.0, mid=TR.MID, far=TR.FAR)
    m = _model(oracle, kifs, scene, fold, trap)
    origin = list(scene[1].into_buffer_data().origin)
    outside = FR.closest_approach(origin, m.pos[m.hit]) > 1.2
    print("wide: hits", int(m.hit.sum()), "hits whose ray stays outside radius 1.2:", int(outside.sum()))
    assert outside.sum() >= 20
    got = _call(fgs, kifs, fold=fold, trap=trap, plane=True)
    assert got.st == OK
    _assert_bytes(got.colour[0], FT.encode(oracle, m.rgb, 1), "wide")
    _assert_plane(got.plane[0], m.u, "wide")
    assert (got.colour[0] != folded_call(fgs, kifs, fold, LR.A).colour[0]).any()


# ---- (e) bands, batches, supersampling, a caller's stream
def test_bands_equal_the_rows_of_the_full_frame(fgs, kifs, oracle):
    scene, fold, trap = FT.named_scene(oracle, kifs, cases, "flake", W, H)
    _setup(fgs, *scene)
    m = _model(oracle, kifs, scene, fold, trap, LR.A, OR.DEFAULT)
    full = _call(fgs, kifs, fold=fold, trap=trap, ao=OR.DEFAULT, plane=True)
    assert full.st == OK
    _assert_bytes(full.colour[0], FT.encode(oracle, m.rgb, 1), "frame")
    for y0, y1 in ((8, 29), (5, 45)):
        band = _call(fgs, kifs, fold=fold, trap=trap, ao=OR.DEFAULT, y0=y0, y1=y1, plane=True)
        assert band.st == OK and band.colour.shape[1] == y1 - y0
        _assert_bytes(band.colour[0], full.colour[0][y0:y1], (y0, y1))
        assert (band.plane[0] == full.plane[0][y0:y1]).all(), (y0, y1)
    empty = _call(fgs, kifs, fold=fold, trap=trap, y0=7, y1=7, plane=True)
    assert empty.st == OK and empty.untouched()


def _lone(g, kifs, cam, **kw):
    g.set_camera(cam)
    r = _call(g, kifs, **kw)  # cameras NULL, count 1: the context's camera
    assert r.st == OK
    return r


def test_three_views_each_the_lone_call(fgs, kifs, oracle):
    (screen, cam, gui, iters), fold, trap = FT.named_scene(oracle, kifs, cases, "tetra_torus", W, H)
    cams = [cam, kifs.CameraData(origin_distance=1.6, phi=2.0, theta=-0.3), kifs.CameraData(origin_distance=4.5, phi=4.0, theta=0.6)]
    _setup(fgs, screen, cam, gui, iters)
    r = _call(fgs, kifs, fold=fold, trap=trap, cams=cams, count=3, plane=True)
    assert r.st == OK
    for i, c in enumerate(cams):
        lone = _lone(fgs, kifs, c, fold=fold, trap=trap, plane=True)
        _assert_bytes(r.colour[i], lone.colour[0], ("view", i))
        assert (r.plane[i] == lone.plane[0]).all(), ("plane of view", i)
    m = _model(oracle, kifs, (screen, cams[1], gui, iters), fold, trap)
    assert m.hit.any() and not m.hit.all()
    _assert_bytes(r.colour[1], FT.encode(oracle, m.rgb, 1), "view 1, model")
    _assert_plane(r.plane[1], m.u, "view 1, model")


def test_sixty_four_views_each_the_lone_call(fgs, kifs):
    screen, _, gui, iters = cases(kifs, 34, 9)["box"]
    cams = [kifs.CameraData(origin_distance=2.4 + 0.02 * i, phi=0.37 * i, theta=0.4 * np.sin(i)) for i in range(64)]
    _setup(fgs, screen, cams[0], gui, iters)
    trap = dict(FT.NAMED["flake"][1], scale=1.0, bias=-0.25, mid=TR.MID, far=TR.FAR)
    r = _call(fgs, kifs, fold=FR.FLAKE, trap=trap, cams=cams, count=64, plane=True)
    assert r.st == OK
    for i in (0, 1, 17, 31, 62, 63):
        lone = _lone(fgs, kifs, cams[i], fold=FR.FLAKE, trap=trap, plane=True)
        _assert_bytes(r.colour[i], lone.colour[0], ("view", i))
        assert (r.plane[i] == lone.plane[0]).all(), ("plane of view", i)
    assert len({r.colour[i].tobytes() for i in range(64)}) >= 48


@pytest.mark.parametrize("k", [1, 2, 3, 4])
def test_supersampled_samples_are_coloured_one_by_one(k, fgs, kifs, oracle):
    (screen, cam, gui, iters), fold, trap = FT.named_scene(oracle, kifs, cases, "flake", 70, 21)
    _setup(fgs, screen, cam, gui, iters, k=k)
    try:
        r = _call(fgs, kifs, fold=fold, trap=trap, ao=OR.DEFAULT)
        planed = _call(fgs, kifs, fold=fold, trap=trap, ao=OR.DEFAULT, plane=True)
    finally:
        fgs.set_supersampling(1)
    assert r.st == OK
    _assert_bytes(r.colour[0], FT.supersampled_bytes(oracle, kifs, screen, cam, gui, iters, fold, trap, k, LR.A, ao=OR.DEFAULT), k)
    if k > 1:  # a resolved pixel has no single u
        assert planed.st == BAD_ARG and planed.untouched()
    else:
        assert planed.st == OK


def test_a_launch_on_the_callers_stream(fgs, kifs, oracle):
    import torch
    scene, fold, trap = FT.named_scene(oracle, kifs, cases, "flake", W, H)
    _setup(fgs, *scene)
    want = _call(fgs, kifs, fold=fold, trap=trap, plane=True)
    s = torch.cuda.Stream(device="cuda:0")
    got = _call(fgs, kifs, fold=fold, trap=trap, plane=True, stream=s.cuda_stream)
    assert want.st == OK and got.st == OK
    _assert_bytes(got.colour[0], want.colour[0], "caller's stream")
    assert (got.plane[0] == want.plane[0]).all()


# ---- (f) the record's ring
def _ring_cases(oracle, kifs):
    """Six calls on one scene, each with a fold system and a trap of its own."""
    scene = cases(kifs, W, H)["box"]
    out = []
    for i in range(6):
        fold = dict(FR.ALL_STAGES, iterations=1 + i % 4, scale=1.6 + 0.2 * i, offset=(1.0, 0.8 - 0.05 * i, 0.6))
        trap = dict(centre=(0.2 * i, 0.5, -0.1 * i, 0.0), axes=(15, 1, 3, 7, 2, 5)[i], iterations=i, scale=0.4 + 0.1 * i, bias=-0.05 * i,
                    mid=TR.MID, far=TR.FAR)
        out.append((fold, trap))
    return scene, out


@pytest.mark.parametrize("animated", [False, True])
def test_six_calls_in_flight_each_keep_their_own_record(animated, fgs, kifs, oracle):
    """The ring that carries the record is four deep: six calls back to back with no synchronisation between them -- and,
    `animated`, an animated batch on the same ring after every one -- must each render with their own fold and trap."""
    import torch
    from kifs_raymarching_amd._lib import lib
    scene, calls = _ring_cases(oracle, kifs)
    screen, cam, gui, iters = scene
    _setup(fgs, *scene)
    want = [_model(oracle, kifs, scene, fold, trap) for fold, trap in calls]
    assert len({FT.encode(oracle, m.rgb, 1).tobytes() for m in want}) == 6
    options = [gui, kifs.GuiData(**{**gui.__dict__, "fractal_color": (30, 200, 90)})]
    # (the destinations are filled and settled beforehand: nothing between the calls waits for the device)
    buffers = [(torch.full((1, H * (4 * W + 12) + 64), SENT_U8, dtype=torch.uint8, device="cuda:0"),
                torch.full((1, H * (4 * W + 8) + 64), SENT_U8, dtype=torch.uint8, device="cuda:0")) for _ in calls]
    torch.cuda.synchronize()
    pending, frames = [], []
    for (fold, trap), b in zip(calls, buffers):
        pending.append(_enqueue(fgs, kifs, fold=fold, trap=trap, plane=True, buffers=b))
        if animated:
            frames.append(fgs.render_animation(options, cameras=[cam, cam]))
    torch.cuda.synchronize()
    assert lib.kifs_synchronize(fgs._ctx) == 0
    for i, (p, m) in enumerate(zip(pending, want)):
        r = _collect(p)
        assert r.st == OK
        _assert_bytes(r.colour[0], FT.encode(oracle, m.rgb, 1), ("call", i))
        _assert_plane(r.plane[0], m.u, ("call", i))
    if animated:
        first = frames[0].cpu().numpy()
        assert (first[0] != first[1]).any()
        for f in frames[1:]:
            assert (f.cpu().numpy() == first).all()


# ---- (g) refusals and isolation
def test_refusals_write_nothing(fgs, kifs):
    from test_gpu_lighting import _bad_lights, _bad_terms
    screen, cam, gui, iters = scene = cases(kifs, W, H)["torus"]
    _setup(fgs, *scene)
    two = [cam, cam]
    refusals = [dict(outs=None), dict(fold=None), dict(trap=None), dict(count=0, cams=[]), dict(count=65, cams=[cam] * 65),
                dict(count=2, cams=None), dict(encode=2), dict(encode=-1),
                dict(y0=-1), dict(y1=H + 1), dict(y0=10, y1=9),
                dict(cams=two, count=2, null_out=1), dict(cams=two, count=2, misalign_out=1), dict(misalign_out=0)]
    refusals += [dict(fold=f) for f in _bad_folds()]
    refusals += [dict(trap=dict(t, centre=tuple(t["centre"]))) for t in _bad_traps()]
    refusals += [dict(spec=s) for s in _bad_lights()]
    refusals += [dict(term=t) for t in _bad_terms()]
    # the plane: misaligned, a pitch below the width or no multiple of four, a stride no multiple of four or below a band
    refusals += [dict(plane_offset=2), dict(ppad=-4), dict(ppad=2), dict(pstride=6), dict(cams=two, count=2, pstride=4 * W)]
    for kw in refusals:
        r = _call(fgs, kifs, **dict(dict(plane=True), **kw))
        assert r.st == BAD_ARG, (kw, r.st)
        assert r.untouched(), kw
    r = _call(fgs, kifs, ctx=None, plane=True)
    assert r.st == BAD_ARG and r.untouched()
    for kw in (dict(cpad=-4), dict(cpad=2)):  # the colour pitch: as the batch call refuses it
        r = _call(fgs, kifs, plane=True, **kw)
        assert r.st == BAD_SIZE and r.untouched(), kw
    # the edges of the ranges are accepted
    for kw in (dict(fold=dict(FR.ALL_STAGES, iterations=24)), dict(trap=dict(FT.POINT8, iterations=32)), dict(trap=dict(FT.POINT8, iterations=0)),
               dict(fold=dict(FR.ALL_STAGES, iterations=0)), dict(spec=None), dict(ppad=0, plane=True)):
        assert _call(fgs, kifs, **kw).st == OK, kw
    # the two Julia groups have no folded form
    for name in ("julia_24", "genjulia"):
        _setup(fgs, *cases(kifs, W, H)[name])
        r = _call(fgs, kifs, plane=True)
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
            r = _call(g, kifs, plane=True)
            assert r.st == UNCONFIGURED and r.untouched()
            u = np.zeros(2, dtype=np.float32)
            p = np.zeros(6, dtype=np.float32)
            f, t = _cfold(FR.MENGER), _ctrap(FT.POINT8)
            fp = lambda a: a.ctypes.data_as(C.POINTER(C.c_float))
            assert lib.kifs_eval_fold_trap(bare, C.byref(f), C.byref(t), fp(p), 2, fp(u)) == UNCONFIGURED
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
    trap = kifs.OrbitTrap(centre=(0.0, 0.0, 0.0, 0.0), axes=3, iterations=4, scale=1.1, bias=-0.25)
    light = kifs.Light(**LR.A)
    colour, plane = fgs.render_folded_trapped_batch(cams, fold, trap, light=light, u_plane=True)
    bare = fgs.render_folded_trapped_batch(cams, fold, trap)
    fgs.synchronize()
    assert tuple(colour.shape) == (70, 24, 40, 4) and tuple(plane.shape) == (70, 24, 40) and tuple(bare.shape) == (70, 24, 40, 4)
    colour, plane = colour.cpu().numpy(), plane.cpu().numpy()
    for i in (0, 63, 64, 69):
        fgs.set_camera(cams[i])
        c, p = fgs.render_folded_trapped(fold, trap, light=light, u_plane=True)
        _assert_bytes(colour[i], c.cpu().numpy(), ("frame", i))
        assert FT.same_bits(plane[i], p.cpu().numpy()).all(), ("plane", i)
    one = _lone(fgs, kifs, cams[69], fold=fold.into_buffer_data(), trap=trap.into_buffer_data())  # ... which is the raw entry point's frame
    _assert_bytes(colour[69], one.colour[0], "raw")
    fgs.set_camera(cams[3])
    _assert_bytes(fgs.render_folded_trapped(kifs.FoldSystem(), kifs.OrbitTrap(scale=0.0)).cpu().numpy(), fgs.render(),
                  "no iterations and a neutral trap under the default light")


def test_a_long_lived_context_does_not_notice_the_call(kifs):
    """256 x 128 Sierpinski: the plain, lit, trapped and folded renders are the same bytes before and after the call, and
    the debug values and the tile order are where the plain renders left them."""
    from kifs_raymarching_amd._lib import lib
    screen, cam, gui, iters = cases(kifs, 256, 128)["sierpinski"]
    with kifs.GraphicState(0, screen_data=screen, camera_data=cam, gui_data=gui) as g:
        g.set_iters(*iters)
        fold = kifs.FoldSystem(stages=("tetra",), iterations=3)
        trap = kifs.OrbitTrap(centre=(1.0, 1.0, 1.0, 0.0), axes=7, iterations=6, scale=0.5)
        light = kifs.Light(**LR.A)

        def others():
            return [g.render().copy(), g.render_lit(light, ao=kifs.AmbientOcclusion()).cpu().numpy(),
                    g.render_trapped(trap, light=light).cpu().numpy(), g.render_folded(fold, light=light).cpu().numpy()]

        first = others()
        before = (g.debug_last_kernel(), lib.kifs_debug_last_kernel(g._ctx), g.debug_last_round_steps(), g.debug_get_tile_order())
        colour, plane = g.render_folded_trapped(fold, trap, light=light, ao=kifs.AmbientOcclusion(), u_plane=True)
        g.render_folded_trapped_batch([cam, cam, cam], fold, trap)
        g.synchronize()
        g.eval_fold_trap(fold, trap, np.zeros((5, 3), dtype=np.float32))
        after = (g.debug_last_kernel(), lib.kifs_debug_last_kernel(g._ctx), g.debug_last_round_steps(), g.debug_get_tile_order())
        assert before[:3] == after[:3] and (before[3] == after[3]).all()
        assert bool((colour.cpu().numpy() != first[3]).any()) and bool(np.isfinite(plane.cpu().numpy()).any())
        for a, b in zip(first, others()):
            assert (a == b).all()
