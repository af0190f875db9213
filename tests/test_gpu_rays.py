"""Ray queries on the GPU (kifs_trace_rays_async, kifs_rays_kernels.hip), bit for bit.  The generated rays of
tests/ray_cases.py -- interior origins, scaled and zero directions, shuffled so that the lanes of a wave hold unrelated
rays -- against the CPU restatement of the contract (tests/ray_reference.c, held to the oracle by
tests/test_ray_reference.py): every f32 bit of every texel, every colour byte, both encodes.  The pixel rays of a frame
against the library's own frame and geometry plane and the oracle's frame, plain, with heatmap and with soft shadows,
also with the rays of three cameras mixed in one call.  No tolerance anywhere: both sides run the contract's operation
sequence.  Every destination is pre-filled with a sentinel and is 64 slots longer than needed, so that a missing or a
stray store shows."""
import ctypes as C

import numpy as np
import pytest

import geometry_reference as GR
import kernel_forms as F
import ray_cases
import ray_reference as RR
from geometry_cases import PIPELINES, Raw, cases

pytestmark = pytest.mark.gpu

W, H = 64, 48
OK, UNCONFIGURED, BAD_ARG = 0, 4, 7
SENT_U8 = 0xA5
SENT_F32 = np.float32(-12345.5)
SLACK = 64
SHADOW = dict(soft_shadow=True, **F.SHADOW)


@pytest.fixture(scope="module")
def rgs(kifs):
    g = kifs.GraphicState(0)
    yield g
    g.close()


def _scene(g, gui, iters, shadow=False, heatmap=None):
    """The context's scene: options, iteration counts, extensions.  `heatmap` overrides the image's flag."""
    u = gui.u if isinstance(gui, Raw) else gui.into_buffer_data()
    if heatmap is not None:
        u.is_heatmap = 1 if heatmap else 0
    g.set_raw_uniforms(options=u)
    g.set_iters(*iters)
    g.set_extensions(**(SHADOW if shadow else dict(soft_shadow=False)))
    g.set_supersampling(1)


def _trace(ctx, rays, encode=1, geometry=True, colours=True, n=None, rays_offset=0, geom_offset=0, rgba_offset=0, null_rays=False):
    """The raw entry point on sentinel-filled destinations SLACK slots longer than needed: (status, texels (n, 4) float32
    or None, pixels (n, 4) uint8 or None); everything beyond the first n slots is asserted to hold the sentinel still, and
    after a refusal everything."""
    import torch
    from kifs_raymarching_amd._lib import lib
    rays = np.ascontiguousarray(rays, dtype=np.float32)
    n = rays.shape[0] if n is None else n
    slots = (n if 0 <= n <= rays.shape[0] else 0) + SLACK  # (a refused count allocates nothing for itself)
    d_rays = torch.from_numpy(np.concatenate([rays.reshape(-1), np.zeros(8, dtype=np.float32)])).to("cuda:0")
    geom = torch.full((slots * 4 + 4,), float(SENT_F32), dtype=torch.float32, device="cuda:0")
    rgba = torch.full((slots * 4 + 4,), SENT_U8, dtype=torch.uint8, device="cuda:0")
    torch.cuda.synchronize()
    st = lib.kifs_trace_rays_async(ctx, None, None if null_rays else d_rays.data_ptr() + rays_offset, n,
                                   geom.data_ptr() + geom_offset if geometry else None,
                                   rgba.data_ptr() + rgba_offset if colours else None, encode)
    assert lib.kifs_synchronize(ctx) == 0
    hg, hc = geom.cpu().numpy(), rgba.cpu().numpy()
    wrote = n if st == OK else 0
    assert (hg[4 * wrote if geometry else 0:].view(np.uint32) == SENT_F32.view(np.uint32)).all(), "a texel store outside the call's n"
    assert (hc[4 * wrote if colours else 0:] == SENT_U8).all(), "a colour store outside the call's n"
    if st != OK:
        return st, None, None
    return st, hg[:4 * n].reshape(n, 4) if geometry else None, hc[:4 * n].reshape(n, 4) if colours else None


def _assert_same(got, want, what):
    same = GR.same_bits(got, want)
    if not same.all():
        at = tuple(np.argwhere(~same)[0])
        pytest.fail(f"{what}: {int((~same).sum())} of {same.size} floats differ; first at {at}: "
                    f"got {got[at]!r} ({got[at].view(np.uint32):#x}), want {want[at]!r} ({want[at].view(np.uint32):#x})")


def _assert_bytes(got, want, what):
    bad = (got != want).any(-1)
    assert not bad.any(), f"{what}: {int(bad.sum())} of {bad.size} pixels differ; first at {int(np.argmax(bad))}: " \
                          f"got {got[np.argmax(bad)]}, want {want[np.argmax(bad)]}"


_REF = {}


def _reference(oracle, kifs, name, encode=1, seed=1):
    """(rays, texels, pixels) of the generated rays in scene `name`, computed once per (scene, encode, seed)."""
    key = (name, encode, seed)
    if key not in _REF:
        _, _, gui, iters = cases(kifs, W, H)[name]
        rays, _ = ray_cases.rays(seed)
        geom, rgba, _ = RR.trace_scene(oracle, kifs, gui, iters, rays, encode)
        geom.setflags(write=False)
        rgba.setflags(write=False)
        _REF[key] = (rays, geom, rgba)
    return _REF[key]


@pytest.mark.parametrize("name", PIPELINES)
@pytest.mark.parametrize("encode", [1, 0])
def test_every_pipeline_bit_exact(name, encode, rgs, kifs, oracle):
    _, _, gui, iters = cases(kifs, W, H)[name]
    _scene(rgs, gui, iters)
    rays, want_geom, want_rgba = _reference(oracle, kifs, name, encode)
    st, geom, rgba = _trace(rgs._ctx, rays, encode)
    assert st == OK
    _assert_same(geom, want_geom, name)
    _assert_bytes(rgba, want_rgba, name)
    if name != "unknown_id":
        hit = RR.hits(want_geom)
        assert hit.sum() >= 200 and (~hit).sum() >= 200


@pytest.mark.parametrize("name", PIPELINES)
@pytest.mark.parametrize("encode", [1, 0])
def test_far_and_grazing_rays_bit_exact(name, encode, rgs, kifs, oracle):
    """ray_cases.grazing: 1600 rays (genjulia: 8000, ray_cases.N_GRAZING_OF) whose lines are tangent to spheres of 0.3 to
    1.15 bounding radii, from distances 2.5, 8, 31.9 and 32.1 -- the far side of rays::never_inside, both sides of its
    |o|^2 <= 1024 switch --, direction lengths 0.5 and 1.  The reference has no cull: a ray culled wrongly is a hit turned
    into the miss texel."""
    _, _, gui, iters = cases(kifs, W, H)[name]
    _scene(rgs, gui, iters)
    key = ("grazing", name, encode)
    if key not in _REF:
        rays, dist, _ = ray_cases.grazing(3, ray_cases.BOUND[name], ray_cases.N_GRAZING_OF.get(name, ray_cases.N_GRAZING))
        geom, rgba, _ = RR.trace_scene(oracle, kifs, gui, iters, rays, encode)
        geom.setflags(write=False)
        rgba.setflags(write=False)
        _REF[key] = (rays, geom, rgba, dist)
    rays, want_geom, want_rgba, dist = _REF[key]
    st, geom, rgba = _trace(rgs._ctx, rays, encode)
    assert st == OK
    _assert_same(geom, want_geom, name)
    _assert_bytes(rgba, want_rgba, name)
    if name != "unknown_id":
        hit = RR.hits(want_geom)
        assert all(hit[dist == d].sum() >= 30 and (~hit)[dist == d].sum() >= 30 for d in ray_cases.DISTANCES)


def _oracle_frame(oracle, kifs, screen, cam, options, iters, encode, shadow):
    s = oracle.from_bytes(oracle.Screen, kifs.uniform_bytes(screen.into_buffer_data()))
    c = oracle.from_bytes(oracle.Camera, kifs.uniform_bytes(cam.into_buffer_data()))
    o = oracle.from_bytes(oracle.Options, kifs.uniform_bytes(options))
    ext = oracle.Ext(1, F.SHADOW["shadow_steps"], F.SHADOW["shadow_k"], F.SHADOW["shadow_t0"], F.SHADOW["shadow_max_t"]) if shadow else None
    return oracle.render(s, c, o, oracle.iters(*iters), encode=encode, ext=ext)


@pytest.mark.parametrize("name", PIPELINES)
def test_pixel_rays_give_the_frame_and_its_geometry_plane(name, rgs, kifs, oracle):
    """The rays of a frame's pixels through the ray call: the texels are render_geometry's plane and the colours the
    frame's bytes -- kifs_render's and the oracle's -- plain and in heatmap mode."""
    from kifs_raymarching_amd.configs import pixel_rays
    screen, cam, gui, iters = cases(kifs, W, H)[name]
    rays = pixel_rays(screen, cam)
    rgs.update_screen_data(screen)
    rgs.set_camera(cam)
    for heatmap in (False, True):
        options = gui.into_buffer_data()
        options.is_heatmap = 1 if heatmap else 0
        _scene(rgs, Raw(options), iters)
        frame = rgs.render()
        colour, plane = rgs.render_geometry()
        st, geom, rgba = _trace(rgs._ctx, rays)
        assert st == OK
        _assert_same(geom, plane.cpu().numpy().reshape(-1, 4), f"{name} heatmap={heatmap}: texels against render_geometry")
        _assert_bytes(rgba, frame.reshape(-1, 4), f"{name} heatmap={heatmap}: colours against kifs_render")
        want = _oracle_frame(oracle, kifs, screen, cam, options, iters, 1, False)
        _assert_bytes(rgba, want.reshape(-1, 4), f"{name} heatmap={heatmap}: colours against the oracle")


SHADOW_SCENES = [s for s, v in F.SCENES.items() if v.shadow]


@pytest.mark.parametrize("scene", SHADOW_SCENES)
def test_pixel_rays_give_the_shadowed_frame(scene, rgs, kifs, oracle):
    """The same with soft shadows on, for the `*_shadow` scenes of tests/kernel_forms.py (every estimate that reads the
    shader's lane mask): the secondary march from the hit point is the frame's."""
    from kifs_raymarching_amd.configs import pixel_rays
    assert len(SHADOW_SCENES) == 5
    s = F.SCENES[scene]
    screen, cam, options = kifs.ScreenData(W, H), F.camera(kifs, scene, 2), F.options(kifs, scene)
    rgs.update_screen_data(screen)
    rgs.set_camera(cam)
    _scene(rgs, Raw(options), s.iters, shadow=True)
    frame = rgs.render()
    st, _, rgba = _trace(rgs._ctx, pixel_rays(screen, cam))
    assert st == OK
    _assert_bytes(rgba, frame.reshape(-1, 4), f"{scene}: colours against kifs_render")
    want = _oracle_frame(oracle, kifs, screen, cam, options, s.iters, 1, True)
    _assert_bytes(rgba, want.reshape(-1, 4), f"{scene}: colours against the oracle")
    plain = _oracle_frame(oracle, kifs, screen, cam, options, s.iters, 1, False)
    assert (plain != want).any(), "no pixel of this frame is in shadow"


@pytest.mark.parametrize("name", ["julia_24", "sierpinski"])
def test_three_cameras_in_one_call(name, rgs, kifs, oracle):
    """The pixel rays of three cameras, concatenated and shuffled: the lanes of one wave hold different origins.  With
    soft shadows on, and once more with heatmap on, every ray's bytes are its pixel of the oracle's frame."""
    from kifs_raymarching_amd.configs import pixel_rays
    screen, cam, gui, iters = cases(kifs, W, H)[name]
    cams = [cam] + [kifs.CameraData(origin_distance=cam.origin_distance, min_distance=cam.min_distance, phi=cam.phi + 0.9 * k,
                                    theta=cam.theta + 0.25 * k) for k in (1, 2)]
    rays = np.concatenate([pixel_rays(screen, c) for c in cams])
    assert len({tuple(r) for r in rays[:, 0:3]}) == 3
    order = np.random.default_rng(20261020).permutation(rays.shape[0])
    for heatmap in (False, True):
        _scene(rgs, gui, iters, shadow=True, heatmap=heatmap)
        options = gui.into_buffer_data()
        options.is_heatmap = 1 if heatmap else 0
        want = np.concatenate([_oracle_frame(oracle, kifs, screen, c, options, iters, 1, True).reshape(-1, 4) for c in cams])
        st, _, rgba = _trace(rgs._ctx, rays[order])
        assert st == OK
        _assert_bytes(rgba, want[order], f"{name} heatmap={heatmap}")
        if not heatmap:
            plain = np.concatenate([_oracle_frame(oracle, kifs, screen, c, options, iters, 1, False).reshape(-1, 4) for c in cams])
            assert (plain != want).any(), "no pixel of these frames is in shadow"


@pytest.mark.parametrize("name", ["julia_24", "bunny"])
def test_a_rays_result_does_not_depend_on_its_neighbours(name, rgs, kifs, oracle):
    """trace(perm(rays)) == perm(trace(rays)) for a seeded permutation."""
    _, _, gui, iters = cases(kifs, W, H)[name]
    _scene(rgs, gui, iters)
    rays, _, _ = _reference(oracle, kifs, name)
    perm = np.random.default_rng(7).permutation(rays.shape[0])
    _, geom, rgba = _trace(rgs._ctx, rays)
    st, pgeom, prgba = _trace(rgs._ctx, rays[perm])
    assert st == OK
    _assert_same(pgeom, geom[perm], name)
    _assert_bytes(prgba, rgba[perm], name)


@pytest.mark.parametrize("n", [1, 63, 64, 65, 255, 256, 257, 1000])
def test_sizes_around_a_wave_and_a_workgroup(n, rgs, kifs, oracle):
    """The first n slots equal the reference, everything beyond is the sentinel (checked by _trace)."""
    _, _, gui, iters = cases(kifs, W, H)["sierpinski"]
    _scene(rgs, gui, iters)
    rays, want_geom, want_rgba = _reference(oracle, kifs, "sierpinski")
    st, geom, rgba = _trace(rgs._ctx, rays[:n])
    assert st == OK
    _assert_same(geom, want_geom[:n], f"n={n}")
    _assert_bytes(rgba, want_rgba[:n], f"n={n}")
    # fewer rays than the array holds: the count is the argument, not the allocation
    st, geom, rgba = _trace(rgs._ctx, rays[:n + 70], n=n)
    assert st == OK
    _assert_same(geom, want_geom[:n], f"n={n} of {n + 70}")
    _assert_bytes(rgba, want_rgba[:n], f"n={n} of {n + 70}")


@pytest.mark.parametrize("name", ["julia_25", "torus"])
def test_either_output_alone_is_the_call_with_both(name, rgs, kifs, oracle):
    _, _, gui, iters = cases(kifs, W, H)[name]
    _scene(rgs, gui, iters, shadow=True)
    rays, _, _ = _reference(oracle, kifs, name)
    for encode in (1, 0):
        _, geom, rgba = _trace(rgs._ctx, rays, encode)
        st, only_geom, none = _trace(rgs._ctx, rays, encode, colours=False)
        assert st == OK and none is None
        _assert_same(only_geom, geom, f"{name}: geometry only")
        st, none, only_rgba = _trace(rgs._ctx, rays, encode, geometry=False)
        assert st == OK and none is None
        _assert_bytes(only_rgba, rgba, f"{name}: colour only")


def test_a_context_without_screen_or_camera_and_any_supersampling(kifs, oracle):
    """The call reads options, iteration counts and extensions only: a context that never had kifs_set_screen or
    kifs_set_camera called gives the reference's bits, and so does one with a 3 x 3 supersampling factor."""
    from kifs_raymarching_amd._lib import lib
    _, _, gui, iters = cases(kifs, W, H)["julia_24"]
    rays, want_geom, want_rgba = _reference(oracle, kifs, "julia_24")
    st = C.c_int(0)
    ctx = lib.kifs_create(0, C.byref(st))
    assert ctx and st.value == OK
    try:
        assert _trace(ctx, rays)[0] == UNCONFIGURED  # options never set
        u = gui.into_buffer_data()
        assert lib.kifs_set_options(ctx, C.byref(u)) == OK and lib.kifs_set_iters(ctx, *iters) == OK
        for factor in (1, 3):
            assert lib.kifs_set_supersampling(ctx, factor) == OK
            st, geom, rgba = _trace(ctx, rays)
            assert st == OK
            _assert_same(geom, want_geom, f"no screen, supersampling {factor}")
            _assert_bytes(rgba, want_rgba, f"no screen, supersampling {factor}")
        # the context still has no screen: a render is refused as before
        assert lib.kifs_render_async(ctx, None, 16, 64, 0, 1, 1) == UNCONFIGURED
    finally:
        lib.kifs_destroy(ctx)


def test_a_trace_leaves_the_render_state_alone(kifs, oracle):
    """On a context that renders: a batch before and after the trace gives the same bytes, and the launch-state hooks
    report what they reported before it."""
    import torch
    screen, cam, gui, iters = cases(kifs, 330, 149)["julia_24"]
    rays, want_geom, _ = _reference(oracle, kifs, "julia_24")
    with kifs.GraphicState(0, screen_data=screen, camera_data=cam, gui_data=gui) as g:
        g.set_iters(*iters)
        cams = [kifs.CameraData(origin_distance=3.0, phi=0.3 + 0.2 * k) for k in range(4)]
        outs = [torch.zeros((149, 330, 4), dtype=torch.uint8, device="cuda:0") for _ in cams]

        def batch():
            for o in outs:
                o.fill_(SENT_U8)
            g.render_batch_async(outs, cams)
            g.synchronize()
            return [o.cpu().numpy() for o in outs]

        before = batch()
        state = (g.debug_last_kernel(), g.debug_last_round_steps(), g.debug_last_group_tiles(), g.debug_get_tile_order().tolist())
        st, geom, _ = _trace(g._ctx, rays)
        assert st == OK
        _assert_same(geom, want_geom, "on a rendering context")
        assert (g.debug_last_kernel(), g.debug_last_round_steps(), g.debug_last_group_tiles(), g.debug_get_tile_order().tolist()) == state
        after = batch()
        for a, b in zip(before, after):
            assert (a == b).all()


def test_refusals_write_nothing(rgs, kifs, oracle):
    """Every refusal returns its status and leaves the sentinel-filled outputs untouched (checked by _trace)."""
    _, _, gui, iters = cases(kifs, W, H)["sphere"]
    _scene(rgs, gui, iters)
    rays = ray_cases.rays(1)[0][:300]
    ctx = rgs._ctx
    assert _trace(ctx, rays)[0] == OK
    assert _trace(ctx, rays, n=-1)[0] == BAD_ARG
    assert _trace(ctx, rays, n=(1 << 28) + 1)[0] == BAD_ARG
    assert _trace(ctx, rays, null_rays=True)[0] == BAD_ARG
    assert _trace(ctx, rays, null_rays=True, n=0)[0] == BAD_ARG
    for off in (4, 8, 12):
        assert _trace(ctx, rays, n=299, rays_offset=off)[0] == BAD_ARG
        assert _trace(ctx, rays, n=299, geom_offset=off)[0] == BAD_ARG
    for off in (1, 2, 3):
        assert _trace(ctx, rays, n=299, rgba_offset=off)[0] == BAD_ARG
    assert _trace(ctx, rays, geometry=False, colours=False)[0] == BAD_ARG
    for encode in (-1, 2, 7):
        assert _trace(ctx, rays, encode)[0] == BAD_ARG
    st, geom, rgba = _trace(ctx, rays, n=0)  # nothing to do: OK, nothing enqueued, nothing written
    assert st == OK and geom.shape == (0, 4) and rgba.shape == (0, 4)
    from kifs_raymarching_amd._lib import lib
    assert lib.kifs_trace_rays_async(None, None, 16, 1, 16, 16, 1) == BAD_ARG


@pytest.mark.parametrize("name", ["julia_24", "genjulia", "bunny"])
def test_non_finite_rays_keep_to_themselves(name, rgs, kifs, oracle):
    """Eight rays with a NaN or an infinite component scattered among 512 finite ones: the call returns, and the finite
    rays' words are those of the call without the eight."""
    _, _, gui, iters = cases(kifs, W, H)[name]
    _scene(rgs, gui, iters)
    rays, want_geom, want_rgba = _reference(oracle, kifs, name)
    rays, want_geom, want_rgba = rays[:512], want_geom[:512], want_rgba[:512]
    nan, inf = np.float32(np.nan), np.float32(np.inf)
    bad = np.array([[nan, 0, 0, 0, 1, 0, 0, 0], [0, 3, 0, 0, 0, nan, 0, 0], [inf, 0, 0, 0, -1, 0, 0, 0], [3, 0, 0, 0, -inf, 0, 0, 0],
                    [0, 0, -inf, 0, 0, 0, inf, 0], [nan, nan, nan, 0, nan, nan, nan, 0], [0.1, 0.2, 0.3, 0, inf, inf, inf, 0],
                    [2.5, 0, 0, 0, -1, 0, nan, 0]], dtype=np.float32)
    at = np.array([0, 63, 64, 130, 255, 256, 300, 519])  # positions in the mixed array, ascending
    mixed = np.zeros((520, 8), dtype=np.float32)
    finite = np.ones(520, dtype=bool)
    finite[at] = False
    mixed[at] = bad
    mixed[finite] = rays
    st, geom, rgba = _trace(rgs._ctx, mixed)
    assert st == OK
    _assert_same(geom[finite], want_geom, name)
    _assert_bytes(rgba[finite], want_rgba, name)
