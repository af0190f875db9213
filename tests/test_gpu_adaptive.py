"""Adaptive anti-aliasing on the GPU (kifs_render_adaptive_async, kifs_adaptive_kernels.hip), byte for byte: off the
edge mask the frame is the oracle's plain frame, on it the oracle's k x k resolve, and the edge count is the mask's
(tests/adaptive_reference.py, held to the oracle by tests/test_adaptive_reference.py).  No tolerance anywhere.  Frames
are 74 x 45 -- ragged tiles, 74 % 32 = 10 and 45 % 8 = 5 -- and every destination is pre-filled with a sentinel so that
a missing store shows.  The seeded scenes of tests/extension_fuzz_cases.py run the same comparison at frames narrower than
one classify row of 64 pixels and lower than 4 k rows, from cameras inside, on and just outside the bounding sphere, with
four kinds of thresholds, lone and in batches."""
import ctypes as C

import numpy as np
import pytest

import adaptive_reference as AR
import extension_fuzz_cases as X
import extension_fuzz_support as S
from geometry_cases import PIPELINES, Raw, cases
from helpers import oracle_frame, oracle_uniforms

pytestmark = pytest.mark.gpu

W, H = 74, 45
BAD_SIZE, UNCONFIGURED, BAD_ARG = 3, 4, 7
SENT = 0xA5
SENT_COUNT = 0x5A5A5A5A


@pytest.fixture(scope="module")
def ags(kifs):
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


def _call(g, kifs, k=2, th=AR.SILHOUETTE, cams=None, count=1, encode=1, pitch=None, counts=True, aa=True, outs=True):
    """The raw entry point on sentinel-filled destinations: (status, frames (count, H, pitch) uint8 -- whole rows, padding
    included --, edge counts (count,) or None)."""
    import torch
    from kifs_raymarching_amd._lib import AdaptiveAAC, lib
    w, h = g.screen_data.width, g.screen_data.height
    pitch = 4 * w if pitch is None else pitch
    colour = torch.full((count, h * pitch + 64,), SENT, dtype=torch.uint8, device="cuda:0")
    edge = torch.full((count,), SENT_COUNT, dtype=torch.int32, device="cuda:0")
    torch.cuda.synchronize()
    ptrs = (C.c_void_p * count)(*[colour[i].data_ptr() for i in range(count)]) if outs else None
    arr = None if cams is None else kifs.camera_array(cams)
    par = AdaptiveAAC(int(k), th[0], th[1])
    st = lib.kifs_render_adaptive_async(g._ctx, None, count, arr, ptrs, pitch, C.byref(par) if aa else None,
                                        edge.data_ptr() if counts else None, encode)
    assert lib.kifs_synchronize(g._ctx) == 0
    host = colour.cpu().numpy()
    assert (host[:, h * pitch:] == SENT).all()  # nothing past the last row
    return st, host[:, :h * pitch].reshape(count, h, pitch), edge.cpu().numpy()


def _pixels(rows, w):
    """(H, pitch) bytes -> (H, W, 4)."""
    return rows[:, :4 * w].reshape(rows.shape[0], w, 4)


_GEOM, _MEANS = {}, {}


def _expected(oracle, kifs, key, scene, k, th, encode=1):
    """expected_frame with the scene's geometry plane and its resolved means shared between the tests (key names the scene)."""
    screen, cam, gui, iters = scene
    if key not in _GEOM:
        _GEOM[key] = AR.geometry(oracle, kifs, screen, cam, gui, iters)
    return AR.expected_frame(oracle, kifs, screen, cam, gui, iters, k, th[0], th[1], encode, geom=_GEOM[key],
                             means=_MEANS.setdefault(key, {}))


def _check(got, count, want, mask, what):
    frame = _pixels(got, want.shape[1])
    bad = (frame != want).any(-1)
    assert not bad.any(), (what, int(bad.sum()), "pixels differ;", int((bad & mask).sum()), "of them edge pixels; first at",
                           tuple(np.argwhere(bad)[0]))
    assert int(count) == int(mask.sum()), what


def _distance(kifs, scene, distance):
    screen, cam, gui, iters = scene
    return screen, kifs.CameraData(origin_distance=distance, phi=cam.phi, theta=cam.theta), gui, iters


@pytest.mark.parametrize("name", PIPELINES)
@pytest.mark.parametrize("k,encode", [(2, 1), (2, 0), (3, 1), (4, 0)])
def test_every_pipeline_bit_exact(name, k, encode, ags, kifs, oracle):
    """Silhouette-only thresholds.  k = 3 leaves a lane of every wave idle and the queues are no multiple of 7 long."""
    scene = cases(kifs, W, H)[name]
    _setup(ags, *scene)
    st, got, counts = _call(ags, kifs, k=k, encode=encode)
    assert st == 0
    assert ags.debug_last_kernel() == "render_adaptive_kernel"
    want, mask = _expected(oracle, kifs, name, scene, k, AR.SILHOUETTE, encode)
    _check(got[0], counts[0], want, mask, (name, k, encode))
    if name == "unknown_id":  # the empty queue: the plain frame
        assert counts[0] == 0 and (_pixels(got[0], W) == ags.render(encode=encode)).all()
    else:
        assert mask.sum() % 7 != 0
        assert (want != oracle_frame(oracle, kifs, *scene, encode=encode)).any()


@pytest.mark.parametrize("name", ["julia_24", "sphere", "sierpinski"])
def test_default_thresholds(name, ags, kifs, oracle):
    scene = cases(kifs, W, H)[name]
    _setup(ags, *scene)
    st, got, counts = _call(ags, kifs, k=2, th=AR.DEFAULT)
    assert st == 0
    want, mask = _expected(oracle, kifs, name, scene, 2, AR.DEFAULT)
    assert mask.sum() > AR.edge_mask(_GEOM[name], *AR.SILHOUETTE).sum()  # creases, not only the silhouette
    _check(got[0], counts[0], want, mask, name)


def test_every_hit_is_an_edge(ags, kifs, oracle):
    scene = cases(kifs, W, H)["julia_25"]
    _setup(ags, *scene)
    st, got, counts = _call(ags, kifs, k=2, th=AR.ALL_HITS)
    assert st == 0
    want, mask = _expected(oracle, kifs, "julia_25", scene, 2, AR.ALL_HITS)
    assert (mask[_GEOM["julia_25"][..., 3].view(np.uint32) != AR.MISS_T]).all()
    _check(got[0], counts[0], want, mask, "all hits")


@pytest.mark.parametrize("name,distance,k", [("sierpinski", 1.1, 3), ("julia_24", 1.1, 2), ("box", 1.3, 2)])
def test_border_and_degenerate_masks(name, distance, k, ags, kifs, oracle):
    """Edge pixels in the frame's first and last rows and columns; nearly every pixel an edge; a camera inside the box:
    every pixel hits at t = 0 and none is an edge."""
    scene = _distance(kifs, cases(kifs, W, H)[name], distance)
    _setup(ags, *scene)
    st, got, counts = _call(ags, kifs, k=k, th=AR.DEFAULT)
    assert st == 0
    want, mask = _expected(oracle, kifs, (name, distance), scene, k, AR.DEFAULT)
    if name == "sierpinski":
        assert mask[0].any() and mask[-1].any() and mask[:, 0].any() and mask[:, -1].any()
    elif name == "julia_24":
        assert mask.sum() == 2596
    else:
        assert not mask.any() and (_pixels(got[0], W) == ags.render()).all()
    _check(got[0], counts[0], want, mask, (name, distance))


def test_heatmap_frames_resolve_heatmap_colours(ags, kifs, oracle):
    screen, cam, gui, iters = cases(kifs, W, H)["julia_24"]
    heat = kifs.GuiData(**{**gui.__dict__, "is_heatmap": True, "fractal_color": (255, 128, 30)})
    scene = (screen, cam, heat, iters)
    _setup(ags, *scene)
    st, got, counts = _call(ags, kifs, k=2, th=AR.DEFAULT)
    assert st == 0
    want, mask = _expected(oracle, kifs, "julia_24_heatmap", scene, 2, AR.DEFAULT)
    # the mask is the primary ray's geometry, which the heatmap does not change
    assert (mask == AR.edge_mask(AR.geometry(oracle, kifs, screen, cam, gui, iters), *AR.DEFAULT)).all() and mask.any()
    _check(got[0], counts[0], want, mask, "heatmap")


def test_soft_shadows_apply_per_sample(ags, kifs, oracle):
    """Off the mask: the oracle's frame with the extension.  On it: the bytes of the context's own supersampled render with
    the extension, each within +-1 of the range of its k^2 samples' bytes in the oracle's virtual frame (as
    tests/test_gpu_ssaa.py holds that render)."""
    import aa_reference as AA
    k = 2
    scene = cases(kifs, W, H)["sierpinski"]
    screen, cam, gui, iters = scene
    ext = dict(soft_shadow=True, shadow_steps=64, shadow_k=8.0, shadow_t0=0.02, shadow_max_t=10.0)
    s, c, o = oracle_uniforms(oracle, kifs, (screen, cam, gui))
    oext = oracle.Ext(1, 64, 8.0, 0.02, 10.0)
    shadowed = oracle.render(s, c, o, oracle.iters(*iters), ext=oext)
    virt = oracle.render(AA.virtual_screen(oracle, s, k), c, o, oracle.iters(*iters), ext=oext).astype(np.int16)
    blocks = virt.reshape(H, k, W, k, 4)
    lo, hi = blocks.min(axis=(1, 3)), blocks.max(axis=(1, 3))
    _, mask = _expected(oracle, kifs, "sierpinski", scene, k, AR.DEFAULT)
    _setup(ags, *scene)
    ags.set_extensions(**ext)
    try:
        st, got, counts = _call(ags, kifs, k=k, th=AR.DEFAULT)
        ags.set_supersampling(k)
        full = ags.render()
    finally:
        ags.set_supersampling(1)
        ags.set_extensions(soft_shadow=False)
    assert st == 0 and counts[0] == mask.sum()
    frame = _pixels(got[0], W)
    assert (frame[~mask] == shadowed[~mask]).all()
    assert (frame[mask] == full[mask]).all()
    f16 = frame.astype(np.int16)
    assert ((f16 >= lo - 1) & (f16 <= hi + 1))[mask].all()
    assert (shadowed != oracle_frame(oracle, kifs, *scene)).any() and (full[mask] != shadowed[mask]).any()


def _away(cam):
    u = cam.into_buffer_data()
    for r in range(3):  # (the view direction is minus the first column)
        u.matrix[0][r] = -u.matrix[0][r]
    return u


def test_batch_frames_equal_the_lone_calls(ags, kifs, oracle):
    """Five cameras with different edge counts, one of them looking away from the scene, in one call."""
    screen, _, gui, iters = cases(kifs, W, H)["sierpinski"]
    poses = [kifs.CameraData(origin_distance=d, phi=p, theta=t) for d, p, t in
             ((3.0, 1.0, 0.3), (2.2, 0.2, -0.4), (4.5, 2.0, 0.1), (1.6, 0.7, 0.6))]
    cams = [poses[0].into_buffer_data(), poses[1].into_buffer_data(), _away(poses[2]), poses[2].into_buffer_data(),
            poses[3].into_buffer_data()]
    _setup(ags, screen, poses[0], gui, iters)
    st, got, counts = _call(ags, kifs, k=2, th=AR.DEFAULT, cams=cams, count=5)
    assert st == 0
    assert counts[2] == 0 and len(set(counts.tolist())) == 5
    for i, cam in enumerate(cams):
        ags.set_raw_uniforms(camera=cam)
        st1, lone, c1 = _call(ags, kifs, k=2, th=AR.DEFAULT)  # cameras NULL, count 1: the context's camera
        assert st1 == 0 and (got[i] == lone[0]).all() and counts[i] == c1[0], i
        st2, explicit, c2 = _call(ags, kifs, k=2, th=AR.DEFAULT, cams=[cam], count=1)
        assert st2 == 0 and (explicit[0] == lone[0]).all() and c2[0] == c1[0], i
    # the lone call of the context's camera is the model's frame for that camera
    ags.set_camera(poses[1])
    _, lone, c1 = _call(ags, kifs, k=2, th=AR.DEFAULT)
    want, mask = _expected(oracle, kifs, "sierpinski_pose1", (screen, poses[1], gui, iters), 2, AR.DEFAULT)
    _check(lone[0], c1[0], want, mask, "context camera")
    # without counts the frames are the same
    st, again, untouched = _call(ags, kifs, k=2, th=AR.DEFAULT, cams=cams, count=5, counts=False)
    assert st == 0 and (again == got).all() and (untouched == SENT_COUNT).all()


def test_batch_beyond_the_inline_views(ags, kifs):
    """65 views: more than one round of the three passes over the same scratch memory."""
    screen, _, gui, iters = cases(kifs, 40, 24)["julia_24"]
    cams = [kifs.CameraData(origin_distance=2.6 + 0.02 * i, phi=0.37 * i, theta=0.2 * np.sin(i)) for i in range(65)]
    _setup(ags, screen, cams[0], gui, iters)
    st, got, counts = _call(ags, kifs, k=3, th=AR.DEFAULT, cams=cams, count=65)
    assert st == 0
    assert len(set(counts.tolist())) > 8 and counts.min() > 0
    for i, cam in enumerate(cams):
        ags.set_camera(cam)
        st1, lone, c1 = _call(ags, kifs, k=3, th=AR.DEFAULT)
        assert st1 == 0 and (got[i] == lone[0]).all() and counts[i] == c1[0], i


def test_rounds_under_the_scratch_cap(kifs):
    """Seven 4096 x 4096 views: at 20 bytes a pixel and view only six fit the 2 GiB cap on the scratch block, so the call
    runs as two rounds of 4 and 3 views over one block of 1.25 GiB -- the smallest shape at which the cap, not the kernel
    argument's 64 views, decides the rounds and leaves them uneven (below 1.68 Mpixel a view it never binds).  Every frame
    and count equals the same view's lone call on a second context, on the device; one frame of the second round is the
    plain batch frame wherever the model's mask of its own geometry plane is false, and its count is that mask's.  No
    oracle frame at this size."""
    import torch
    w = h = 4096
    views = 7
    screen, _, gui, iters = cases(kifs, w, h)["julia_24"]
    cams = [kifs.CameraData(origin_distance=2.3 + 0.2 * i, phi=0.55 * i, theta=0.12 * (i - 3)) for i in range(views)]
    th = AR.DEFAULT
    with kifs.GraphicState(0, screen_data=screen, camera_data=cams[0], gui_data=gui) as g, \
            kifs.GraphicState(0, screen_data=screen, camera_data=cams[0], gui_data=gui) as lone:
        g.set_iters(*iters)
        lone.set_iters(*iters)
        colour = torch.full((views, h, w, 4), SENT, dtype=torch.uint8, device="cuda:0")
        counts = torch.full((views,), SENT_COUNT, dtype=torch.int32, device="cuda:0")
        one = torch.full((1, h, w, 4), SENT, dtype=torch.uint8, device="cuda:0")
        count1 = torch.full((1,), SENT_COUNT, dtype=torch.int32, device="cuda:0")
        torch.cuda.synchronize()
        g.render_adaptive_batch(cams, k=2, normal_cos=th[0], depth_rel=th[1], colour=colour, edge_counts=counts)
        g.synchronize()
        assert g.debug_last_kernel() == "render_adaptive_kernel"
        got_counts = counts.cpu().numpy()
        assert got_counts.min() > 0 and len(set(got_counts.tolist())) == views
        for i, cam in enumerate(cams):
            lone.set_camera(cam)
            lone.render_adaptive_batch(None, k=2, normal_cos=th[0], depth_rel=th[1], colour=one, edge_counts=count1)
            lone.synchronize()
            assert torch.equal(colour[i], one[0]), f"view {i}: {int((colour[i] != one[0]).any(-1).sum())} pixels differ"
            assert int(got_counts[i]) == int(count1.item()), i
        # view 5, the second round's second: its plain pixels, and its count against the mask
        v = 5
        _, geometry = lone.render_geometry_batch([cams[v]])
        plain = torch.empty((h, w, 4), dtype=torch.uint8, device="cuda:0")
        lone.render_batch_async([plain], [cams[v]])
        lone.synchronize()
        mask = torch.from_numpy(AR.edge_mask(geometry[0].cpu().numpy(), *th)).to("cuda:0")
        assert int(mask.sum().item()) == int(got_counts[v])
        differs = (colour[v] != plain).any(-1)
        assert not (differs & ~mask).any() and (differs & mask).any()


def test_padded_pitch_is_left_alone(ags, kifs, oracle):
    scene = cases(kifs, W, H)["torus"]
    _setup(ags, *scene)
    pitch = 4 * W + 40
    st, got, counts = _call(ags, kifs, k=2, th=AR.DEFAULT, pitch=pitch)
    assert st == 0
    want, mask = _expected(oracle, kifs, "torus", scene, 2, AR.DEFAULT)
    _check(got[0], counts[0], want, mask, "pitch")
    assert (got[0][:, 4 * W:] == SENT).all()


def test_refusals_write_nothing(ags, kifs):
    from kifs_raymarching_amd._lib import AdaptiveAAC, lib
    scene = cases(kifs, W, H)["torus"]
    _setup(ags, *scene)
    nan, inf = float("nan"), float("inf")
    cam = scene[1]

    def refused(status, **kw):
        st, got, counts = _call(ags, kifs, **kw)
        assert st == status, kw
        assert (got == SENT).all() and (counts == SENT_COUNT).all(), kw

    for k in (1, 0, 5, -2):
        refused(BAD_ARG, k=k)
    refused(BAD_ARG, th=(nan, 0.05))
    refused(BAD_ARG, th=(0.9, nan))
    refused(BAD_ARG, th=(0.9, -0.001))
    refused(BAD_ARG, aa=False)
    refused(BAD_ARG, outs=False)
    refused(BAD_ARG, pitch=4 * W - 4)
    refused(BAD_ARG, pitch=4 * W + 2)
    refused(BAD_ARG, count=2)                      # cameras NULL stands for one frame
    refused(BAD_ARG, cams=[], count=0)
    refused(BAD_ARG, encode=2)
    ags.set_supersampling(2)
    try:
        refused(BAD_ARG)
    finally:
        ags.set_supersampling(1)
    aa = AdaptiveAAC(2, 0.9, 0.05)
    outs = (C.c_void_p * 1)(0)
    assert lib.kifs_render_adaptive_async(None, None, 1, None, outs, 4 * W, C.byref(aa), None, 1) == BAD_ARG
    assert lib.kifs_render_adaptive_async(ags._ctx, None, 1, None, outs, 4 * W, C.byref(aa), None, 1) == BAD_ARG  # a null frame
    # +inf is a depth threshold, and -inf / +inf are normal thresholds
    st, _, counts = _call(ags, kifs, th=(-inf, inf))
    assert st == 0 and counts[0] > 0
    st, _, _ = _call(ags, kifs, cams=[cam], count=1, th=(inf, 0.0))
    assert st == 0
    with kifs.GraphicState(0) as fresh:  # nothing set yet
        fresh.screen_data = kifs.ScreenData(W, H)
        st, got, counts = _call(fresh, kifs)
        assert st == UNCONFIGURED and (got == SENT).all() and (counts == SENT_COUNT).all()


def test_virtual_screen_beyond_the_limit(kifs):
    screen, cam, gui, iters = cases(kifs, 20000, 8)["sphere"]
    with kifs.GraphicState(0, screen_data=screen, camera_data=cam, gui_data=gui) as g:
        st, got, counts = _call(g, kifs, k=4)  # 4 x 20000 > 65536
        assert st == BAD_SIZE and (got == SENT).all() and (counts == SENT_COUNT).all()
        st, got, counts = _call(g, kifs, k=3)
        assert st == 0 and not (got == SENT).all()


def test_no_side_effects_on_the_plain_path(kifs):
    """A 720p Julia frame has enough tiles for the tile-cost feedback: adaptive calls in between neither record costs nor
    move the sort, and the plain frames around them are the same bytes from the same kernel."""
    from kifs_raymarching_amd._lib import lib
    screen, cam, gui, iters = cases(kifs, 1280, 720)["julia_24"]
    with kifs.GraphicState(0, screen_data=screen, camera_data=cam, gui_data=gui) as g:
        g.set_iters(*iters)
        frames = [g.render() for _ in range(5)]
        assert all((f == frames[0]).all() for f in frames)
        kernel = g.debug_last_kernel()
        before = g.debug_get_tile_order()
        for _ in range(4):
            colour, edges = g.render_adaptive(k=2)
            assert g.debug_last_kernel() == "render_adaptive_kernel" and lib.kifs_debug_last_kernel(g._ctx) == 7
            assert (g.debug_get_tile_order() == before).all()
        got = colour.cpu().numpy()
        differs = (got != frames[0]).any(-1)
        assert 0 < differs.sum() <= edges < 0.1 * differs.size  # only edge pixels changed, and they are few
        after = g.render()
        assert (after == frames[0]).all() and g.debug_last_kernel() == kernel != "render_adaptive_kernel"


def test_scratch_regrowth_after_a_larger_screen(kifs, oracle):
    small = cases(kifs, W, H)["sphere"]
    large = cases(kifs, 150, 94)["sphere"]
    with kifs.GraphicState(0, screen_data=small[0], camera_data=small[1], gui_data=small[2]) as g:
        g.set_iters(*small[3])
        st, got, counts = _call(g, kifs, k=2, th=AR.DEFAULT)
        assert st == 0
        want, mask = _expected(oracle, kifs, "sphere", small, 2, AR.DEFAULT)
        _check(got[0], counts[0], want, mask, "small")
        g.update_screen_data(large[0])
        st, got, counts = _call(g, kifs, k=2, th=AR.DEFAULT)
        assert st == 0
        want, mask = _expected(oracle, kifs, "sphere_150x94", large, 2, AR.DEFAULT)
        _check(got[0], counts[0], want, mask, "large")
        colour, edges = g.render_adaptive(k=2)  # the Python form: the same frame, the same count
        assert edges == mask.sum() and (colour.cpu().numpy() == want).all()


def test_calls_of_one_context_on_two_streams(kifs):
    """The scratch planes, queues and counters belong to the context: a call on another stream is ordered after the
    previous call by the library, so two calls enqueued back to back on two streams give the frames and counts of the
    same calls made one at a time.  (Every hit an edge, k = 4: the first call's last pass is still running when the
    second is enqueued.)"""
    import torch
    from kifs_raymarching_amd._lib import AdaptiveAAC, lib
    w, h = 320, 180
    screen, _, gui, iters = cases(kifs, w, h)["julia_24"]
    cams = [kifs.CameraData(origin_distance=2.2, phi=0.3), kifs.CameraData(origin_distance=2.6, phi=1.4, theta=0.3)]
    par = AdaptiveAAC(4, *AR.ALL_HITS)
    with kifs.GraphicState(0, screen_data=screen, camera_data=cams[0], gui_data=gui) as g:
        g.set_iters(*iters)
        streams = [torch.cuda.Stream(), torch.cuda.Stream()]

        def run(order):
            """The two calls in `order` (pairs of camera, stream index or None for the context's), no wait in between."""
            colour = torch.full((2, h, w, 4), SENT, dtype=torch.uint8, device="cuda:0")
            edge = torch.full((2,), SENT_COUNT, dtype=torch.int32, device="cuda:0")
            torch.cuda.synchronize()
            for i, s in order:
                g.set_camera(cams[i])
                ptrs = (C.c_void_p * 1)(colour[i].data_ptr())
                handle = None if s is None else streams[s].cuda_stream
                assert lib.kifs_render_adaptive_async(g._ctx, handle, 1, None, ptrs, 4 * w, C.byref(par),
                                                      edge[i:].data_ptr(), 1) == 0
            torch.cuda.synchronize()
            return colour.cpu().numpy(), edge.cpu().numpy()

        want, counts = [], []
        for i in range(2):  # one at a time, on the context's stream
            colour, edge = run([(i, None)])
            want.append(colour[i])
            counts.append(edge[i])
        assert counts[0] != counts[1] and min(counts) > 1000
        for order in ([(0, 0), (1, 1)], [(1, None), (0, 0)], [(0, 1), (1, None)]):
            colour, edge = run(order)
            for i in range(2):
                assert (colour[i] == want[i]).all() and edge[i] == counts[i], (order, i)


@pytest.mark.parametrize("index", range(X.N))
def test_fuzz_scene_bit_exact(index, ags, kifs, oracle):
    """A seeded scene at k = 2 + index % 3 and its thresholds, lone; every third one also as a 3-view batch that mixes
    camera families, with a count per view.  Every fourth scene runs with soft shadows, against the oracle's frame and
    resolve with the extension (kor_shade_pixel_ext): bit for bit like the rest."""
    scene = X.scenes(kifs)[index]
    name, family, screen, cam, gui, iters, encode = scene
    w, h, k, th = screen.width, screen.height, X.supersampling(index), X.thresholds(index)
    what = f"{S.describe(index, scene)}; k {k}, thresholds {th}"
    shadow = S.shadow_of(oracle, kifs, index)
    pitch = 4 * w + (40 if index % 2 else 0)
    launches = [None] + ([X.batch_cameras(kifs, index, scene, 0xada)] if X.has_batch(index) else [])
    S.setup(ags, screen, cam, gui, iters, shadow=shadow)
    try:
        results = []
        for cams in launches:
            results.append(_call(ags, kifs, k=k, th=th, cams=cams, count=1 if cams is None else len(cams), encode=encode,
                                 pitch=pitch))
            assert ags.debug_last_kernel() == "render_adaptive_kernel", what
    finally:
        ags.set_extensions(soft_shadow=False)
    for cams, (st, got, counts) in zip(launches, results):
        assert st == 0, what
        assert (got[:, :, 4 * w:] == SENT).all(), f"{what}: the padding of the rows"
        for v, c in enumerate([cam] if cams is None else cams):
            want, mask = AR.expected_frame(oracle, kifs, screen, c, gui, iters, k, th[0], th[1], encode,
                                           geom=S.geometry(oracle, kifs, index)[0] if v == 0 else None,
                                           ext=X.oracle_ext(oracle, shadow))
            _check(got[v], counts[v], want, mask, f"{what}; view {v} of {len(got)} ({c})")
